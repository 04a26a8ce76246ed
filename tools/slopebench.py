"""Timing of the slopes of whole streams (moihgp_slope_stream) at C3's shape: 4096 latents x 10^4 ticks, Matern-5/2, against a whole smooth call and
the off-grid smoother whose sweeps they run.

Prints one line per (dtype, cache state, call) with the median, the quartiles and the extremes of the event-timed duration of whole calls: smooth
(forward + backward + the small status kernel), interpolate K=1 and K=3 (tables + both sweeps + status kernel), slope "all" K=1 and K=3 (the same
kernels behind slope_tables_kernel) and slope "past" K=1 (tables + the forward sweep + status kernel).  The calls of one line-up alternate, so that
drift of the machine hits them alike; the spread of `interpolate` over its own repeats is what a gap between it and slope "all" is read against.
--other-lib PATH adds `smooth (other)`: the same smooth call through another build of the library (say the parent commit's), loaded beside this one
and timed in the same alternation.  "cold" evicts the caches between calls by writing a 2 GB buffer; "resident" repeats the call on the same
buffers.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split (slope_tables_kernel beside interp_tables_kernel)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multioutputihgp_amd.streams import KERNEL_ID, LatentBank, _stream_ptr  # noqa: E402


class OtherSmoother:
    """moihgp_smooth_stream of another build of the library, on a handle of its own with the same parameters."""

    def __init__(self, path, dt, prm, kernel):
        lib = C.CDLL(path)
        lib.moihgp_new_latents.restype = C.c_void_p
        lib.moihgp_new_latents.argtypes = [C.c_int, C.c_double, C.c_size_t, C.POINTER(C.c_double)]
        lib.moihgp_del.restype = None
        lib.moihgp_del.argtypes = [C.c_void_p]
        lib.moihgp_smooth_stream.restype = C.c_int
        lib.moihgp_smooth_stream.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p]
        p = np.ascontiguousarray(prm, dtype=np.float64)
        self.lib, self.h = lib, lib.moihgp_new_latents(KERNEL_ID[kernel], float(dt), p.shape[0], p.ctypes.data_as(C.POINTER(C.c_double)))
        if not self.h:
            raise RuntimeError(f"{path}: moihgp_new_latents failed")

    def smooth(self, Ty, x, ys, status):
        rc = self.lib.moihgp_smooth_stream(self.h, 0 if Ty.dtype == torch.float64 else 1, C.c_void_p(Ty.data_ptr()), Ty.shape[1], Ty.stride(0),
                                           C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(ys.data_ptr()), ys.stride(0),
                                           C.c_void_p(status.data_ptr()), _stream_ptr())
        if rc:
            raise RuntimeError(f"moihgp_smooth_stream of the other library returned {rc}")

    def close(self):
        self.lib.moihgp_del(self.h)


def fracs_of(K):
    return [j / (K + 1) for j in range(1, K + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--path", type=int, default=-1, help='options "interp_path" and "smoother_path": -1 automatic, 0 scan kernels, 1 serial fp64')
    ap.add_argument("--other-lib", default=None, help="another build of libmoihgp.so whose smooth call is timed in the same alternation")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")
    bank.set_option("smoother_path", a.path)
    bank.set_option("interp_path", a.path)
    other = OtherSmoother(a.other_lib, 0.1, prm, "Matern52ss") if a.other_lib else None
    flush = torch.empty(2 << 28, dtype=torch.float32, device="cuda")
    for dt in (torch.float32, torch.float64):
        name = str(dt).split(".")[-1]
        Ty = torch.randn((a.L, a.T), dtype=dt, device="cuda")
        ys, ysm = torch.empty_like(Ty), torch.empty_like(Ty)
        x = torch.zeros((a.L, bank.d), dtype=dt, device="cuda")
        status = torch.empty((a.L,), dtype=torch.int32, device="cuda")
        out = torch.empty((3, a.L, Ty.stride(0)), dtype=dt, device="cuda")[:, :, :a.T]
        calls = {"smooth": lambda: bank.smooth(Ty, x=x, ysmooth=ys)}
        if other:
            calls["smooth (other)"] = lambda: other.smooth(Ty, x, ys, status)
        for K in (1, 3):
            calls[f"interpolate K={K}"] = lambda K=K: bank.interpolate(Ty, fracs_of(K), x=x, out=out[:K], ysmooth=ysm)
            calls[f"slope all K={K}"] = lambda K=K: bank.slope(Ty, fracs_of(K), "all", x=x, out=out[:K], ysmooth=ysm)
        calls["slope past K=1"] = lambda: bank.slope(Ty, fracs_of(1), "past", x=x, out=out[:1], ysmooth=ysm)
        for f in calls.values():       # warm up every call (tables, code objects)
            f()
        torch.cuda.synchronize()
        for cold in (False, True):
            ts = {k: [] for k in calls}
            for _ in range(a.iters):
                for k, f in calls.items():
                    x.zero_()
                    if cold:
                        flush.fill_(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3)
            base = float(np.median(ts["smooth (other)" if other else "smooth"]))
            for k in calls:
                t = np.array(ts[k])
                med, q1, q3 = float(np.median(t)), float(np.percentile(t, 25)), float(np.percentile(t, 75))
                print(f"{k} {name} L={a.L} T={a.T} {'cold' if cold else 'resident'}: {med:.1f} us (quartiles {q1:.1f} .. {q3:.1f}, range "
                      f"{t.min():.1f} .. {t.max():.1f}, n={len(t)}) = {med / base:.2f} {'other ' if other else ''}smooth calls", flush=True)
    if other:
        other.close()


if __name__ == "__main__":
    main()
