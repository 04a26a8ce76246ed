"""Timing of the off-grid smoother (moihgp_interp_stream) at C3's shape: 4096 latents x 10^4 ticks, Matern-5/2, against a whole smooth call.

Prints one line per (dtype, cache state, call) with the median, the quartiles and the extremes of the event-timed duration of whole calls: one
smooth (the yardstick: forward + backward + the small status kernel), and interpolate calls with K offsets (tables + forward + backward sweep + the
small status kernel).  The calls of one line-up alternate, so that drift of the machine hits them alike.  Two traffic figures per line: the nominal
(3 + 3 K) planes of the stream (read y, write ysmooth, K planes written, and per plane one more pass each way between the two sweeps), and the
(5 + 3 K) planes the two sweeps move as they are built (forward: read y, write p and K planes; backward: read y and p, write ysmooth, read and write
K planes); a smooth is 5 planes by either count.  "cold" evicts the caches between calls by writing a 2 GB buffer; "resident" repeats the call on
the same buffers.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split (interp_tables_kernel, interp_fwd_kernel,
interp_bwd_kernel)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multioutputihgp_amd.streams import LatentBank  # noqa: E402


def fracs_of(K):
    """K offsets j / (K + 1): the planes of a (K + 1)-fold upsampling."""
    return [j / (K + 1) for j in range(1, K + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 3, 7], choices=range(1, 9))
    ap.add_argument("--path", type=int, default=-1, help='options "interp_path" and "smoother_path": -1 automatic, 0 scan kernels, 1 serial fp64')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")
    bank.set_option("smoother_path", a.path)
    bank.set_option("interp_path", a.path)
    flush = torch.empty(2 << 28, dtype=torch.float32, device="cuda")
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        name = str(dt).split(".")[-1]
        Ty = torch.randn((a.L, a.T), dtype=dt, device="cuda")
        ys = torch.empty_like(Ty)
        x = torch.zeros((a.L, bank.d), dtype=dt, device="cuda")
        calls = {"smooth": (5, 5, lambda: bank.smooth(Ty, x=x, ysmooth=ys))}
        ysm = torch.empty_like(Ty)
        out = torch.empty((max(a.K), a.L, Ty.stride(0)), dtype=dt, device="cuda")[:, :, :a.T]
        for K in a.K:
            calls[f"interpolate K={K}"] = (3 + 3 * K, 5 + 3 * K, lambda K=K: bank.interpolate(Ty, fracs_of(K), x=x, out=out[:K], ysmooth=ysm))
        for f in calls.values():       # warm up every call (tables, code objects)
            f[2]()
        torch.cuda.synchronize()
        mb = a.L * a.T * es / 1e6
        for cold in (False, True):
            ts = {k: [] for k in calls}
            for _ in range(a.iters):
                for k, (_, _, f) in calls.items():
                    if cold:
                        flush.fill_(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3)
            base = float(np.median(ts["smooth"]))
            for k, (nominal, moved, _) in calls.items():
                t = np.array(ts[k])
                med, q1, q3 = float(np.median(t)), float(np.percentile(t, 25)), float(np.percentile(t, 75))
                print(f"{k} {name} L={a.L} T={a.T} {'cold' if cold else 'resident'}: {med:.1f} us (quartiles {q1:.1f} .. {q3:.1f}, range "
                      f"{t.min():.1f} .. {t.max():.1f}, n={len(t)}) = {med / base:.2f} smooth calls; nominal {nominal} planes = {nominal * mb:.0f} MB -> "
                      f"{nominal * mb * 1e6 / (med * 1e-6) / 1e12:.2f} TB/s, moved {moved} planes -> {moved * mb * 1e6 / (med * 1e-6) / 1e12:.2f} TB/s",
                      flush=True)


if __name__ == "__main__":
    main()
