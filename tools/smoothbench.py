"""Timing of the steady-state RTS smoother (moihgp_smooth_stream) at C3's shape: 4096 latents x 10^4 ticks, Matern-5/2.

Prints one line per (dtype, cache state) with the event-timed duration of a whole smooth call (forward + backward + the small status kernel)
and the algorithmic traffic of its stream passes (forward: read y, write p; backward: read y, read p, write ys).  "cold" evicts the caches
between calls by writing a 2 GB buffer; "resident" repeats the call on the same buffers.  Run under `rocprofv3 --kernel-trace --stats` for the
per-kernel split (smooth_fwd_kernel, smooth_bwd_kernel, smoother_tables_kernel: --rebuild forces one table build per call).
--exact adds two legs per (dtype, cache state): exact-edge smoothing (moihgp_smooth_stream_exact) without and with the variance rows, beside the
smooth call they extend, and the time of one stream-sized plane write (a fill) to hold the extra against.
--posterior adds two legs: the exact posterior across missing ticks (moihgp_posterior_stream) with its variance rows and nll, on the gap-free
stream and on a copy with 1 % of the ticks missing (posterior_fwd_kernel, posterior_bwd_kernel in a kernel trace)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multioutputihgp_amd.streams import LatentBank  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--path", type=int, default=-1, help='option "smoother_path": -1 automatic, 0 scan kernels, 1 serial fp64')
    ap.add_argument("--exact", action="store_true", help="also time smooth_exact without and with var, and one plane write")
    ap.add_argument("--posterior", action="store_true", help="also time posterior() with var and nll, gap-free and with 1 %% of the ticks missing")
    ap.add_argument("--rebuild", action="store_true", help="rewrite the tables before every call (times the tables kernel too)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")
    bank.set_option("smoother_path", a.path)
    flush = torch.empty(2 << 28, dtype=torch.float32, device="cuda")
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        Ty = torch.randn((a.L, a.T), dtype=dt, device="cuda")
        ys = torch.empty_like(Ty)
        x = torch.zeros((a.L, bank.d), dtype=dt, device="cuda")
        _, _, status = bank.smooth(Ty, x=x, ysmooth=ys)
        torch.cuda.synchronize()
        vf, vs = bank.latent_variances()
        var = torch.empty_like(Ty)
        legs = [("smooth", lambda: bank.smooth(Ty, x=x, ysmooth=ys))]
        if a.exact:
            head, tail = bank.edge_lengths()
            print(f"edge lengths: head {head.min()} .. {head.max()}, tail {tail.min()} .. {tail.max()}")
            legs += [("smooth_exact, no var", lambda: bank.smooth_exact(Ty, x=x, ysmooth=ys, want_var=False)),
                     ("smooth_exact, var", lambda: bank.smooth_exact(Ty, x=x, ysmooth=ys, var=var)),
                     ("one plane write", lambda: var.fill_(1.0))]
        if a.posterior:
            Tyg = Ty.clone()
            Tyg[torch.rand((a.L, a.T), device="cuda") < 0.01] = float("nan")
            legs += [("posterior, gap-free", lambda: bank.posterior(Ty, x=x, mean=ys, var=var)),
                     ("posterior, 1 % missing", lambda: bank.posterior(Tyg, x=x, mean=ys, var=var))]
        print(f"status != 0: {int((status != 0).sum())} latents; var_smoothed / var_filtered in [{np.min(vs / vf):.3f}, {np.max(vs / vf):.3f}]")
        mb = a.L * a.T * es / 1e6
        for cold, (name, call) in [(c, leg) for c in (False, True) for leg in legs]:
            ts = []
            for _ in range(a.iters):
                if a.rebuild:
                    bank.update(prm)
                if cold:
                    flush.fill_(1.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            t = float(np.median(ts)) * 1e3
            traffic = f"  (traffic {2 * mb:.0f} MB + {3 * mb:.0f} MB -> {5 * mb * 1e6 / (t * 1e-6) / 1e12:.2f} TB/s)" if name == "smooth" else ""
            print(f"{name} {str(dt).split('.')[-1]} L={a.L} T={a.T} {'cold' if cold else 'resident'}: {t:.1f} us{traffic}", flush=True)


if __name__ == "__main__":
    main()
