"""Timing of seeded forecast paths (moihgp_forecast_paths) at 4096 latents, Matern-5/2: one line per (dtype, S, n) with the event-timed duration of
a whole call (one kernel; the smoother's tables are built by the warm-up call) and, beside it, the time of a device `copy_` of a tensor of the
planes' size in the same process -- the store-side ceiling: the kernel reads next to nothing and writes S x L x n scalars -- and their ratio."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 1024), (8, 1024), (64, 256), (64, 1024)]      # (S, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    from multioutputihgp_amd.streams import LatentBank
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")

    def timed(f):
        ts = []
        for _ in range(a.iters + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts[3:])), min(ts[3:]), max(ts[3:])

    for dt in (torch.float32, torch.float64):
        x = 0.3 * torch.randn((a.L, bank.d), dtype=dt, device="cuda")
        _, _, status = bank.forecast_paths(x, 8, 1, seed=1)
        torch.cuda.synchronize()
        print(f"status != 0: {int((status != 0).sum())} latents")
        for S, n in SHAPES:
            out = torch.empty((S, a.L, n), dtype=dt, device="cuda")
            src = torch.randn((S, a.L, n), dtype=dt, device="cuda")
            dst = torch.empty_like(src)
            t = timed(lambda: bank.forecast_paths(x, n, S, seed=1, out=out, want_states=False))
            c = timed(lambda: dst.copy_(src))
            gb = out.numel() * out.element_size() / 1e9
            print(f"paths {str(dt).split('.')[-1]} S={S} n={n} L={a.L} ({gb:.3f} GB): {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}) = "
                  f"{gb / t[0] * 1e3:.2f} TB/s written; copy_ of the same size {c[0]:.1f} us (min {c[1]:.1f}, max {c[2]:.1f}); ratio {t[0] / c[0]:.2f}",
                  flush=True)
            del out, src, dst


if __name__ == "__main__":
    main()
