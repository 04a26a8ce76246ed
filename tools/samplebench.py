"""Timing of seeded posterior sampling (moihgp_sample_stream) at C3's shape: 4096 latents x 10^4 ticks, Matern-5/2.

Plain run: one line per (dtype, S) with the event-timed duration of a whole sample call (the smoother's three kernels, the sweep and the small
serial / status kernel; the tables are built by the warm-up call), and what is left per sample after the time of a smooth on the same buffers.

--alternate: after a warm-up, `--iters` rounds of [smooth, sample S=1, sample S=8] per dtype, for a run under
`rocprofv3 --kernel-trace --output-format csv`: the parent's smooth_bwd_kernel and the sample sweep are then timed in the same job, interleaved.
--summarize FILE: per-kernel median / min / max of such a kernel trace, and the sweep's time per sample at S = 8 against smooth_bwd_kernel (within
that kernel's own spread)."""
import argparse
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarize(path):
    """The S = 1 and S = 8 launches of sample_sweep_kernel have the same grid (L x one group of eight), so each sweep dispatch takes its S from the
    sample_serial_kernel dispatch that follows it on the stream, whose grid is ceil(L S / 64) workgroups."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    gcol = "Grid_Size_X" if rows and "Grid_Size_X" in rows[0] else "Grid_Size"
    recs = []
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        m = re.match(r"(?:moihgp::\(anonymous namespace\)::)?(\w+)<([^>]*)>", name)
        key = f"{m.group(1)}<{m.group(2)}>" if m else name.split("(")[0]
        if re.search(r"smooth_fwd|smooth_bwd|smooth_serial|sample_|sampler_", key):
            recs.append((key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r[gcol])))
    grids = sorted({g for k, _, g in recs if k.startswith("sample_serial_kernel")})
    if len(grids) != 2:
        sys.exit(f"summarize: expected sample_serial_kernel dispatches of two grid sizes (S = 1 and S = 8), found {grids}")
    label = {grids[0]: "S=1", grids[1]: "S=8"}
    dur = {}
    for i, (key, us, g) in enumerate(recs):
        if key.startswith("sample_sweep_kernel") or key.startswith("sample_serial_kernel"):
            tv = key.split("<")[1].split(",")[0]
            nxt = next((gg for kk, _, gg in recs[i:] if kk.startswith(f"sample_serial_kernel<{tv},")), None)
            if nxt is None:
                sys.exit(f"summarize: no sample_serial_kernel dispatch follows dispatch {i} ({key})")
            key += " " + label[nxt]
        dur.setdefault(key, []).append(us)
    stat = {}
    for k in sorted(dur):
        v = np.array(dur[k][len(dur[k]) // 5:])           # the first fifth of each kernel's dispatches is warm-up
        stat[k] = (float(np.median(v)), float(v.min()), float(v.max()), len(v))
        print(f"{k:72s} n={len(v):3d}  median {stat[k][0]:8.1f} us  min {stat[k][1]:8.1f}  max {stat[k][2]:8.1f}")
    for tv in ("float", "double"):
        bwd = next((stat[k] for k in stat if k.startswith(f"smooth_bwd_kernel<{tv}, 3")), None)
        s1 = next((stat[k] for k in stat if k.startswith(f"sample_sweep_kernel<{tv}, 3") and k.endswith("S=1")), None)
        s8 = next((stat[k] for k in stat if k.startswith(f"sample_sweep_kernel<{tv}, 3") and k.endswith("S=8")), None)
        if not (bwd and s1 and s8):
            sys.exit(f"summarize: {tv}: smooth_bwd_kernel, sample_sweep_kernel S=1 and S=8 are not all in the trace")
        spread = max(bwd[2] - bwd[0], bwd[0] - bwd[1]) / bwd[0]
        print(f"{tv}: smooth_bwd median {bwd[0]:.1f} us (spread +-{100 * spread:.1f} %); sample sweep S=1 median {s1[0]:.1f} us; S=8 median "
              f"{s8[0]:.1f} us = {s8[0] / 8:.1f} us per sample = {s8[0] / 8 / bwd[0]:.2f} x smooth_bwd -> "
              f"{'ok' if s8[0] / 8 <= bwd[0] * (1 + spread) else 'SLOWER than smooth_bwd by more than its spread'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--path", type=int, default=-1, help='option "sample_path": -1 automatic, 0 scan kernel, 1 serial fp64')
    ap.add_argument("--alternate", action="store_true", help="rounds of [smooth, sample S=1, sample S=8] for a kernel-trace run")
    ap.add_argument("--summarize", metavar="FILE", help="kernel-trace csv of an --alternate run")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch
    from multioutputihgp_amd.streams import LatentBank
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")
    bank.set_option("sample_path", a.path)
    for dt in (torch.float32, torch.float64):
        Ty = torch.randn((a.L, a.T), dtype=dt, device="cuda")
        x = torch.zeros((a.L, bank.d), dtype=dt, device="cuda")
        out = torch.empty((8, a.L, a.T), dtype=dt, device="cuda")
        ys = torch.empty_like(Ty)
        _, _, _, status = bank.sample(Ty, 8, seed=1, x=x, out=out, ysmooth=ys)
        torch.cuda.synchronize()
        print(f"status != 0: {int((status != 0).sum())} latents")
        if a.alternate:
            for _ in range(a.iters + a.iters // 4 + 1):
                bank.smooth(Ty, x=x, ysmooth=ys)
                bank.sample(Ty, 1, seed=1, x=x, out=out[:1], ysmooth=ys)
                bank.sample(Ty, 8, seed=1, x=x, out=out, ysmooth=ys)
                torch.cuda.synchronize()
            continue

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
        sm = timed(lambda: bank.smooth(Ty, x=x, ysmooth=ys))
        print(f"smooth {str(dt).split('.')[-1]} L={a.L} T={a.T}: {sm[0]:.1f} us (min {sm[1]:.1f}, max {sm[2]:.1f})", flush=True)
        for S in (1, 8):
            t = timed(lambda: bank.sample(Ty, S, seed=1, x=x, out=out[:S], ysmooth=ys))
            print(f"sample {str(dt).split('.')[-1]} S={S} L={a.L} T={a.T}: {t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f}); beyond the smooth "
                  f"{(t[0] - sm[0]) / S:.1f} us per sample", flush=True)


if __name__ == "__main__":
    main()
