"""Timing of multi-horizon forecasts (moihgp_forecast_stream) at C3's shape: 4096 latents x 10^4 ticks, Matern-5/2.

Plain run: one line per (dtype, K, cache state) with the event-timed duration of a whole forecast call (tables kernel + sweep + the small serial /
status kernel), its algorithmic traffic (1 + K) L T sizeof(scalar) and the share of the 8 TB/s HBM peak that is.  "cold" evicts the caches
between calls by writing a 2 GB buffer; "resident" repeats the call on the same buffers.

--alternate: after a warm-up, `--iters` rounds of [smooth, forecast K=1, forecast K=many, scores K=1, scores K=many] per dtype (`--many` 4 or 8),
for a run under `rocprofv3 --kernel-trace --output-format csv`: the parent's smooth_fwd_kernel, the forecast sweep and the scoring sweep
(moihgp_forecast_scores) are then timed in the same job, interleaved.
--summarize FILE: per-kernel median / min / max of such a kernel trace, the K = 1 sweep against smooth_fwd_kernel, the K = many call against
that many times it, and the scoring sweeps against the forecast sweeps of the same K."""
import argparse
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12


def summarize(path, many=4):
    rows = list(csv.DictReader(open(path)))
    dur = {}
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        m = re.match(r"(?:moihgp::\(anonymous namespace\)::)?(\w+)<([^>]*)>", name)
        key = f"{m.group(1)}<{m.group(2)}>" if m else name.split("(")[0]
        if not re.search(r"smooth_fwd|smooth_bwd|smooth_serial|forecast_", key):
            continue
        dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    stat = {}
    for k in sorted(dur):
        v = np.array(dur[k][len(dur[k]) // 5:])           # the first fifth of each kernel's dispatches is warm-up
        stat[k] = (float(np.median(v)), float(v.min()), float(v.max()), len(v))
        print(f"{k:60s} n={len(v):3d}  median {stat[k][0]:8.1f} us  min {stat[k][1]:8.1f}  max {stat[k][2]:8.1f}")
    for tv in ("float", "double"):
        fwd = next((stat[k] for k in stat if k.startswith(f"smooth_fwd_kernel<{tv}, 3")), None)
        k1 = next((stat[k] for k in stat if k.startswith(f"forecast_sweep_kernel<{tv}, {tv}, 3, 1")), None)
        k4 = next((stat[k] for k in stat if k.startswith(f"forecast_sweep_kernel<{tv}, {tv}, 3, 2")), None)
        if not (fwd and k1):
            continue
        spread = max(fwd[2] - fwd[0], fwd[0] - fwd[1]) / fwd[0]
        print(f"{tv}: smooth_fwd median {fwd[0]:.1f} us (spread +-{100 * spread:.1f} %); forecast sweep K=1 median {k1[0]:.1f} us = "
              f"{k1[0] / fwd[0]:.2f} x  -> {'ok' if k1[0] <= fwd[0] * (1 + spread) else 'SLOWER than smooth_fwd by more than its spread'}")
        if k4:
            small = sum(stat[k][0] for k in stat if k.startswith("forecast_tables_kernel<3") or k.startswith(f"forecast_serial_kernel<{tv}, 3"))
            print(f"{tv}: forecast K={many} sweep median {k4[0]:.1f} us + tables and status kernels {small:.1f} us = {k4[0] + small:.1f} us vs {many} x "
                  f"smooth_fwd {many * fwd[0]:.1f} us -> {'ok' if k4[0] + small < many * fwd[0] else 'NOT under that many sweeps'}")
        # the scoring sweeps (forecast_score_kernel<Tv, Ta, D, KG, NG, STAGED>; K = 1 is KG = NG = 1) against the forecast sweep of the same K, with
        # that kernel's own range as the margin
        sc = {k: stat[k] for k in stat if k.startswith(f"forecast_score_kernel<{tv}, {tv}, 3, ")}
        one = [k for k in sc if re.match(rf"forecast_score_kernel<{tv}, {tv}, 3, 1, 1\b", k)]
        for K, fc, keys in ((1, k1, one), (many, k4, [k for k in sc if k not in one])):
            if not (fc and keys):
                continue
            s = sc[keys[0]]
            margin = max(fc[2] - fc[0], fc[0] - fc[1])
            print(f"{tv}: scores K={K} sweep median {s[0]:.1f} us (min {s[1]:.1f}, max {s[2]:.1f}) vs forecast K={K} sweep {fc[0]:.1f} us "
                  f"(min {fc[1]:.1f}, max {fc[2]:.1f}) = {s[0] / fc[0]:.2f} x  -> {'ok' if s[0] <= fc[0] + margin else 'SLOWER than the forecast sweep by more than its range'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gains", default="kalman", choices=["kalman", "handle"])
    ap.add_argument("--path", type=int, default=-1, help='option "forecast_path": -1 automatic, 0 scan kernel, 1 serial fp64')
    ap.add_argument("--alternate", action="store_true", help="rounds of [smooth, forecast K=1, forecast K=many, scores K=1, scores K=many] for a kernel-trace run")
    ap.add_argument("--many", type=int, default=4, choices=[4, 8], help="the larger K of --alternate and --summarize")
    ap.add_argument("--summarize", metavar="FILE", help="kernel-trace csv of an --alternate run")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.many)
    import torch
    from multioutputihgp_amd.streams import LatentBank
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    prm = np.column_stack([rng.uniform(0.5, 2, a.L), rng.uniform(0.5, 2, a.L), rng.uniform(0.02, 0.3, a.L)])
    bank = LatentBank(0.1, prm, kernel="Matern52ss")
    bank.set_option("forecast_path", a.path)
    horizons = {1: [1], 4: [1, 10, 100, 1000], 8: [1, 2, 5, 10, 20, 50, 100, 1000]}
    flush = None if a.alternate else torch.empty(2 << 28, dtype=torch.float32, device="cuda")
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        Ty = torch.randn((a.L, a.T), dtype=dt, device="cuda")
        x = torch.zeros((a.L, bank.d), dtype=dt, device="cuda")
        out = torch.empty((8, a.L, a.T), dtype=dt, device="cuda")
        ys = torch.empty_like(Ty)
        _, _, status = bank.forecast(Ty, horizons[4], x=x, out=out[:4], gains=a.gains)
        torch.cuda.synchronize()
        print(f"status != 0: {int((status != 0).sum())} latents")
        if a.alternate:
            for _ in range(a.iters + a.iters // 4 + 1):
                bank.smooth(Ty, x=x, ysmooth=ys)
                bank.forecast(Ty, horizons[1], x=x, out=out[:1], gains=a.gains)
                bank.forecast(Ty, horizons[a.many], x=x, out=out[:a.many], gains=a.gains)
                bank.forecast_scores(Ty, horizons[1], x=x, gains=a.gains)
                bank.forecast_scores(Ty, horizons[a.many], x=x, gains=a.gains)
                torch.cuda.synchronize()
            continue
        for K in (1, 4, 8):
            mb = (1 + K) * a.L * a.T * es
            for cold in (False, True):
                ts = []
                for _ in range(a.iters + 3):
                    if cold:
                        flush.fill_(1.0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    bank.forecast(Ty, horizons[K], x=x, out=out[:K], gains=a.gains)
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                t = float(np.median(ts[3:])) * 1e3
                print(f"forecast {str(dt).split('.')[-1]} K={K} L={a.L} T={a.T} {a.gains} {'cold' if cold else 'resident'}: {t:.1f} us "
                      f"(min {min(ts[3:]) * 1e3:.1f}, max {max(ts[3:]) * 1e3:.1f}; traffic {mb / 1e6:.0f} MB -> {mb / (t * 1e-6) / 1e12:.2f} TB/s, "
                      f"{100 * mb / (t * 1e-6) / HBM_PEAK:.0f} % of peak)", flush=True)


if __name__ == "__main__":
    main()
