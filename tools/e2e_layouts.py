"""End-to-end timing of the three routes from observations to filtered outputs at the c3e2e shape of bench.py: Y [T = 10^4][M = 4096],
M = L = 4096, Matern-5/2, fp32 and fp64.

    (a) series-major throughout:        project_stream -> LatentBank.filter -> unproject_stream
    (b) the tiled sweep by retiling:    project_stream -> tile_stream -> LatentBank.filter_tiled -> untile_stream -> unproject_stream
    (c) segment-major throughout:       project_stream_tiled -> LatentBank.filter_tiled -> unproject_stream_tiled

Plain run: `--iters` rounds of [a, b, c] (`--routes`) interleaved in one process after a warm-up; per route the event-timed duration of the
whole pipeline and of its stages (median, min, max), one JSON line per (dtype, route).  The three routes' outputs are compared first: (b) and
(c) must equal each other bit for bit, and (a) as well at this many latents.

Kernel times come from a run of its own under the profiler, without counters:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/e2e_layouts.py --routes ac
    python tools/e2e_layouts.py --summarize DIR/.../*_kernel_trace.csv
--summarize prints per-kernel median / min / max, says whether the trace holds a retile_kernel, and compares the segment-major projection and
un-projection GEMMs of (c) with the series-major ones of (a) against the min-max spread of (a)'s kernel in that job.  (The series-major
projection and un-projection are the same instantiation of gemm_mfma_kernel; they alternate in the trace, projection first.)"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 1234


def _stats(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(v.min()), float(v.max())


def summarize(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        name = re.sub(r"^void ", "", r["Kernel_Name"])
        m = re.match(r"(?:moihgp::)?(?:\(anonymous namespace\)::)?(\w+)<(.*?)>\(", name)
        key = f"{m.group(1)}<{m.group(2)}>" if m else name.split("(")[0]
        if not re.search(r"gemm_mfma_kernel|retile_kernel|filter_|ls_project|nll_total", key):
            continue
        dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"retile_kernel dispatches in this trace: {sum(len(v) for k, v in dur.items() if k.startswith('retile_kernel'))}")
    for k in sorted(dur):
        med, lo, hi = _stats(dur[k][len(dur[k]) // 5:])          # the first fifth of each kernel's dispatches is warm-up
        print(f"{k:75s} n={len(dur[k]) - len(dur[k]) // 5:3d}  median {med:9.1f} us  min {lo:9.1f}  max {hi:9.1f}")
    for tv in ("float", "double"):
        ser = next((dur[k] for k in dur if k == f"gemm_mfma_kernel<{tv}, {tv}, {tv}, true, true, false, 0>"), None)
        seg = {m: next((dur[k] for k in dur if k == f"gemm_mfma_kernel<{tv}, {tv}, {tv}, true, true, false, {m}>"), None) for m in (1, 2)}
        if not ser or not seg[1] or not seg[2] or len(ser) % 2:
            continue
        for what, a, c in (("projection", ser[0::2], seg[1]), ("un-projection", ser[1::2], seg[2])):
            a, c = a[len(a) // 5:], c[len(c) // 5:]
            am, alo, ahi = _stats(a)
            cm, clo, chi = _stats(c)
            verdict = "ok" if cm <= am + (ahi - alo) else "SLOWER than the series-major kernel by more than its min-max spread"
            print(f"{tv} {what}: series-major (a) median {am:.1f} us (min {alo:.1f}, max {ahi:.1f}, spread {ahi - alo:.1f}); segment-major (c) median "
                  f"{cm:.1f} us (min {clo:.1f}, max {chi:.1f}) = {cm / am:.4f} x -> {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--routes", default="abc", help="which of the routes a, b, c to run (a kernel-trace run of 'ac' shows that (c) launches no retile_kernel)")
    ap.add_argument("--dtypes", default="fp32,fp64")
    ap.add_argument("--summarize", metavar="FILE", help="kernel-trace csv of a run under rocprofv3 --kernel-trace")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    if not a.routes or set(a.routes) - set("abc"):
        ap.error("--routes takes letters out of a, b, c")
    import torch
    from multioutputihgp_amd import MOIHGP
    from multioutputihgp_amd import streams as S
    if not torch.cuda.is_available():
        raise SystemExit("e2e_layouts: no GPU (timings are taken on the device or not at all)")
    torch.cuda.set_device(0)
    M, L, T = a.M, a.L, a.T
    rng = np.random.default_rng(SEED)
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    p = gp.params.copy()
    p[M * L:M * L + L] = rng.uniform(0.5, 2.0, L)
    p[M * L + L] = 0.04
    p[M * L + L + 1:] = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.02, 0.3, L)]).ravel()
    gp.update(p)
    bank = S.LatentBank.from_handle(gp)

    def route_a(Y, ev):
        ev[0].record(); Ty = S.project_stream(gp, Y)
        ev[1].record(); yl, x, nll = bank.filter(Ty, T=T)
        ev[2].record(); Yhat = S.unproject_stream(gp, yl, T)
        ev[3].record()
        return Yhat, x, nll

    def route_b(Y, ev):
        ev[0].record(); Tt = S.tile_stream(S.project_stream(gp, Y), T)
        ev[1].record(); yt, x, nll = bank.filter_tiled(Tt, T)
        ev[2].record(); Yhat = S.unproject_stream(gp, S.untile_stream(yt, T), T)
        ev[3].record()
        return Yhat, x, nll

    def route_c(Y, ev):
        ev[0].record(); Tt = S.project_stream_tiled(gp, Y)
        ev[1].record(); yt, x, nll = bank.filter_tiled(Tt, T)
        ev[2].record(); Yhat = S.unproject_stream_tiled(gp, yt, T)
        ev[3].record()
        return Yhat, x, nll

    routes = {"a": route_a, "b": route_b, "c": route_c}
    names = {"a": "series-major throughout", "b": "project -> tile -> filter_tiled -> untile -> unproject", "c": "segment-major throughout"}
    for dn in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "fp64": torch.float64}[dn]
        g = torch.Generator(device="cuda"); g.manual_seed(SEED + 1)
        Y = torch.randn((T, M), generator=g, device="cuda", dtype=dtype)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        res = {r: routes[r](Y, ev) for r in a.routes}
        torch.cuda.synchronize()
        first = a.routes[0]
        for r in a.routes[1:]:
            same = all(torch.equal(u, v) for u, v in zip(res[r], res[first]))
            print(f"{dn}: outputs of route ({r}) {'equal' if same else 'DIFFER from'} those of route ({first}) bit for bit"
                  + ("" if same else f" (max |dYhat| {float((res[r][0] - res[first][0]).abs().max()):.3e})"), flush=True)
        del res
        times = {r: [] for r in a.routes}
        for it in range(a.warm + a.iters):
            for r in a.routes:
                torch.cuda.synchronize()
                routes[r](Y, ev)
                torch.cuda.synchronize()
                if it >= a.warm:
                    times[r].append([ev[0].elapsed_time(ev[3]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])])
        for r in a.routes:
            t = np.array(times[r])
            tot, pr, fl, un = (_stats(t[:, i]) for i in range(4))
            print(json.dumps({"route": r, "what": names[r], "dtype": dn, "M": M, "L": L, "T": T, "iters": a.iters,
                              "total_ms": {"median": tot[0], "min": tot[1], "max": tot[2]},
                              "project_ms": {"median": pr[0], "min": pr[1], "max": pr[2]},
                              "filter_ms": {"median": fl[0], "min": fl[1], "max": fl[2]},
                              "unproject_ms": {"median": un[0], "min": un[1], "max": un[2]},
                              "timed_by": "torch events on the launch stream; project_ms of (b) includes tile_stream, unproject_ms of (b) untile_stream"}),
                  flush=True)
        del Y


if __name__ == "__main__":
    main()
