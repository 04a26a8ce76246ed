"""The gradient sweeps (csrc/grad.hip, grad_gen.hip, grad_x.hip, grad_scan_x.hip through LatentBank.grad) entry by entry, each entry of `grad`,
`dx`, `x`, `nll` against a conditioning scale of its own and `yhat` per row, instead of max |a - b| over max |b| of the whole array.

The reference is grad_np: the loop of oracle/moihgp_numpy.py::filter_stream(want_grad=True) (ihgp.h:37-57, :204-222) on the C oracle's matrices
(cref.ihgp_array(...)[l].mat(name), the wide build for stacked kernels), vectorised over latents, for any d and P, all arithmetic in one dtype.
Along its float64 trajectory it accumulates what every entry is held against:
    grad[l, p]   G = sum over observed ticks of (|v dv_p| + 1/2 |v^2 / S - 1| |dS_p|) / S: the magnitudes of what is added, cancelling or not
    nll[l]       N = sum over observed ticks of 1/2 (v^2 / S + |log S|)
    x[l, i], dx[l, p, i]   the largest magnitude the entry took at any tick, start state included
    yhat[l, :]   the row maximum (conftest.rel_err_rows)
Where a scale is exactly zero (nll and grad of a row with nothing observed) the device value must be exactly zero.  Stream and start states of
every case are float32 numbers (rounded before the reference runs), so one cached reference serves both precisions and both output modes and
input rounding is no error.  Only calm latents are compared: max |yhat| < CALM = 1e3 under the C oracle (tests/test_parameter_box.py).

Cases (CASES: 43 on the reference's own models, 78 stacked; shapes and seeds of the existing tests wherever one reaches the route, so that a failure
here can be put next to a pass there; every case in fp64 and fp32, with and without the stream of means):
    vs      test_gradstream_vs_oracle's draw (seed L * 31 + T).  L = 3, T = 1, 3, 127, 129, 255, 256, 257, 511, 512, 513: the short-window
            instantiations (fp64 T <= 256, 2-tick chunks, segments of 128; fp32 T <= 512, 4-tick chunks, segments of 256), less than one chunk,
            one tick either side of a segment and of the switch to the long-stream ones (8- / 16-tick chunks, segments of 512 / 1024); and that
            test's own (Matern32, 9, 128), (Matern52, 70, 1030: 18 workgroups, the last half full), (Matern32, 4, 2600) and (Matern52, 6, 1500)
            (ragged ends inside a chunk), (Matern52, 8, 700, 1 % gaps in half of the rows)
    seg     test_gradstream_segment_boundaries_of_the_long_stream_kernels' draw (seed T * 7 + k): T = 1023 .. 1025, 2047 .. 2049
    gaps    L = 8, T = 2600 and 300 (seed [T, k, 20261020]): rows 0 .. 3 clean, row 4 never observed, rows 5 .. 7 missing tick 0, T - 1, both sides
            of the segment edges, a run of 20: the second pass (grad_gen.hip) beside the first in one launch
    unstable  the sequential third pass (grad_seq_kernel) beside the others in one launch: rows 0, 1 clean (first pass), rows 3, 4 with 2 % gaps
            (second), row 2 left to the third.  What sends a latent there is grad_scan_kernel's own test and nothing else: an entry of AKHA^(16 CK)
            not below 1e18 (fp32) or 1e150 (fp64), CK the chunk length of the instantiation picked for T (fp64 2 / 8, fp32 4 / 16).  rho(AKHA) > 1
            alone does not do it: the rho = 1.17 row of test_gpu_parity.py at T = 120 has max |AKHA^32| = 5e2 and |AKHA^64| = 8e4 and stays in the
            scan in both precisions.
            (Matern32, 5, 600), row 2 = (99.2, 4.07, 2.6e-3), rho = 1.47: max |AKHA^256| = 4.6e43, so fp32 takes the third pass; in fp64
            max |AKHA^128| = 1.3e22 and the row stays in the scan (fp64 needs rho^128 > 1e150, rho > 14.8, which no Matern32 row of a log-uniform
            search of 4000 draws reached: 1.53 at most).
            (Matern52, 5, 300), row 2 = (4.59, 16.0, 1.0e-5), rho = 175, from that search, far outside synth_params' box: max |AKHA^128| = 8.5e288
            and |AKHA^64| = 2.5e145, so both precisions take the third pass.
            test_the_unstable_draws_meet_the_kernels_own_criterion asserts all this on the oracle's matrices for every reference-model case (no
            other latent of the list meets the criterion), test_the_third_pass_is_reached_on_the_device_matrices on the device's own.  Row 2 is
            not calm and is not compared.  The seeds ([T, 20261020, k]) are the first k whose other rows have no growing powers (max |AKHA^n| < 1):
            k = 0 for Matern32 had a calm row with max |AKHA^256| = 15 that alone tripled the reference's float32 figures at d = 2, so k = 1
    xvs     test_stacked_gradstream_vs_oracle's draw (seed 9 L + T + J), every kernel of STACKED: (3, 1), (5, 64), (4, 65), (7, 130, 5 % gaps): the
            tick-by-tick kernel (grad_x.hip, T < 512)
    xlong   test_stacked_gradstream_long_streams_vs_oracle's draw (seed 11 L + T + J), every kernel of STACKED: (3, 512), (2, 543), (5, 2048),
            (3, 2081), (2, 4133): whole 32-tick chunks, a T mod 32 tail in the tick-by-tick kernel, exactly one 2048-tick segment, a chunk past it, two
            and a ragged end; (4, 2500, gap at 1700), (3, 1024, gap at 0), (4, 2100, gaps at 0, 31, 32, 2047, 2048, 2099): at most kFewGaps = 3
            gapped chunks per window, cut at them; (3, 1100, every 37th tick missing, row 2 never observed): more, walked whole
LatentBank.grad has no argument that reaches out_mode == 2 of launch_grad_t (the pre-step predicted means of the window objective); that mode
stays with test_window_objective_vs_oracle_loop.

Conditions (test_cases_are_calm_and_hide_entries_from_the_old_bar; a seed that missed them would be changed; none of the existing tests' had to be, and the one new
shape that missed, xlong (3, 2100), where one of Matern32x2's three rows reaches 1.5e18, became (4, 2100)):
    in every case at least three quarters of the latents are calm: all of them in 118 cases, 0.80 in the two `unstable`, 0.75 in xlong Matern32x3 (4, 2100)
    of the compared entries, those below 1e-2 of their case's largest compared entry (which the old fp32 bar of 1e-2 on the global maximum cannot
    see at all): grad 1230 of 2708 (0.45), dx 12820 of 17892 (0.72); (Matern32, 9, 128) alone 0.89 / 0.89, Matern52x4 (3, 2081) 0.74 / 0.89
    every parameter index p of every one of the 8 kernels has such entries, in grad and in dx, in at least one case

Measured (CPU figures from the reference alone, device figures from one run on an MI355X; worst entry over all cases of the family):
    grad_np in float64 against cref.grad_stream: yhat 2.1e-15, x 1.3e-15, dx 8.1e-15, nll 3.2e-16, grad 2.0e-15 (two evaluations of one loop, apart by
    summation order over up to 4133 ticks); NP_AGREES = 1e-13 is the worst with one decade of margin
                              yhat      x         dx        nll       grad
    reference fp32, d = 2     2.79e-06  3.00e-06  2.51e-06  5.26e-06  4.85e-06     grad_np in numpy.float32 against float64 (REF32, rounded up; another numpy's
    reference fp32, d = 3     4.88e-07  5.01e-07  2.92e-06  9.99e-06  7.53e-06     summation order may move these, so the CPU test holds the figure of the day to
    reference fp32, stacked   2.65e-06  1.39e-06  8.45e-06  2.88e-05  3.31e-05     REF32_SLACK = 2 times the record and under the bar; the bars follow the record)
    bar fp32, d = 2           8.9e-06   9.5e-06   8.2e-06   1.7e-05   1.5e-05      FP32_BAR = REF32 * 10^0.5: the half decade that
    bar fp32, d = 3           1.5e-06   1.6e-06   9.5e-06   3.2e-05   2.4e-05      test_reference_sweeps_are_calm_and_fp32_has_room grants an
    bar fp32, stacked         8.5e-06   4.4e-06   2.7e-05   9.2e-05   1.1e-04      evaluation that rounds in another order; capped at today's
    device fp32, d = 2        2.30e-07  2.16e-07  4.13e-07  9.35e-08  3.16e-07     (1e-3 for yhat, x, nll, 1e-2 for dx, grad), which binds nowhere
    device fp32, d = 3        5.88e-07  9.98e-07  1.35e-06  4.84e-08  1.62e-07
    device fp32, stacked      5.67e-08  5.40e-08  1.03e-07  1.38e-10  5.88e-10
    bar fp64 (all families)   1e-09     1e-09     1e-08     1e-09     1e-08        FP64_TIGHT and the bars of test_gradstream_fuzz_vs_oracle
    device fp64, d = 2        1.69e-15  1.70e-15  2.64e-15  3.02e-15  4.36e-15
    device fp64, d = 3        6.81e-16  1.33e-15  4.32e-14  4.78e-15  2.10e-14
    device fp64, stacked      1.25e-14  1.30e-14  1.75e-12  6.29e-15  3.59e-13
The device stays under every bar, so none is widened.  It is well under the reference's own fp32 figures because it keeps the gradient and NLL sums in
fp64 (and the whole stacked sweep), where grad_np in float32 sums in float32; the closest cell is x at d = 3 (T = 3, Matern52: 0.62 of its bar).
What the stacked fp32 bars are worth: grad_x.hip and grad_scan_x.hip do all their arithmetic in fp64 whatever the stream's type, so only what is
stored as fp32 (x, dx, yhat) errs at fp32 size.  The stacked fp32 bars of nll and grad (9.2e-5, 1.1e-4), derived like the others from a float32
loop that resembles nothing on the device, sit five decades above its figures (1.4e-10, 5.9e-10) and bound little: in the stacked fp32 cells only
yhat, x and dx are meaningfully held by the fp32 bar, and the fp64 cases (same kernels, same arithmetic, bars of 1e-9 / 1e-8) carry nll and grad.
The metric test: in (Matern32, 9, 128) grad[6, 0] (value 12.9, G = 13.0, largest entry 1.44e7) moved by 1e-3 G reads 9.1e-10 under the old
expression and 1.0e-3 here; dx[6, 1, 0] (-1.8e-2, scale 5.0e-2, largest 2.7e4) moved alike reads 1.9e-9 and 1.0e-3.

That it bites (two numerically wrong, otherwise identical builds of the library, run once, not part of the tree; the case list of that run had
(Matern32, 5, 120) with the rho = 1.17 row where the two `unstable` draws now stand, hence 84 fp32 reference-model cases and not 86):
    grad_scan_kernel's fp32 replay with the lengthscale's dK_1 y term times 1.001: test_gradstream_vs_oracle passed all 14 cases and
    test_gradstream_fuzz_vs_oracle all 80; test_gradstream_segment_boundaries_of_the_long_stream_kernels failed its 7 Matern52 fp32 cases (dx at
    1.15e-2 against 1e-2) and none of Matern32; here all 84 fp32 cases of test_reference_models_entry_by_entry failed, on dx (8e-4 .. 1.4e-3 against 8.2e-6)
    gp_table_kernel of grad_scan_x.hip with parameter 0's table times 1.001: test_stacked_gradstream_vs_oracle and _long_streams_vs_oracle failed their
    60 fp64 cases of T >= 512 and passed all 120 fp32 ones; here all 108 fp64 and 102 of the 108 fp32 cases of T >= 512 failed, on dx (the six that passed: the
    dense-gap windows of Matern52x2 and Matern52x3, walked whole, and Matern52x4 (2, 543); dx error 8e-7 .. 1.8e-5 under the bar of 2.7e-5)
"""
import functools

import numpy as np
import pytest

from conftest import rel_err, rel_err_rows
from parity_support import FP32_TOL, FP64_TIGHT, KMAP, STACKED, synth, synth_params, synth_params_stacked
from stream_support import round32

CALM = 1e3
HIDDEN = 1e-2                                            # an entry below this share of its case's largest is invisible to the old fp32 bar
DT = 0.1
QUANTITIES = ("yhat", "x", "dx", "nll", "grad")
FAMILIES = ("d2", "d3", "stacked")
# row 2 of the two `unstable` draws and the third word of their seeds (see the docstring): test_gpu_parity's rho(AKHA) = 1.47 under the literal
# DARE, and a Matern52 row with rho = 175 from a search far outside synth_params' box
UNSTABLE = dict(Matern32=((99.2440457, 4.06889466, 2.55306111e-03), 1), Matern52=((4.58613987, 15.9717062, 1.03683147e-05), 0))
UNSTABLE_CASES = (("unstable", "Matern32", 5, 600, None), ("unstable", "Matern52", 5, 300, None))
THIRD_PASS = {(UNSTABLE_CASES[0], "fp32"), (UNSTABLE_CASES[1], "fp32"), (UNSTABLE_CASES[1], "fp64")}      # where row 2 goes to grad_seq_kernel
SEQ_LIMIT = dict(fp64=1e150, fp32=1e18)                  # grad_scan_kernel leaves a latent to grad_seq_kernel when an entry of AKHA^(16 CK) is not below this

NP_AGREES = 1e-13                                        # grad_np in float64 against the C oracle: 8.1e-15 measured, one decade of margin
FP64_BAR = dict(yhat=FP64_TIGHT, x=FP64_TIGHT, nll=FP64_TIGHT, dx=1e-8, grad=1e-8)
TODAY32 = dict(yhat=FP32_TOL, x=FP32_TOL, nll=FP32_TOL, dx=FP32_TOL * 10, grad=FP32_TOL * 10)
# the reference's own float32 figures (REF32, measured, see the docstring) with half a decade of margin, never above TODAY32
REF32 = dict(d2=dict(yhat=2.8e-6, x=3.0e-6, dx=2.6e-6, nll=5.3e-6, grad=4.9e-6),
             d3=dict(yhat=4.9e-7, x=5.1e-7, dx=3.0e-6, nll=1.0e-5, grad=7.6e-6),
             stacked=dict(yhat=2.7e-6, x=1.4e-6, dx=8.5e-6, nll=2.9e-5, grad=3.4e-5))
REF32_SLACK = 2.0                                        # another numpy's summation order may move a recorded figure by this much; the bars stay
HALF_DECADE = 10 ** 0.5
FP32_BAR = {f: {q: min(REF32[f][q] * HALF_DECADE, TODAY32[q]) for q in QUANTITIES} for f in FAMILIES}


# ------------------------------------------------------------------------------------------------ the cases
def _k52(kern):
    return 1 if kern == "Matern52" else 0


# (route, kernel, L, T, variant): the seed of each route is that of the existing test which reaches it with the same shape
REF_CASES = (
    # test_gradstream_vs_oracle's seeds (L * 31 + T): the short-window instantiations (fp64: T <= 256, 2-tick chunks, segments of 128; fp32:
    # T <= 512, 4-tick chunks, segments of 256) up to the switch to the long-stream ones, and the suite's own cases
    [("vs", k, 3, T, None) for k in ("Matern32", "Matern52") for T in (1, 3, 127, 129, 255, 256, 257, 511, 512, 513)]
    + [("vs", "Matern32", 9, 128, None), ("vs", "Matern52", 70, 1030, None), ("vs", "Matern32", 4, 2600, None), ("vs", "Matern52", 6, 1500, None),
       ("vs", "Matern52", 8, 700, 0.01)]
    # test_gradstream_segment_boundaries_of_the_long_stream_kernels' seeds: one tick either side of one and two segments (512 / 1024 ticks)
    + [("seg", k, 3, T, None) for k in ("Matern32", "Matern52") for T in (1023, 1024, 1025, 2047, 2048, 2049)]
    # gaps: rows 0 .. 3 clean, row 4 never observed, rows 5 .. 7 with the listed ticks missing; two draws whose row 2 goes to the third pass
    + [("gaps", k, 8, 2600, "chosen") for k in ("Matern32", "Matern52")]
    + [("gaps", k, 8, 300, "short") for k in ("Matern32", "Matern52")]
    + list(UNSTABLE_CASES))
GAPS = dict(chosen=[0, 511, 512, 1023, 1024] + list(range(1500, 1520)) + [2047, 2048, 2599], short=[0, 127, 128, 200, 201, 202, 255, 256, 299])
STACKED_CASES = (
    # test_stacked_gradstream_vs_oracle's seeds (9 L + T + J): the tick-by-tick kernel
    [("xvs", k, L, T, nanf) for k in STACKED for L, T, nanf in ((3, 1, None), (5, 64, None), (4, 65, None), (7, 130, 0.05))]
    # test_stacked_gradstream_long_streams_vs_oracle's seeds (11 L + T + J): the time-parallel sweep and its tail
    + [("xlong", k, L, T, gap) for k in STACKED for L, T, gap in (
        (3, 512, None), (2, 543, None), (5, 2048, None), (3, 2081, None), (2, 4133, None),      # whole chunks, a tail, one segment, a chunk past it, two and a ragged end
        (4, 2500, (1700,)), (3, 1024, (0,)),                                                      # at most kFewGaps gapped chunks in a window: cut at them
        (4, 2100, (0, 31, 32, 2047, 2048, 2099)),                                                 # three in the first window, one in the second, one in the tail
        (3, 1100, "dense"))])                                                                     # more than kFewGaps: walked whole; row 2 never observed
CASES = tuple(REF_CASES) + tuple(STACKED_CASES)
METRIC_CASE = ("vs", "Matern32", 9, 128, None)          # the case the old bar hides most of (see the docstring)


def _cid(c):
    v = c[4]
    return "%s-%s-L%d-T%d%s" % (c[0], c[1], c[2], c[3], "" if v is None else "-" + (v if isinstance(v, str) else "gap" + "_".join(map(str, v)) if isinstance(v, tuple) else "nan%g" % v))


def family(kern):
    return "d2" if kern == "Matern32" else "d3" if kern == "Matern52" else "stacked"


def _inputs(c):
    """Parameters, stream and start states of one case, drawn in the order of the existing test named by its route."""
    route, kern, L, T, v = c
    J = int(kern[-1]) if kern in STACKED else 0
    if route == "vs":
        rng = np.random.default_rng(L * 31 + T)
        prm = synth_params(L, rng)
        Ty = synth(L, T, rng, v or 0.0)
        if v:
            Ty[:L // 2] = np.nan_to_num(Ty[:L // 2], nan=0.1)
    elif route == "seg":
        rng = np.random.default_rng(T * 7 + _k52(kern))
        prm = synth_params(L, rng)
        Ty = synth(L, T, rng)
    elif route == "gaps":
        rng = np.random.default_rng([T, _k52(kern), 20261020])
        prm = synth_params(L, rng)
        Ty = synth(L, T, rng)
        Ty[5:, GAPS[v]] = np.nan
        Ty[4, :] = np.nan
    elif route == "unstable":
        rng = np.random.default_rng([T, 20261020, UNSTABLE[kern][1]])
        prm = synth_params(L, rng)
        prm[2] = UNSTABLE[kern][0]
        Ty = synth(L, T, rng, 0.02)
        Ty[:2] = np.nan_to_num(Ty[:2], nan=0.1)
    elif route == "xvs":
        rng = np.random.default_rng(9 * L + T + J)
        prm = synth_params_stacked(L, J, rng)
        Ty = synth(L, T, rng, v or 0.0)
    else:
        assert route == "xlong"
        rng = np.random.default_rng(11 * L + T + J)
        prm = synth_params_stacked(L, J, rng)
        Ty = synth(L, T, rng)
        if v == "dense":
            Ty[1:, ::37] = np.nan
            Ty[2, :] = np.nan
        elif v is not None:
            Ty[1:, list(v)] = np.nan
    P = prm.shape[1]
    d = (2 if kern.startswith("Matern32") else 3) * max(J, 1)
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, P, d))
    return prm, round32(Ty), round32(x0), round32(dx0)         # fp32 numbers: one reference serves both precisions, input rounding is no error


# ------------------------------------------------------------------------------------------------ the reference and its scales
MATS = ("A", "K", "S", "HA", "AKHA", "dA", "dS", "dK", "dAKHA", "HdA")


def grad_np(igps, Ty, x0, dx0, dtype=np.float64):
    """oracle/moihgp_numpy.py::filter_stream(want_grad=True) (ihgp.h:37-57, :204-222) on the C oracle's matrices, vectorised over latents, every
    operation in `dtype`.  Besides the results it returns `scale`: what each entry is held against, accumulated in float64 along the trajectory
    (meant to be taken from the float64 run)."""
    f = np.dtype(dtype).type
    L, T = Ty.shape
    m = {k: np.stack([np.asarray(g.mat(k), dtype=np.float64) for g in igps]).astype(f) for k in MATS}
    A, K, S, HA, AKHA, dA, dS, dK, dAKHA, HdA = (m[k] for k in MATS)
    P = dS.shape[1]
    logS = np.log(S)
    Ty = Ty.astype(f)
    x = np.array(x0, dtype=f); dx = np.array(dx0, dtype=f)
    yhat = np.zeros((L, T), dtype=f); nll = np.zeros(L, dtype=f); grad = np.zeros((L, P), dtype=f)
    half = f(0.5); one = f(1)
    G = np.zeros((L, P)); N = np.zeros(L)
    xs = np.abs(x).astype(np.float64); dxs = np.abs(dx).astype(np.float64)
    S64, dS64, logS64 = S.astype(np.float64), dS.astype(np.float64), logS.astype(np.float64)
    with np.errstate(all="ignore"):
        for t in range(T):
            y = Ty[:, t]
            miss = np.isnan(y)
            obs = ~miss
            y0 = np.where(miss, f(0), y)
            # ihgp.h:204-222 on the pre-step (x, dx)
            v = y0 - np.einsum("li,li->l", HA, x)
            dv = -np.einsum("lpi,li->lp", HdA, x) - np.einsum("li,lpi->lp", HA, dx)
            w = v * v / S
            nll_t = half * (w + logS)
            g_t = (v[:, None] * dv - half * (w - one)[:, None] * dS) / S[:, None]
            nll = np.where(obs, nll + nll_t, nll)
            grad = np.where(obs[:, None], grad + g_t, grad)
            v64, dv64 = v.astype(np.float64), dv.astype(np.float64)
            w64 = v64 * v64 / S64
            G += np.where(obs[:, None], (np.abs(v64[:, None] * dv64) + 0.5 * np.abs(w64 - 1.0)[:, None] * np.abs(dS64)) / S64[:, None], 0.0)
            N += np.where(obs, 0.5 * (w64 + np.abs(logS64)), 0.0)
            # ihgp.h:37-57
            xn = np.einsum("lij,lj->li", AKHA, x) + K * y0[:, None]
            dxn = np.einsum("lpij,lj->lpi", dAKHA, x) + np.einsum("lij,lpj->lpi", AKHA, dx) + dK * y0[:, None, None]
            if miss.any():
                xm = np.einsum("lij,lj->li", A, x)
                dxm = np.einsum("lpij,lj->lpi", dA, x) + np.einsum("lij,lpj->lpi", A, dx)
                xn = np.where(miss[:, None], xm, xn)
                dxn = np.where(miss[:, None, None], dxm, dxn)
            x, dx = xn, dxn
            yhat[:, t] = x[:, 0]
            np.maximum(xs, np.abs(x), out=xs); np.maximum(dxs, np.abs(dx), out=dxs)
    for a in (x, dx, yhat, nll, grad):
        assert a.dtype == f
    up = lambda a: a.astype(np.float64)
    with np.errstate(all="ignore"):
        ymax = np.max(np.abs(up(yhat)), axis=1, initial=0.0)
    return dict(yhat=up(yhat), x=up(x), dx=up(dx), nll=up(nll), grad=up(grad),
                scale=dict(yhat=np.broadcast_to(ymax[:, None], yhat.shape), x=xs, dx=dxs, nll=N, grad=G))


def _calm(yhat):
    with np.errstate(all="ignore"):
        return np.all(np.isfinite(yhat), axis=1) & (np.max(np.abs(np.nan_to_num(yhat, nan=np.inf, posinf=np.inf, neginf=np.inf)), axis=1, initial=0.0) < CALM)


@functools.lru_cache(maxsize=None)
def case(c):
    """Inputs, the C oracle's structs and sweep, the float64 reference with its scales and the calm rows of one case: computed once, left unchanged."""
    from oracle import cref
    prm, Ty, x0, dx0 = _inputs(c)
    igps = cref.ihgp_array(c[1], DT, prm)
    with np.errstate(all="ignore"):
        o = cref.grad_stream(igps, Ty, x0=x0, dx0=dx0)
    ref = grad_np(igps, Ty, x0, dx0)
    for a in (Ty, x0, dx0) + tuple(ref[q] for q in QUANTITIES) + tuple(ref["scale"].values()):
        a.setflags(write=False)
    return dict(prm=prm, Ty=Ty, x0=x0, dx0=dx0, igps=igps, oracle=o, ref=ref, calm=_calm(o["yhat"]))


@functools.lru_cache(maxsize=None)
def case32(c):
    """The same loop in numpy.float32 (matrices rounded once from float64)."""
    C = case(c)
    return grad_np(C["igps"], C["Ty"], C["x0"], C["dx0"], dtype=np.float32)


def entry_errors(got, ref, rows):
    """Worst |got - ref| / scale per quantity over the rows `rows`, entry by entry; where a scale is exactly zero the value must be exactly zero."""
    out = {}
    for q in QUANTITIES:
        if got.get(q) is None:
            continue
        a = np.asarray(got[q], dtype=np.float64)[rows]; b = ref[q][rows]; s = np.asarray(ref["scale"][q])[rows]
        if q == "yhat":
            assert a.shape == b.shape
            out[q] = rel_err_rows(a, b)
            continue
        assert a.shape == b.shape == s.shape, (q, a.shape, b.shape, s.shape)
        zero = s == 0
        assert np.all(a[zero] == 0), (q, "nonzero where nothing can have been added")
        e = np.abs(a - b)[~zero] / s[~zero]
        assert np.all(np.isfinite(e)), q
        out[q] = float(e.max()) if e.size else 0.0
    return out


def _oracle_as_result(o):
    return dict(yhat=o["yhat"], x=o["x"], dx=o["dx"], nll=o["nll_per_latent"], grad=o["grad"])


def hidden(C, q):
    """(mask of the compared entries of quantity q below HIDDEN of the case's largest compared entry, number compared)."""
    a = np.abs(C["ref"][q][C["calm"]])
    return a < HIDDEN * a.max(), a.size


# ------------------------------------------------------------------------------------------------ CPU: the premises, from the reference alone
def test_numpy_restatement_equals_the_c_oracle():
    """grad_np in float64 against cref.grad_stream on every case, every quantity on its own scale: two correct evaluations of one loop, apart by
    summation order only."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for c in CASES:
        C = case(c)
        assert C["calm"].any(), _cid(c)
        for q, e in entry_errors(_oracle_as_result(C["oracle"]), C["ref"], C["calm"]).items():
            worst[q] = max(worst[q], e)
    print("grad_np (float64) against the C oracle, worst over %d cases: %s" % (len(CASES), ", ".join("%s %.1e" % kv for kv in worst.items())))
    assert max(worst.values()) < NP_AGREES, worst


def test_cases_are_calm_and_hide_entries_from_the_old_bar():
    """The conditions that keep the GPU tests from being vacuous (stated in the docstring)."""
    tot = dict(grad=[0, 0], dx=[0, 0])
    cover = {}
    for c in CASES:
        C = case(c)
        calm = C["calm"].mean()
        shares = {}
        for q in ("grad", "dx"):
            h, n = hidden(C, q)
            tot[q][0] += int(h.sum()); tot[q][1] += n
            shares[q] = h.mean()
            per_p = h.reshape(h.shape[0], h.shape[1], -1).any(axis=(0, 2))
            cover.setdefault((c[1], q), np.zeros(len(per_p), dtype=bool))
            cover[(c[1], q)] |= per_p
        print("%s: calm %.2f, hidden grad %.2f dx %.2f" % (_cid(c), calm, shares["grad"], shares["dx"]))
        assert calm >= 0.75, (_cid(c), calm)
    print("hidden over the list: grad %d of %d (%.2f), dx %d of %d (%.2f)" % (tot["grad"][0], tot["grad"][1], tot["grad"][0] / tot["grad"][1],
                                                                                tot["dx"][0], tot["dx"][1], tot["dx"][0] / tot["dx"][1]))
    for (kern, q), m in sorted(cover.items()):
        print("%s %s: parameters with hidden entries %s" % (kern, q, "".join("x" if b else "." for b in m)))
    assert tot["grad"][0] >= tot["grad"][1] / 3 and tot["dx"][0] >= tot["dx"][1] / 3
    for key, m in cover.items():
        assert m.all(), key


def chunk_ticks(T, prec):
    """The chunk length CK of the instantiation launch_grad_stream (grad.hip) picks for a stream of T ticks."""
    return (2 if T <= 256 else 8) if prec == "fp64" else (4 if T <= 512 else 16)


def largest_power(akha, T, prec):
    """max |AKHA^(16 CK)| per latent: what grad_scan_kernel holds against SEQ_LIMIT before it sweeps a latent (it tests nothing else: neither a
    spectral radius nor a status flag; grad_gen_kernel, the second pass, has no such test and never sees a latent flagged here)."""
    n = 16 * chunk_ticks(T, prec)
    with np.errstate(all="ignore"):
        return np.array([np.abs(np.linalg.matrix_power(np.asarray(m, dtype=np.float64), n)).max() for m in akha])


def third_pass_rows(akha, T, prec):
    return [int(l) for l in np.flatnonzero(~(largest_power(akha, T, prec) < SEQ_LIMIT[prec]))]       # (the kernel's own expression: a NaN is sent too)


def test_the_unstable_draws_meet_the_kernels_own_criterion():
    """What sends a latent to the sequential third pass is grad_scan_kernel's test on the largest power of its scan, not rho(AKHA) > 1.  Row 2 of
    the two `unstable` draws meets it where THIRD_PASS says (Matern32: fp32 only; Matern52: both precisions); nothing else on the list does.
    The other rows of those draws are ordinary: their largest power stays below one, so the case's fp32 figures are not those of a growing scan."""
    for c in REF_CASES:
        akha = [g.mat("AKHA") for g in case(c)["igps"]]
        for prec in ("fp64", "fp32"):
            pw = largest_power(akha, c[3], prec)
            sent = third_pass_rows(akha, c[3], prec)
            if c in UNSTABLE_CASES:
                print("%s %s: max |AKHA^%d| per latent %s, limit %g, sent to the third pass: %s"
                      % (_cid(c), prec, 16 * chunk_ticks(c[3], prec), " ".join("%.1e" % v for v in pw), SEQ_LIMIT[prec], sent))
                assert np.all(np.delete(pw, 2) < 1.0), (_cid(c), prec, pw)
                if (c, prec) in THIRD_PASS:
                    assert pw[2] > 1e6 * SEQ_LIMIT[prec]               # far enough over that the device's own matrices agree (asserted on the GPU)
            assert sent == ([2] if (c, prec) in THIRD_PASS else []), (_cid(c), prec, pw)
    for c in UNSTABLE_CASES:
        C = case(c)
        assert not C["calm"][2] and C["calm"].sum() == 4
        gapped = np.isnan(C["Ty"]).any(axis=1)
        assert not gapped[:2].any() and gapped[3:].all()               # rows 0, 1: first pass; rows 3, 4: second; row 2: third, in one launch


def test_reference_in_float32_has_room_under_the_bars():
    """The fp32 premise: grad_np in numpy.float32 against float64, worst per quantity and family over the list.  REF32 records these figures as
    one numpy gave them, and the device's bars are half a decade above the record.  numpy's float32 einsum sums in an order that changes with
    its version and the SIMD width, so the figure of the day is held to REF32_SLACK times the record, not to the record itself; it must also
    lie under the device's bar (the room for another rounding order is not used up by numpy alone), and no bar may exceed today's."""
    worst = {f: dict.fromkeys(QUANTITIES, 0.0) for f in FAMILIES}
    for c in CASES:
        C = case(c)
        for q, e in entry_errors(case32(c), C["ref"], C["calm"]).items():
            worst[family(c[1])][q] = max(worst[family(c[1])][q], e)
    for f in FAMILIES:
        print("reference float32 against float64, %s: %s" % (f, ", ".join("%s %.2e" % kv for kv in worst[f].items())))
    for f in FAMILIES:
        for q in QUANTITIES:
            assert worst[f][q] <= REF32_SLACK * REF32[f][q], (f, q, worst[f][q])
            assert worst[f][q] < FP32_BAR[f][q] <= TODAY32[q]


@pytest.mark.parametrize("q", ["grad", "dx"])
def test_entry_metric_sees_what_the_global_maximum_hides(q):
    """One hidden entry of the float64 reference moved by 1e-3 of its own scale: the old expression (global maximum, 1e-2) accepts, the new one
    rejects at the fp32 bar; and rejects a move of 1e-7 at the fp64 bar."""
    C = case(METRIC_CASE)
    ref = C["ref"]
    h, n = hidden(C, q)
    assert h.mean() > 0.5
    rows = np.flatnonzero(C["calm"])
    s = np.where(h, ref["scale"][q][C["calm"]], np.inf)
    i = np.unravel_index(np.argmin(s), s.shape)                        # the hidden entry with the smallest scale
    idx = (int(rows[i[0]]),) + tuple(int(j) for j in i[1:])
    for eps, bar in ((1e-3, FP32_BAR[family(METRIC_CASE[1])][q]), (1e-7, FP64_BAR[q])):
        got = {k: ref[k] for k in QUANTITIES}
        got[q] = ref[q].copy()
        got[q][idx] += eps * ref["scale"][q][idx]
        old = rel_err(got[q], ref[q])
        new = entry_errors(got, ref, C["calm"])[q]
        print("%s entry %s (value %.2e, scale %.2e, largest %.2e) moved by %g of its scale: old %.2e (bar 1e-2), new %.2e (bar %.1e)"
              % (q, idx, ref[q][idx], ref["scale"][q][idx], np.abs(ref[q]).max(), eps, old, new, bar))
        assert old < 1e-2 and new > bar


# ------------------------------------------------------------------------------------------------ GPU
_WORST = {}


@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import load_library
    from multioutputihgp_amd import streams
    lib = load_library()
    assert lib.moihgp_device_count() >= 1
    yield dict(streams=streams, lib=lib, torch=torch)
    for (prec, fam), w in sorted(_WORST.items()):
        print("device worst, %s %s: %s" % (prec, fam, ", ".join("%s %.2e" % (q, w[q]) for q in QUANTITIES if q in w)))


def _to_dev(env, a, dtype):
    torch = env["torch"]
    L, T = a.shape
    t = env["streams"].alloc_stream(L, T, dtype)
    t.zero_()
    t[:, :T] = torch.tensor(a, dtype=dtype)
    return t


def device_errors(env, c, prec, want_yhat):
    """One bank.grad call of one case on the device: the worst entry error per quantity over the calm rows."""
    torch = env["torch"]
    C = case(c)
    dtype = torch.float64 if prec == "fp64" else torch.float32
    bank = env["streams"].LatentBank(DT, C["prm"], kernel=KMAP.get(c[1], c[1]))
    T = c[3]
    r = bank.grad(_to_dev(env, C["Ty"], dtype), T=T, x=torch.tensor(C["x0"], dtype=dtype).cuda(), dx=torch.tensor(C["dx0"], dtype=dtype).cuda(), want_yhat=want_yhat)
    torch.cuda.synchronize()
    assert (r["yhat"] is not None) == want_yhat
    got = {q: (r[q][:, :T] if q == "yhat" else r[q]).cpu().numpy() for q in QUANTITIES if r[q] is not None}
    return entry_errors(got, C["ref"], C["calm"])


def _run(env, c, prec, want_yhat):
    e = device_errors(env, c, prec, want_yhat)
    bars = FP64_BAR if prec == "fp64" else FP32_BAR[family(c[1])]
    w = _WORST.setdefault((prec, family(c[1])), {})
    for q, v in e.items():
        w[q] = max(w.get(q, 0.0), v)
    print("%s %s %s: %s" % (_cid(c), prec, "means" if want_yhat else "no means", ", ".join("%s %.2e" % kv for kv in e.items())))
    for q, v in e.items():
        assert v < bars[q], (q, v, bars[q])


@pytest.mark.gpu
@pytest.mark.parametrize("want_yhat", [True, False], ids=["means", "nomeans"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("c", REF_CASES, ids=_cid)
def test_reference_models_entry_by_entry(env, c, prec, want_yhat):
    _run(env, c, prec, want_yhat)


@pytest.mark.gpu
@pytest.mark.parametrize("c", UNSTABLE_CASES, ids=_cid)
def test_the_third_pass_is_reached_on_the_device_matrices(env, c):
    """grad_scan_kernel's criterion (see test_the_unstable_draws_meet_the_kernels_own_criterion) on the matrices the device itself solved for:
    row 2 of the `unstable` draws, and no other, is left to grad_seq_kernel where THIRD_PASS says."""
    C = case(c)
    bank = env["streams"].LatentBank(DT, C["prm"], kernel=KMAP[c[1]])
    akha = [bank.latent(l)["AKHA"] for l in range(c[2])]
    for prec in ("fp64", "fp32"):
        pw = largest_power(akha, c[3], prec)
        print("%s %s: device max |AKHA^%d| per latent %s" % (_cid(c), prec, 16 * chunk_ticks(c[3], prec), " ".join("%.1e" % v for v in pw)))
        assert third_pass_rows(akha, c[3], prec) == ([2] if (c, prec) in THIRD_PASS else []), (prec, pw)


@pytest.mark.gpu
@pytest.mark.parametrize("want_yhat", [True, False], ids=["means", "nomeans"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("c", STACKED_CASES, ids=_cid)
def test_stacked_models_entry_by_entry(env, c, prec, want_yhat):
    _run(env, c, prec, want_yhat)
