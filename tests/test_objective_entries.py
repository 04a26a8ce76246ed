"""The full objective gradient [U (M L) | S (L) | sigma (1) | per-latent (L P)], the loss and the carried state of all three device routes (the
fused one-workgroup kernel and the multi-kernel path behind negLogLikelihood(x, y, dx), and the windowed objective of csrc/window.hip), every
entry against a conditioning scale of its own instead of max |a - b| over max |b| of the whole concatenated vector.

The reference and the scales are objective_reference.py's (its docstring states them).  Bars: fp64 is the only precision of these routes, and
the bars are FP64_BAR of test_gradient_entries.py: 1e-9 x scale for the loss and x, 1e-8 x scale for every gradient entry and dx.

Cases (every draw is objective_reference.draw: test_window_objective_vs_oracle_loop's, seed M + 3 L + W (+ J when stacked); the per-tick ABI
feeds three ticks forward with step, W = 3 in the seed):
    per-tick ABI, both kernels of KMAP, threading off and on (the flag changes only the loss), negLogLikelihood with and without gradient, step
        fused      (2, 1), (8, 4), (6, 6: m_n = 0, the residual is pure noise), (126, 65: the 64-lane stride over L), (128, 64: M L = 8192 exactly),
                   (91, 90: the largest L), (2940, 1: 6143 doubles of LDS, the last shape that fits; M strides the 256 threads eleven times)
        unfused    the same shapes with MOIHGP_TICK_FUSED=0 set before the handle is constructed
        multi      (129, 64: just past the fused limit, project_partial_kernel with three chunks), (2941, 1: past the LDS limit, threading forced
                   off), (2049, 3: the 32-chunk cap), (257, 257: M = L, one past the 256 stride of the finaliser in L and in M), (300, 255),
                   (300, 256).  fused_lik_fits, restated, refuses every one of them but (2049, 3): 6147 mixing entries and 4375 doubles of LDS fit
                   the one-workgroup kernel, so that shape reaches the multi-kernel path, whose 32-chunk cap it is listed for, only with
                   MOIHGP_TICK_FUSED=0; it runs that way here and, the default route being another kernel, fused as well
        stacked    every kernel of STACKED at (7, 3), Matern52x4 at (70, 65)
    window objective: loss, every gradient entry, xT and dxT
        W edges    (Matern52, 6, 4) and (Matern32, 5, 3) at W = 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512,
                   513, 1025: the 64-tick lane stride of window_z_kernel, the 256-thread stride of window_finalize_kernel, the k depth of the
                   U-gradient product at slabs of 16 and tiles of 32, the short / long window switch at 256 and the 128- / 512-tick segments
        tiles      both kernels at (130, 129, 17), (129, 128, 33), (128, 127, 16), (257, 5, 40), (300, 257, 3), (260, 256, 3: the finaliser's stride
                   over L), (8, 8, 16) and (64, 64, 20) (M = L), (3, 1, 9)
        threaded   (Matern52, 6, 4, 65) and (Matern52, 70, 33, 128): the loss carries the latent sums
        partial    (Matern52, 70, 33, 65) and (Matern32, 6, 3, 17) with NaN at tick 0 row 0 and at tick W / 2 in three rows: the NaN pattern is the
                   reference's (loss, U, S, sigma), the per-latent block and the state finite, entry by entry
        stacked    every kernel of STACKED at (7, 3, W), W = 1, 63, 64, 65 (the 64-tick rounds of grad_x_kernel with out_mode == 2), Matern52x2
                   at (9, 4, 130)
        device     (Matern52, 70, 33, 65) through window_objective_dev: bit-equal to the host form

A second, derived hold on the U block (objective_reference.u_rounding_bound).  The bar of 1e-8 x scale cannot see a single-precision factor in
front of pv: the scale of grad_U is dominated by |y_r| A_c / sigma (sigma = 0.04: many times the pv term), so 6e-8 of the pv term stays
under 1e-8 of the scale (7.4e-9 at most on build (a) below).  The U block is therefore also held to the first-order bound of its own
rounding error in fp64, term by term (the sums over W and M, the products, the carried state through HA x by its impulse response), against the restatement run on the device's own
polar factor (getParams), so that no input of the two evaluations differs: 1.3e-13 .. 1.5e-12 of the scale over the list, four decades under
the bar.  The bars above stay as they are and are asserted first.

Conditions (test_cases_hide_entries_from_the_old_bar; no seed had to be changed): of the compared entries, those below 1e-2 of their own case's
largest entry: U 1662279 of 2000639 (0.83), S 8666 of 8857 (0.98), per-latent 22075 of 28361 (0.78); each of the three blocks has such entries
in at least one case of every route (fused, multi-kernel, stacked ABI, window, stacked window).  sigma is a single entry and, wherever M > L, the
largest of its vector: hidden in one of 185 vectors (a stacked ABI tick), so no condition is put on it.
The metric test: in (Matern52, 70, 33, 128) (largest entry 1.17e5, sigma's) the S entry of the smallest scale (33.6) and the per-latent one
(1.405) moved by 1e-6 of their scale read 2.9e-10 and 1.2e-11 under the old expression and 1.0e-6 here.  No U entry of that draw can do the
same: the smallest U scale is 2.33e3, so a move of 1e-6 of it reads 1.98e-8 under the old expression; the old bar hides a U entry up to 5.0e-7
of its scale, and the U entry is moved by 4e-7 (old 7.9e-9, here 4.0e-7: forty bars).

Measured (CPU figures from the reference alone; device figures from one run on an MI355X, worst entry over all cases of the route):
    restatement against the C oracle's tick loop, 187 comparisons: U 5.1e-16, S 4.6e-15, sigma 2.6e-16, per-latent 8.3e-14, loss 2.3e-16,
    x 9.6e-14, dx 8.5e-13; NP_AGREES = 1e-11 is the worst with one decade of margin.  The last four are the rounding of Ty, an input perturbation
    to them that their scales do not hold (dx at (Matern52, 300, 255): an entry that cancels in all three ticks).  Smallest scale / |value| per
    block: U 1.01, S 1.00, sigma 1.51, per-latent 1.00: the scales are not slack.
                              U         S         sigma     per-lat.  loss      x         dx        U / rounding bound
    bar                       1e-08     1e-08     1e-08     1e-08     1e-09     1e-09     1e-08     1
    ABI fused                 4.52e-15  4.16e-14  4.11e-16  7.37e-13  2.47e-16  1.35e-13  4.19e-13  0.028
    ABI fused shapes, unfused 4.52e-15  4.16e-14  4.11e-16  7.37e-13  2.47e-16  1.35e-13  4.19e-13  0.028
    ABI multi-kernel          1.05e-14  1.86e-13  1.33e-15  6.52e-12  9.66e-16  2.01e-12  1.82e-11  0.0031
    ABI stacked               3.17e-15  4.91e-14  5.74e-16  7.18e-13  6.46e-17  1.54e-13  5.52e-12  0.016
    window, W edges           1.01e-14  4.08e-15  3.50e-16  2.39e-14  1.79e-16  2.41e-14  3.34e-13  0.022
    window, tiles             8.65e-15  7.32e-14  7.28e-16  2.32e-13  3.23e-16  9.23e-14  4.61e-13  0.010
    window, threaded          7.96e-16  3.29e-15  2.01e-16  1.79e-14  1.15e-16  1.97e-15  3.64e-14  0.0029
    window, partial           NaN       NaN       NaN       1.44e-13  NaN       4.64e-15  3.22e-14  -
    window, stacked           8.18e-16  5.99e-15  2.29e-16  2.16e-13  1.27e-16  1.05e-14  6.65e-12  0.013
    window, device form       5.68e-16  3.69e-15  2.14e-16  2.48e-14  8.08e-18  3.60e-15  3.22e-14  (bit-equal to the host form)
(The worst of the fused shapes is a shape of M <= 128, where both routes sum in the same order; at (2940, 1) the two differ.)  The device stays
under every bar and no defect was found.  The U figure of 1.01e-14 at (Matern52, 6, 4, W = 1) is the device's polar factor against the oracle's,
an input: on the device's own factor no W-edge case is above 0.022 of its rounding bound.

That it bites (two numerically wrong, otherwise identical builds of the library, loaded through MOIHGP_LIB, run once, not part of the tree;
"the existing tests" are the 81 cases of test_window_objective_vs_oracle_loop, test_reference_abi_vs_golden, _vs_oracle_larger,
_fuzz_vs_oracle, test_stacked_full_objects_vs_oracle, test_lik1_follows_the_threading_flag and test_learner_over_hip_library):
    (a) window_z_kernel with 1.0 / sq taken in single precision: all 81 existing cases passed.  Here all 62 window cases of the reference's
        kernels with a finite U block failed (42 W edges, 18 tiles, 2 threaded), every one on the rounding bound (1e5 .. 7e5 times it) and none
        on the 1e-8 bar (U at 7.4e-9 of its scale at most, as worked out above); the stacked windows (window_z_x_kernel, untouched), the two
        partially observed ones (U block NaN) and the per-tick ABI passed
    (b) nll_finalize_body with 0.5 / Sl taken in single precision: 80 of the 81 existing cases passed (the one that failed: the fuzz case with
        M = L = 1).  Here 86 of the 98 per-tick ABI cases failed, all on the S block against the 1e-8 bar; the 12 that passed are (2940, 1) and
        (2941, 1), where the M terms of A make 1/2 / S a small share of the S scale; the window cases (window_finalize_kernel, untouched) passed
"""
import numpy as np
import pytest

import objective_reference as oref
from objective_reference import BLOCKS, QUANTITIES, case, entry_errors, fused_lik_fits, hidden, old_measure, oracle_loop
from parity_support import FP64_TIGHT, KMAP, STACKED

ROUNDING = "U over its rounding bound"
FP64_BAR = dict(loss=FP64_TIGHT, x=FP64_TIGHT, U=1e-8, S=1e-8, sigma=1e-8, lat=1e-8, dx=1e-8)      # test_gradient_entries.FP64_BAR, per block
NP_AGREES = 1e-11                                        # the restatement against the C oracle: 8.5e-13 measured (dx), one decade of margin
REF_KERNELS = ("Matern32", "Matern52")
ABI_TICKS = 3

FUSED_SHAPES = ((2, 1), (8, 4), (6, 6), (126, 65), (128, 64), (91, 90), (2940, 1))
MULTI_SHAPES = ((129, 64), (2941, 1), (2049, 3), (257, 257), (300, 255), (300, 256))
FITS_ANYWAY = ((2049, 3),)                               # listed for the multi-kernel path, accepted by fused_lik_fits (see the docstring)
ABI_STACKED = tuple((k, 7, 3) for k in STACKED) + (("Matern52x4", 70, 65),)
# (route, kernel, M, L): route = fused | unfused | multi | stacked
ABI_CASES = (tuple(("fused", k, M, L) for k in REF_KERNELS for M, L in FUSED_SHAPES + FITS_ANYWAY)
             + tuple(("unfused", k, M, L) for k in REF_KERNELS for M, L in FUSED_SHAPES)
             + tuple(("multi", k, M, L) for k in REF_KERNELS for M, L in MULTI_SHAPES)
             + tuple(("stacked", k, M, L) for k, M, L in ABI_STACKED))

W_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)
TILE_SHAPES = ((130, 129, 17), (129, 128, 33), (128, 127, 16), (257, 5, 40), (300, 257, 3), (260, 256, 3), (8, 8, 16), (64, 64, 20), (3, 1, 9))
# (route, kernel, M, L, W, variant): variant = None | "threaded" | "nan"
WINDOW_CASES = (tuple(("edges", "Matern52", 6, 4, W, None) for W in W_EDGES) + tuple(("edges", "Matern32", 5, 3, W, None) for W in W_EDGES)
                + tuple(("tiles", k, M, L, W, None) for k in REF_KERNELS for M, L, W in TILE_SHAPES)
                + (("threaded", "Matern52", 6, 4, 65, "threaded"), ("threaded", "Matern52", 70, 33, 128, "threaded"))
                + (("partial", "Matern52", 70, 33, 65, "nan"), ("partial", "Matern32", 6, 3, 17, "nan"))
                + tuple(("xwindow", k, 7, 3, W, None) for k in STACKED for W in (1, 63, 64, 65)) + (("xwindow", "Matern52x2", 9, 4, 130, None),))
DEV_CASE = ("Matern52", 70, 33, 65)
METRIC_CASE = ("Matern52", 70, 33, 128)                 # test_window_objective_vs_oracle_loop's own draw (seed 297)
HIDING_ROUTES = ("fused", "multi", "stacked", "window", "xwindow")


def _aid(c):
    return "%s-%s-M%d-L%d" % c


def _wid(c):
    return "%s-%s-M%d-L%d-W%d%s" % (c[:5] + ("" if c[5] is None else "-" + c[5],))


def abi_case(c):
    return case(c[1], c[2], c[3], ABI_TICKS)


def window_case(c):
    return case(c[1], c[2], c[3], c[4], c[5] == "nan")


def _references():
    """(route for the hiding condition, label, case, list of (reference result, loss key)) over the whole list, each reference once."""
    seen = set()
    for c in ABI_CASES:
        key = c[1:]
        if key in seen:
            continue
        seen.add(key)
        C = abi_case(c)
        yield ("fused" if c[0] == "unfused" else c[0]), _aid(c), C, C["ref"]["ticks"]
    seen = set()
    for c in WINDOW_CASES:
        key = (c[1], c[2], c[3], c[4], c[5] == "nan")
        if key in seen:
            continue
        seen.add(key)
        C = window_case(c)
        yield ("xwindow" if c[0] == "xwindow" else "window"), _wid(c), C, [C["ref"]]


# ------------------------------------------------------------------------------------------------ CPU: the premises, from the reference alone
def test_restatement_equals_the_c_oracle():
    """window_np against the tick loop of cref.GP on every case, every entry within NP_AGREES of its scale (two evaluations of one formula, apart
    by summation order and by the rounding of Ty, which enters the per-latent block as an input perturbation); and every scale is at least the
    magnitude of the value it belongs to."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    slack = dict.fromkeys(BLOCKS, np.inf)
    n = 0
    for route, label, C, refs in _references():
        M, L, P = C["M"], C["L"], C["P"]
        o = oracle_loop(C)
        on = oracle_loop(C, threading=True) if L >= 2 else o
        pairs = [(C["ref"], o, on)] if route in ("window", "xwindow") else list(zip(refs, o["ticks"], on["ticks"]))
        for ref, got, got_on in pairs:
            n += 1
            e = entry_errors(got, ref, M, L, P)
            e["loss"] = max(e["loss"], entry_errors(dict(loss=got_on["loss"]), ref, M, L, P, "loss_on" if L >= 2 else "loss")["loss"])
            if "lik2" in got:
                e["loss"] = max(e["loss"], entry_errors(dict(loss=got["lik2"]), ref, M, L, P, "loss_on")["loss"])
            for q, v in e.items():
                worst[q] = max(worst[q], v)
            for k, sl in oref.blocks(M, L, P).items():
                g, s = ref["grad"][sl], ref["scale"]["grad"][sl]
                fin = ~np.isnan(g)
                assert np.all(s[fin] >= np.abs(g[fin]) * (1 - 1e-12)), (label, k)
                nz = fin & (g != 0)
                if nz.any():
                    slack[k] = min(slack[k], float((s[nz] / np.abs(g[nz])).min()))
            for key in ("loss", "loss_on"):
                if np.isfinite(ref[key]):
                    assert ref["scale"][key] >= abs(ref[key]) * (1 - 1e-12), (label, key)
    print("restatement against the C oracle, worst over %d comparisons: %s" % (n, ", ".join("%s %.1e" % kv for kv in worst.items())))
    print("smallest scale / |value| per block: %s" % ", ".join("%s %.2f" % kv for kv in slack.items()))
    assert max(worst.values()) < NP_AGREES, worst


def test_cases_hide_entries_from_the_old_bar():
    """The conditions that keep the GPU tests from being vacuous: over the whole list at least half of the compared U entries and at least half
    of the compared S entries lie below HIDDEN of their own case's largest entry, and the U, S and per-latent blocks have such entries in at
    least one case of every route (sigma is a single entry and, wherever M > L, the largest of the vector)."""
    tot = {k: [0, 0] for k in BLOCKS}
    cover = {}
    for route, label, C, refs in _references():
        row = {k: [0, 0] for k in BLOCKS}
        for ref in refs:
            for k, (h, n) in hidden(ref, C["M"], C["L"], C["P"]).items():
                row[k][0] += h; row[k][1] += n
        for k in BLOCKS:
            tot[k][0] += row[k][0]; tot[k][1] += row[k][1]
            cover[(route, k)] = cover.get((route, k), False) or row[k][0] > 0
        print("%s: hidden %s" % (label, ", ".join("%s %d/%d" % (k, row[k][0], row[k][1]) for k in BLOCKS)))
    print("hidden over the list: %s" % ", ".join("%s %d of %d (%.2f)" % (k, tot[k][0], tot[k][1], tot[k][0] / max(tot[k][1], 1)) for k in BLOCKS))
    print("routes with hidden entries: %s" % ", ".join("%s/%s %s" % (r, k, "yes" if v else "no") for (r, k), v in sorted(cover.items())))
    assert 2 * tot["U"][0] >= tot["U"][1] and 2 * tot["S"][0] >= tot["S"][1]
    for route in HIDING_ROUTES:
        for k in ("U", "S", "lat"):
            assert cover[(route, k)], (route, k)


def _nudge(v, s, eps):
    """v moved towards +inf by eps of s, and on by single floats until the move reads eps under the entry measure."""
    got = v + eps * s
    while abs(got - v) / s < eps:
        got = np.nextafter(got, np.inf)
    return got


@pytest.mark.parametrize("block,eps", [("U", 4e-7), ("S", 1e-6), ("lat", 1e-6)])
def test_entry_metric_sees_what_the_global_maximum_hides(block, eps):
    """One entry of the reference gradient of (Matern52, 70, 33, 128), the one of its block with the smallest scale, moved by eps of that scale:
    it reads at least eps here, forty to a hundred bars, and under 1e-8 in the old expression, which accepts it.  eps is 1e-6 for the S and the
    per-latent entry.  No U entry of this draw can be moved by 1e-6 of its scale and stay under 1e-8 of the largest entry (1.17e5, sigma's): the
    smallest U scale is 2.33e3 (128 ticks of |y_r| A_c / sigma: the absolute terms of U^T y_t do not cancel as its signed terms do), so such a
    move reads 1.98e-8 there; the old bar hides a U entry up to 1e-8 x 1.17e5 / 2.33e3 = 5.0e-7 of its scale, and 4e-7 is moved."""
    C = case(*METRIC_CASE)
    M, L, P = C["M"], C["L"], C["P"]
    ref = C["ref"]
    sl = oref.blocks(M, L, P)[block]
    i = sl.start + int(np.argmin(ref["scale"]["grad"][sl]))
    s, top = ref["scale"]["grad"][i], np.abs(ref["grad"]).max()
    g = ref["grad"].copy()
    g[i] = _nudge(g[i], s, eps)
    new = entry_errors(dict(grad=g), ref, M, L, P)
    old = old_measure(g, ref["grad"])
    print("%s entry %d (value %.3e, scale %.3e, largest of the vector %.3e) moved by %g of its scale: old %.2e (bar 1e-8), new %.2e (bar %.0e)"
          % (block, i - sl.start, ref["grad"][i], s, top, eps, old, new[block], FP64_BAR[block]))
    assert new[block] >= eps and old < 1e-8
    assert eps >= 40 * FP64_BAR[block]
    assert all(v == 0 for k, v in new.items() if k != block)
    if eps < 1e-6:
        assert 1e-6 * s / top > 1e-8                     # why this block's entry is moved by less than the others
    if block == "lat":
        assert abs(ref["grad"][i]) < oref.HIDDEN * top


def test_the_listed_shapes_take_the_routes_they_are_listed_for():
    """fused_lik_fits (csrc/tick.hip) restated: accepts every fused shape, 2940 x 1 with one double of LDS to spare, and refuses every
    multi-kernel shape but (2049, 3)."""
    for M, L in FUSED_SHAPES:
        assert fused_lik_fits(M, L), (M, L)
    assert 2 * 2940 + 7 + 256 == 6143 and not fused_lik_fits(2941, 1) and 128 * 64 == 8192 and not fused_lik_fits(129, 64)
    for M, L in MULTI_SHAPES:
        assert fused_lik_fits(M, L) == ((M, L) in FITS_ANYWAY), (M, L)


# ------------------------------------------------------------------------------------------------ GPU
_WORST = {}


@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import MOIHGP, load_library
    lib = load_library()
    assert lib.moihgp_device_count() >= 1, "the library sees no device"
    yield dict(MOIHGP=MOIHGP, lib=lib, torch=torch)
    for route, w in sorted(_WORST.items()):
        print("device worst, %s: %s" % (route, ", ".join("%s %.2e" % (q, w[q]) for q in QUANTITIES + (ROUNDING,) if q in w)))


def _hold(route, label, e):
    """Record and assert one comparison: every quantity under its bar; the U block also within its rounding bound (a share of it below one)."""
    w = _WORST.setdefault(route, {})
    for q, v in e.items():
        w[q] = max(w.get(q, 0.0), v)
    print("%s: %s" % (label, ", ".join("%s %.2e" % kv for kv in e.items())))
    for q, v in e.items():
        assert v < (1.0 if q == ROUNDING else FP64_BAR[q]), (label, q, v)


def _device_reference(gp, C):
    """The restatement run on the device's own polar factor (getParams), for u_rounding_bound: no input of the two evaluations differs."""
    return oref.window_np(oref.Model(C["gp"], U=gp.params[:C["M"] * C["L"]]), C["Y"], C["x0"], C["dx0"])


def _u_share(grad, ref, C, W):
    """Worst |grad_U - reference on the same mixing| over its rounding bound, entry by entry."""
    M, L = C["M"], C["L"]
    err = np.abs(np.asarray(grad)[:M * L] - ref["grad"][:M * L])
    bound = oref.u_rounding_bound(ref, M, L, W, C["d"])
    assert np.all(np.isfinite(err)) and np.all(bound > 0) and np.all(bound < 1e-3 * FP64_BAR["U"] * ref["scale"]["grad"][:M * L])
    return float((err / bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("threading", [False, True], ids=["serial", "threaded"])
@pytest.mark.parametrize("c", ABI_CASES, ids=_aid)
def test_per_tick_abi_entry_by_entry(env, c, threading, monkeypatch):
    """negLogLikelihood(x, y, dx), negLogLikelihood(x, y) and step over three ticks, the device's own state fed forward as the callers do; each
    tick against the reference's tick on the reference's trajectory."""
    route, kern, M, L = c
    if route == "fused":
        assert fused_lik_fits(M, L)
    elif route == "multi" and (M, L) not in FITS_ANYWAY:
        assert not fused_lik_fits(M, L)
    if route == "unfused" or (route == "multi" and (M, L) in FITS_ANYWAY):
        monkeypatch.setenv("MOIHGP_TICK_FUSED", "0")                   # read in the constructor
    C = abi_case(c)
    P = C["P"]
    gp = env["MOIHGP"](oref.DT, M, L, kernel=KMAP.get(kern, kern), threading=threading)
    assert env["lib"].moihgp_get_threading(gp.handle) == (1 if threading and L >= 2 else 0)
    gp.update(C["params"])
    key = "loss_on" if threading and L >= 2 else "loss"
    x, dx = C["x0"], C["dx0"]
    same_mixing = _device_reference(gp, C)["ticks"]
    for t, (y, ref) in enumerate(zip(C["Y"], C["ref"]["ticks"])):
        l1, g1 = gp.negLogLikelihood(x, y, dx)
        l2 = gp.negLogLikelihood(x, y)
        xn, _, dxn = gp.step(x, y, dx)
        e = entry_errors(dict(loss=l1, grad=g1, x=xn, dx=dxn), ref, M, L, P, key)
        e["loss"] = max(e["loss"], entry_errors(dict(loss=l2), ref, M, L, P, "loss_on")["loss"])
        e[ROUNDING] = _u_share(g1, same_mixing[t], C, 1)
        _hold("abi " + route, "%s %s tick %d" % (_aid(c), "threaded" if threading else "serial", t), e)
        x, dx = xn, dxn


def _window(env, c):
    route, kern, M, L, W, variant = c
    C = window_case(c)
    threading = variant == "threaded"
    gp = env["MOIHGP"](oref.DT, M, L, kernel=KMAP.get(kern, kern), threading=threading)
    gp.update(C["params"])
    loss, grad, xT, dxT = gp.window_objective(C["Y"], C["x0"], C["dx0"])
    return C, gp, dict(loss=loss, grad=grad.copy(), x=xT, dx=dxT)


@pytest.mark.gpu
@pytest.mark.parametrize("c", WINDOW_CASES, ids=_wid)
def test_window_objective_entry_by_entry(env, c):
    """window_objective(Y, x0, dx0): the loss, every gradient entry and the state after the window."""
    route, kern, M, L, W, variant = c
    C, gp, got = _window(env, c)
    ref = C["ref"]
    if variant == "nan":
        sl = oref.blocks(M, L, C["P"])
        assert np.isnan(ref["loss"]) and np.isnan(ref["grad"][:sl["lat"].start]).all() and np.isfinite(ref["grad"][sl["lat"]]).all()
        assert np.isnan(got["loss"]) and np.isfinite(got["x"]).all() and np.isfinite(got["dx"]).all()
    else:
        assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss_on"])
    e = entry_errors(got, ref, M, L, C["P"], "loss_on" if variant == "threaded" else "loss")
    if variant != "nan":
        e[ROUNDING] = _u_share(got["grad"], _device_reference(gp, C), C, W)
    _hold("window " + route, _wid(c), e)


@pytest.mark.gpu
def test_window_objective_on_the_device_is_bit_equal_to_the_host_form(env):
    """window_objective_dev on the installed window: the same kernels writing into the caller's arrays."""
    torch = env["torch"]
    kern, M, L, W = DEV_CASE
    c = ("device", kern, M, L, W, None)
    C, gp, host = _window(env, c)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    loss_d = torch.zeros(1, dtype=torch.float64).cuda(); grad_d = torch.zeros(gp.num_param, dtype=torch.float64).cuda()
    x_d = torch.zeros(L * C["d"], dtype=torch.float64).cuda(); dx_d = torch.zeros(L * C["P"] * C["d"], dtype=torch.float64).cuda()
    gp.window_objective_dev(dev(C["x0"]).reshape(-1), dev(C["dx0"]).reshape(-1), loss_d, grad_d, x_d, dx_d)
    torch.cuda.synchronize()
    got = dict(loss=float(loss_d.cpu()[0]), grad=grad_d.cpu().numpy(), x=x_d.cpu().numpy().reshape(L, -1), dx=dx_d.cpu().numpy().reshape(L, C["P"], -1))
    for q in ("loss", "grad", "x", "dx"):
        assert np.array_equal(np.asarray(got[q]), np.asarray(host[q])), q
    e = entry_errors(got, C["ref"], M, L, C["P"])
    e[ROUNDING] = _u_share(got["grad"], _device_reference(gp, C), C, W)
    _hold("window device", _wid(c), e)
