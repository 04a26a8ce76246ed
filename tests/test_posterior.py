"""Exact smoothing across missing ticks (include/moihgp.h moihgp_posterior_stream): the numpy definition (posterior_reference.posterior_np) held
against the dense GP posterior over the observed ticks on the CPU, then the library against the definition on the GPU.

The kernels walk in blocks of B = 16 ticks (a checkpoint each) and move the rows through LDS in tiles of TILE = 32 ticks, 64 latents per
wavefront with the latent on the lane: T_DEVICE and L_DEVICE below sit on those edges.

Tolerances.  CPU, definition against the dense posterior: means 1e-10 of the row's largest |mean| (floor 1e-3), variances 2e-8 per entry,
relative, nll 1e-10 relative; measured 1.2e-12, 1.6e-9 (the dense solve's error on the draws with R = 1e-6) and 1.1e-12.  GPU: means and end
states at the project's FP64_TIGHT / FP32_TOL relative to the row's largest entry, nll 1e-9 relative.  fp64 variances and P_end, per entry:
ten times the draw's rounding figure (rounding_figure below, the figure the CPU test records and caps: the definition in np.float64 against the same lines in
np.longdouble, a few 1e-15 on most draws, 4e-12 at R = 1e-3, 2e-11 (Matern-3/2) and 3e-10 (Matern-5/2) at R = 1e-6), with a floor of 8 ulps; the
device is compared with the longdouble evaluation, the better estimate of the definition's value, on the device's own A (LatentBank.latent),
which isolates the walk from the matrix exponential.  An entry of P_end is measured against sqrt(P_ii P_jj): its off-diagonal entries pass
through zero.  fp32 variances: FP32_TOL per entry, relative.

Measured on an MI355X (test_posterior_parity, worst over its cases): fp64 means 2.4e-13, end states 3.6e-13, nll 3.2e-13, variances 0.47 of
their bound (the largest error, 1.3e-09, on the Matern-5/2 draw with R = 1e-6); fp32 means and end states 5.9e-8."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from edges_reference import exact_np
from posterior_reference import dense_nll_np, dense_posterior_np, model_tables, posterior_np
from stream_reference import project_np, tables
from stream_support import (FP32_TOL, FP64_TIGHT, KMAP, POOL, assert_declared, assert_exported, bank_of, cxx_fmt, cxx_rows, cxx_run,
                            cxx_test_binary, env, padding_untouched, sentinel_out, tdt_of, to_dev, to_dev_poison, tol_of)  # noqa: F401  (env: the module's fixture)

SYMBOLS = ("moihgp_posterior_stream",)
KERNS = ("Matern32", "Matern52")
B, TILE = 16, 32                                   # kPostBlock, kPostTile of stream_tables.h
T_DENSE = (1, 2, 17, 63, 300)
T_DEVICE = (1, 2, B - 1, B, B + 1, TILE - 1, TILE + 1, 300, 1025)
L_DEVICE = (1, 63, 64, 65, 130)
MEAN_TOL, VAR_TOL, NLL_TOL = 1e-10, 2e-8, 1e-10
ULP_FLOOR = 8 * np.finfo(np.float64).eps


def stream_of(L, T, rng):
    t = np.arange(T)[None, :]
    return np.sin(0.05 * t + 1.0 + np.arange(L)[:, None]) + 0.3 * rng.standard_normal((L, T))


def row_err(got, ref, floor=1e-3):
    """Worst row of max |got - ref| over the row's max |ref| (at least `floor`)."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), floor)))


def entry_err(got, ref):
    """Per entry, relative; [L] the worst of each row."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return np.max(np.abs(got - ref) / np.abs(ref), axis=1) if ref.shape[1] else np.zeros(ref.shape[0])


def cov_err(got, ref):
    """[L]: the worst entry of |got - ref| over sqrt(ref_ii ref_jj), per latent."""
    sd = np.sqrt(np.abs(np.einsum("lii->li", ref)))
    return np.max(np.abs(got - ref) / (sd[:, :, None] * sd[:, None, :]), axis=(1, 2))


def nll_err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


def masks_of(T, rng):
    """The CPU test's six masks [6][T]: none missing, the first tick, the last two ticks, a run of T / 8 + 1 ticks, isolated ticks, all."""
    m = np.zeros((6, T), dtype=bool)
    m[1, 0] = True
    m[2, max(T - 2, 0):] = True
    a = T // 3
    m[3, a:a + T // 8 + 1] = True
    m[4] = rng.random(T) < 0.15
    m[4, T // 2] = True
    m[5] = True
    return m


_FIGURE = {}


def rounding_figure(tb):
    """The fp64 rounding error of the definition on the model tb: posterior_np in np.float64 against the same lines in np.longdouble, the worst
    entry of var (relative) and of P_end (over sqrt(P_ii P_jj)).  The variances depend on the mask alone, not on the observations, and so does
    their rounding error: it peaks where an isolated tick is missing among the first ticks of a low-noise stream (P is still far from steady
    and var there is a small difference of large terms; at R = 1e-6 two fp64 evaluations in different orders of summation differ from the
    80-bit value by 1.4e-11 to 9e-10 at such a tick).  So the rows are: T = 63 and 300 gap-free, with a gap of T / 8 + 1 ticks and 10 %
    scattered, with the two ends missing; and T = 31 with one tick missing at each of the ticks 1 .. 8, alone and with the tick two further on.
    Without the last rows the figure of Matern-5/2 (1.3, 0.8, 1e-6) is 3.9e-11 and the device misses ten times it by 3.2 x (L = 64, T = 16) and
    2.6 x (L = 65, T = 15), at such ticks; no other draw passes 0.47 of its bound either way."""
    key = (tb["A"].tobytes(), tb["Pinf"].tobytes(), tb["R"])
    if key not in _FIGURE:
        rng = np.random.default_rng(5)
        streams = []
        for T in (63, 300):
            y = stream_of(3, T, rng)
            y[1, T // 3:T // 3 + T // 8 + 1] = np.nan
            y[1, rng.random(T) < 0.1] = np.nan
            y[2, 0] = np.nan; y[2, T - 5:] = np.nan
            streams.append(y)
        y = stream_of(16, 31, rng)
        for t in range(1, 9):
            y[t - 1, t] = np.nan
            y[t + 7, [t, t + 2]] = np.nan
        streams.append(y)
        worst = 0.0
        for y in streams:
            n = y.shape[0]
            a, b = posterior_np([tb] * n, y), posterior_np([tb] * n, y, np.longdouble)
            worst = max(worst, float(np.max(np.abs(a["var"] - b["var"]) / b["var"])), float(np.max(cov_err(a["P_end"], b["P_end"]))))
        _FIGURE[key] = worst
    return _FIGURE[key]


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_posterior():
    assert_declared(SYMBOLS)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moihgp.h")).read()
    assert "ceil(T / 16)" in text and "pivoted elimination" in text


def test_library_exports_the_posterior(hip_built):
    assert_exported(hip_built, SYMBOLS)


def test_cxx_predict_posterior_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "posterior_test"))


@pytest.mark.parametrize("kern", KERNS)
def test_definition_is_the_dense_posterior(kern):
    """posterior_np against the dense posterior restricted to the observed ticks, over the whole POOL, T_DENSE and the six masks: means,
    variances, nll, and the one-tick-ahead predictive mean (A x)_0 and variance (A P_end A^T + Q)_00 from the end state."""
    rng = np.random.default_rng(17)
    worst = np.zeros(5)
    for prm in POOL:
        tb = model_tables(kern, 0.1, prm)
        for T in T_DENSE:
            y = np.tile(np.sin(0.05 * np.arange(T) + 1.0) + 0.3 * rng.standard_normal(T), (6, 1))
            y[masks_of(T, rng)] = np.nan
            r = posterior_np([tb] * 6, y)
            assert not r["status"].any()
            for k in range(6):
                mean, var = dense_posterior_np(tb, y[k], 1)
                nll = dense_nll_np(tb, y[k])
                scale = max(float(np.max(np.abs(mean[:T]))), 1e-3)
                em = float(np.max(np.abs(r["mean"][k] - mean[:T]))) / scale
                ev = float(np.max(np.abs(r["var"][k] - var[:T]) / var[:T]))
                en = abs(float(r["nll"][k]) - nll) / max(abs(nll), 1e-300)
                xa = tb["A"] @ r["x"][k]
                Pa = tb["A"] @ r["P_end"][k] @ tb["A"].T + r["Q"][k]
                ea, eva = abs(xa[0] - mean[T]) / scale, abs(Pa[0, 0] - var[T]) / var[T]
                worst = np.maximum(worst, [em, ev, en, ea, eva])
                assert em <= MEAN_TOL and ev <= VAR_TOL and en <= NLL_TOL and ea <= MEAN_TOL and eva <= VAR_TOL, (prm, T, k, em, ev, en, ea, eva)
            # an all-missing row is the prior
            assert np.all(r["mean"][5] == 0.0) and np.all(r["var"][5] == tb["Pinf"][0, 0]) and r["nll"][5] == 0.0
    print(f"{kern}: worst mean {worst[0]:.1e} var {worst[1]:.1e} nll {worst[2]:.1e} ahead mean {worst[3]:.1e} ahead var {worst[4]:.1e}")


@pytest.mark.parametrize("kern", KERNS)
def test_gap_free_definition_equals_exact_edge_smoothing(kern):
    """Without missing ticks the recursion and exact-edge smoothing by its formulas at every tick (edges_reference.exact_np, full) are the same
    posterior: means, end states and variances to 1e-10 (measured 1.7e-14, 3.3e-13 and 1.7e-11, the last on the draws with R = 1e-6)."""
    rng = np.random.default_rng(18)
    worst = np.zeros(3)
    for prm in POOL:
        tb = tables(kern, 0.1, prm)
        for T in T_DENSE:
            y = stream_of(1, T, rng)
            e, r = exact_np([tb], y, full=True), posterior_np([tb], y)
            errs = [row_err(r["mean"], e["ys"]), row_err(r["x"], e["x"]), float(np.max(entry_err(r["var"], e["var"])))]
            worst = np.maximum(worst, errs)
            assert max(errs) <= 1e-10, (prm, T, errs)
    print(f"{kern}: worst mean {worst[0]:.1e} x {worst[1]:.1e} var {worst[2]:.1e}")


@pytest.mark.parametrize("kern", KERNS)
def test_steady_variance_is_far_too_small_inside_a_gap(kern):
    """What the feature rests on: T = 400, a 30-tick gap, the first tick and the last five ticks missing, 5 % scattered.  In the middle of the
    gap the dense posterior variance is at least 10 x var_smoothed on every POOL draw (the smallest ratio measured is 22.3), and the definition
    follows the dense variance there."""
    rng = np.random.default_rng(17)
    T, g0 = 400, 180
    for prm in POOL:
        tb = tables(kern, 0.1, prm)
        y = np.sin(0.05 * np.arange(T) + 1.0) + 0.3 * rng.standard_normal(T)
        y[g0:g0 + 30] = np.nan; y[0] = np.nan; y[T - 5:] = np.nan
        y[rng.random(T) < 0.05] = np.nan
        _, var = dense_posterior_np(tb, y, 1)
        ratio = var[g0 + 15] / tb["var_s"]
        print(f"{kern} {prm}: dense variance in the gap / var_smoothed = {ratio:.3g}")
        assert ratio >= 10.0, (prm, ratio)
        r = posterior_np([tb], y[None, :])
        assert abs(r["var"][0, g0 + 15] - var[g0 + 15]) <= VAR_TOL * var[g0 + 15]


@pytest.mark.parametrize("kern", KERNS)
def test_fp64_rounding_of_the_definition(kern):
    """The figures the device's fp64 variances are held to (ten times these): the definition in fp64 against the same lines in 80-bit arithmetic,
    per pool draw.  Measured: 1.5e-15 - 5.3e-14, 1.7e-13 and 4.2e-12 at R = 1e-3, 1.7e-11 and 3.1e-10 at R = 1e-6.  They must leave the dense bar room."""
    assert np.finfo(np.longdouble).eps < 1e-18
    for prm in POOL:
        fig = rounding_figure(model_tables(kern, 0.1, prm))
        print(f"{kern} {prm}: fp64 against 80-bit {fig:.1e}")
        assert 0.0 < fig <= VAR_TOL / 10


# ------------------------------------------------------------------------------------------------ GPU
def masked_stream(L, T, rng):
    """Rows whose masks differ from lane to lane: 10 % scattered, every other row a run of T / 8 + 1 ticks at its own place, a row in four the
    first tick, a row in four the last two ticks, a row in sixteen wholly missing."""
    Ty = stream_of(L, T, rng)
    miss = rng.random((L, T)) < 0.1
    for l in range(L):
        if l % 2 == 0:
            a = (7 * l) % max(T - T // 8, 1)
            miss[l, a:a + T // 8 + 1] = True
        if l % 4 == 1:
            miss[l, 0] = True
        if l % 4 == 2:
            miss[l, max(T - 2, 0):] = True
        if l % 16 == 5:
            miss[l] = True
    Ty[miss] = np.nan
    return Ty


def posterior_bank(streams, kern, L):
    """(bank, the definition's tables on the device's own A per latent, the rounding figure per latent)."""
    bank, tbs, _ = bank_of(streams, kern, L, model_tables)
    n = min(L, len(POOL))
    dev = [dict(tbs[l], A=bank.latent(l)["A"]) for l in range(n)]
    for l in range(n):                              # the device's A is the model's (two matrix exponentials, to rounding)
        assert np.max(np.abs(dev[l]["A"] - tbs[l]["A"])) <= FP64_TIGHT * np.max(np.abs(tbs[l]["A"])), l
    figs = [rounding_figure(t) for t in dev]
    return bank, [dev[l % n] for l in range(L)], np.array([figs[l % n] for l in range(L)])


def run_posterior(torch, bank, Ty, tdt, T, **kw):
    out = bank.posterior(to_dev(torch, Ty, tdt, T), want_cov=True, **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.double().cpu().numpy() if k != "status" else v.cpu().numpy()) for k, v in out.items()}


def definition_errors(dtype, Ty, tbs, figs, got):
    """The figures of one call against the definition (evaluated in 80-bit arithmetic): dict(mean, x, nll, var [L], cov [L], bound [L], ref)."""
    ref = {k: np.asarray(v, dtype=np.float64) for k, v in posterior_np(tbs, Ty, np.longdouble).items()}
    ok = ref["status"] == 0
    ev, ep = np.zeros(len(tbs)), np.zeros(len(tbs))
    ev[ok], ep[ok] = entry_err(got["var"][ok], ref["var"][ok]), cov_err(got["P_end"][ok], ref["P_end"][ok])
    return dict(mean=row_err(got["mean"][ok], ref["mean"][ok]), x=row_err(got["x"][ok], ref["x"][ok]), nll=nll_err(got["nll"][ok], ref["nll"][ok]),
                var=ev, cov=ep, bound=np.maximum(10 * figs, ULP_FLOOR), ref=ref, ok=ok)


def assert_matches_definition(dtype, Ty, tbs, figs, got, what=""):
    e = definition_errors(dtype, Ty, tbs, figs, got)
    ref, ok, tol = e["ref"], e["ok"], tol_of(dtype)
    rv, rp = float(np.max(e["var"] / e["bound"])), float(np.max(e["cov"] / e["bound"]))
    print(f"{dtype} L={Ty.shape[0]} T={Ty.shape[1]} {what}: mean {e['mean']:.1e} x {e['x']:.1e} nll {e['nll']:.1e} var {float(np.max(e['var'])):.1e} "
          f"({rv:.2f} of its bound) P_end {rp:.2f} of its bound")
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"])
    assert e["mean"] <= tol and e["x"] <= tol and e["nll"] <= 1e-9, (what, e["mean"], e["x"], e["nll"])
    if dtype == "f64":
        assert rv <= 1.0 and rp <= 1.0, (what, rv, rp)
    else:
        assert float(np.max(e["var"])) <= FP32_TOL and rp <= 1.0, (what, float(np.max(e["var"])), rp)
    for k in ("mean", "var", "x", "P_end", "nll"):
        assert np.all(np.isnan(got[k][~ok])), (what, k)
    return e["mean"], e["x"], e["nll"], rv, rp


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNS)
@pytest.mark.parametrize("L", L_DEVICE)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_posterior_parity(env, kern, L, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    bank, tbs, figs = posterior_bank(streams, kern, L)
    worst = np.zeros(5)
    for T in T_DEVICE:
        Ty = masked_stream(L, T, np.random.default_rng(L * 100003 + T))
        if dtype == "f32":
            Ty = Ty.astype(np.float32).astype(np.float64)
        worst = np.maximum(worst, assert_matches_definition(dtype, Ty, tbs, figs, run_posterior(torch, bank, Ty, tdt, T), f"T {T}"))
    print(f"{kern} {dtype} L={L}: mean {worst[0]:.1e} x {worst[1]:.1e} nll {worst[2]:.1e} var / its bound {worst[3]:.2f} P_end / its bound {worst[4]:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNS)
def test_gap_free_agrees_with_smooth_exact(env, kern):
    """Two independent device routes to the same posterior: the means within FP64_TIGHT, the variances per entry within the larger of FP64_TIGHT
    and ten times the draw's rounding figure (measured 7.1e-14 and 3.0e-11); and smooth() gives the same bits before and after a posterior() on
    the same bank."""
    torch, streams = env["torch"], env["streams"]
    L = 8
    bank, tbs, figs = posterior_bank(streams, kern, L)
    for T in (63, 300, 1025):
        Ty = to_dev(torch, stream_of(L, T, np.random.default_rng(21 + T)), torch.float64, T)
        y0, x0, _ = bank.smooth(Ty)
        y0, x0 = y0.clone(), x0.clone()
        ys, var, x, status = bank.smooth_exact(Ty)
        out = bank.posterior(Ty)
        y1, x1, _ = bank.smooth(Ty)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(x0, x1)
        assert not status.cpu().numpy().any() and not out["status"].cpu().numpy().any()
        em = row_err(out["mean"].cpu().numpy(), ys.cpu().numpy())
        ex = row_err(out["x"].cpu().numpy(), x.cpu().numpy())
        ev = entry_err(out["var"].cpu().numpy(), var.cpu().numpy())
        print(f"{kern} T={T}: mean {em:.1e} x {ex:.1e} var {float(np.max(ev)):.1e}")
        assert em <= FP64_TIGHT and ex <= FP64_TIGHT
        assert np.all(ev <= np.maximum(FP64_TIGHT, 10 * figs)), (T, ev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [17, 300, 1025])
def test_nothing_outside_the_rows(env, dtype, T):
    """Poisoned stream padding and a poisoned row past the last latent, sentinel-filled mean and var slabs of another row stride than the
    stream's: the padding and everything past the last latent stay as they were, and the rows are the definition's."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    L = 7
    for kern in KERNS:
        bank, tbs, figs = posterior_bank(streams, kern, L)
        Ty = masked_stream(L, T, np.random.default_rng(24 + T))
        if dtype == "f32":
            Ty = Ty.astype(np.float32).astype(np.float64)
        dev = to_dev_poison(torch, Ty, tdt, T)
        mslab, mview = sentinel_out(torch, 1, L, T, tdt)
        vslab, vview = sentinel_out(torch, 1, L, T, tdt, pad_row=12)
        with pytest.raises(ValueError):
            bank.posterior(dev, mean=mview[0], var=vview[0])                 # one row stride serves both
        vslab, vview = sentinel_out(torch, 1, L, T, tdt)
        assert mview.stride(1) != dev.stride(0)
        out = bank.posterior(dev, mean=mview[0], var=vview[0], want_cov=True)
        torch.cuda.synchronize()
        assert padding_untouched(torch, mslab, mview) and padding_untouched(torch, vslab, vview)
        got = {k: (v.double().cpu().numpy() if k != "status" else v.cpu().numpy()) for k, v in out.items()}
        assert_matches_definition(dtype, Ty, tbs, figs, got, f"{kern} T {T}")
        assert bool((out["var"] > 0).all())


@pytest.mark.gpu
def test_optional_outputs_do_not_change_the_others(env):
    """Every combination of NULL and non-NULL var, P_end, nll and status through the C entry: what is written holds the bits of the full call."""
    torch, streams = env["torch"], env["streams"]
    L, T = 65, 63
    bank, _, _ = posterior_bank(streams, "Matern52", L)
    lib = bank._lib
    Ty = to_dev(torch, masked_stream(L, T, np.random.default_rng(27)), torch.float64, T)
    ld = Ty.stride(0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    full = None
    for want in itertools.product((True, False), repeat=4):
        mean = torch.full((L, ld), 7.0, dtype=torch.float64, device="cuda")
        var, P_end, nll = torch.full_like(mean, 7.0), torch.full((L, 9), 7.0, dtype=torch.float64, device="cuda"), torch.full((L,), 7.0, dtype=torch.float64, device="cuda")
        status = torch.full((L,), 7, dtype=torch.int32, device="cuda")
        x = torch.zeros((L, 3), dtype=torch.float64, device="cuda")
        bufs = [var, P_end, nll, status]
        a = [b if w else None for b, w in zip(bufs, want)]
        rc = lib.moihgp_posterior_stream(bank._h, 0, p(Ty), T, ld, p(x), p(a[1]), p(mean), p(a[0]), ld, p(a[2]), p(a[3]), None)
        torch.cuda.synchronize()
        assert rc == 0
        if full is None:
            full = [mean, x] + bufs
            assert not bool((status == 7).any()) and not bool((nll == 7.0).any()) and not bool((var[:, :T] == 7.0).any())
            continue
        assert torch.equal(mean, full[0]) and torch.equal(x, full[1]), want
        for b, w, f in zip(bufs, want, full[2:]):
            assert torch.equal(b, f) if w else bool((b == 7).all()), want


@pytest.mark.gpu
def test_scratch_grows_and_is_reused(env):
    """Short, long and short again on one handle (whose L is fixed; a second handle of another L beside it): every call is its definition."""
    torch, streams = env["torch"], env["streams"]
    banks = [posterior_bank(streams, "Matern52", L) for L in (5, 70)]
    for T, which in ((17, 0), (17, 1), (1025, 0), (300, 1), (17, 0), (2, 1), (1025, 1), (33, 0)):
        bank, tbs, figs = banks[which]
        Ty = masked_stream(bank.L, T, np.random.default_rng(31 + T + which))
        assert_matches_definition("f64", Ty, tbs, figs, run_posterior(torch, bank, Ty, torch.float64, T), f"T {T} bank {which}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_infinite_observation_gives_status_5_and_leaves_the_neighbours(env, dtype):
    """One row holds a +Inf tick: that latent's outputs are NaN and its status is 5; the other lanes of its wavefront match the definition."""
    torch, streams = env["torch"], env["streams"]
    L, T, bad = 65, 300, 3
    bank, tbs, figs = posterior_bank(streams, "Matern32", L)
    Ty = masked_stream(L, T, np.random.default_rng(41))
    if dtype == "f32":
        Ty = Ty.astype(np.float32).astype(np.float64)
    Ty[bad, 100] = np.inf
    got = run_posterior(torch, bank, Ty, tdt_of(torch, dtype), T)
    assert got["status"][bad] == 5 and not np.delete(got["status"], bad).any()
    assert_matches_definition(dtype, Ty, tbs, figs, got)


@pytest.mark.gpu
def test_bad_calls_return_the_first_error(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    from multioutputihgp_amd._lib import last_error
    L, T, ld = 4, 64, 64
    bank, _, _ = bank_of(streams, "Matern52", L, model_tables)
    lib = bank._lib
    buf = torch.zeros((3 * L + 1, ld), dtype=torch.float64, device="cuda")
    x = torch.zeros((L, bank.d), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    Ty, mean, var = buf[:L], buf[L:2 * L], buf[2 * L:3 * L]

    def call(h, Ty=Ty, mean=mean, var=var, ld_in=ld, ld_out=ld, x=x, T=T):
        return lib.moihgp_posterior_stream(h, 0, p(Ty), T, ld_in, p(x) if x is not None else None, None, p(mean), p(var) if var is not None else None,
                                           ld_out, None, None, None)

    assert call(bank._h) == 0 and call(bank._h, var=None) == 0
    assert call(bank._h, var=buf[L + 1:2 * L + 1]) == 1 and "var must not overlap mean" in last_error(lib)
    assert call(bank._h, var=Ty) == 1 and "var must not overlap the input stream" in last_error(lib)
    assert call(bank._h, mean=Ty) == 1 and "mean must not overlap the input stream" in last_error(lib)
    assert call(bank._h, ld_out=ld + 1) == 1 and "ld_out" in last_error(lib)
    assert call(bank._h, ld_out=ld - 2) == 1 and "ld_out" in last_error(lib)             # a short ld_out
    assert call(bank._h, ld_in=ld + 1) == 1 and "ld (" in last_error(lib)
    assert call(bank._h, mean=buf[L:2 * L, 1:]) == 1 and "16-byte aligned" in last_error(lib)
    assert call(bank._h, mean=Ty, ld_out=ld + 1) == 1 and "ld_out" in last_error(lib)    # the strides come before the overlaps
    assert call(bank._h, x=None) == 1 and "null" in last_error(lib)
    assert call(None) == 1
    torch.cuda.synchronize()
    stacked = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (L, 1)), kernel="Matern32x2")
    xs = torch.zeros((L, stacked.d), dtype=torch.float64, device="cuda")
    assert call(stacked._h, x=xs) == 3
    assert call(stacked._h, x=xs, var=Ty) == 1                                           # ... and the argument checks before the model's
    with pytest.raises(MoihgpError) as e:
        stacked.posterior(Ty)
    assert e.value.rc == 3


@pytest.mark.gpu
def test_posterior_outputs_end_to_end(env, hip_built):
    """project -> posterior_np -> un-project in numpy against posterior_outputs and against MOIHGPRegression::predictPosterior, with missing
    outputs and one wholly missing tick: var_Y inside the gap exceeds var_Y beside it."""
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(25)
    M, L, T, gap = 5, 3, 63, 30
    ticks = (0, gap - 1, gap, -1)
    params, Y = end_to_end_inputs_small(rng, M, L, T, gap)
    exe = cxx_test_binary(hip_built, "posterior_test")
    for kern in KERNS:
        gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
        gp.update(params)
        U, S, igp, Ty = project_np(gp, Y, nan_below_L=True)
        assert np.isnan(Ty[:, gap]).all() and np.isnan(Ty).sum() == L
        ref = posterior_np([model_tables(kern, 0.1, igp[l]) for l in range(L)], Ty)
        Yref = ((U * np.sqrt(S)) @ ref["mean"]).T
        Vref = np.array([(U ** 2) @ (S * ref["var"][:, t]) for t in ticks])
        Ys, varY, nll = streams.posterior_outputs(gp, torch.from_numpy(Y).cuda(), var_ticks=ticks)
        torch.cuda.synchronize()
        assert Ys.shape == (T, M) and varY.shape == (len(ticks), M) and varY.dtype == np.float64 and nll.shape == (L,)
        scale = float(np.max(np.abs(Yref)))
        assert np.max(np.abs(Ys.cpu().numpy() - Yref)) <= FP64_TIGHT * scale
        assert np.max(np.abs(varY - Vref) / Vref) <= 1e-8
        assert nll_err(nll, ref["nll"]) <= 1e-9
        assert np.all(Vref[2] > Vref[1]) and np.all(varY[2] > varY[1])        # the wholly missing tick is known worse than the observed tick before it
        inp = (f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) +
               f"\n{len(ticks)}\n" + " ".join(str(t) for t in ticks) + "\n")
        lines = cxx_run(exe, inp)
        got, gnll = cxx_rows(lines[:-1]), np.array([float(v) for v in lines[-1].split()])
        assert got.shape == (T + len(ticks), M) and gnll.shape == (L,)
        assert np.max(np.abs(got[:T] - Yref)) <= FP64_TIGHT * scale
        assert np.max(np.abs(got[T:] - Vref) / Vref) <= 1e-8
        assert nll_err(gnll, ref["nll"]) <= 1e-9
    bad = Y.copy()
    bad[5, 0] = np.inf                                                        # an infinite observation reaches every latent it mixes into
    with pytest.raises(MoihgpError, match="non-zero status"):
        streams.posterior_outputs(gp, torch.from_numpy(bad).cuda())


def end_to_end_inputs_small(rng, M, L, T, gap):
    """A full model's parameters and observations [T][M]: a few ticks with one or two outputs missing and tick `gap` missing as a whole."""
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05],
                             np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)]).ravel()])
    Y = np.sin(0.02 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :] % 5)) + 0.1 * rng.standard_normal((T, M))
    for t, ms in ((3, [1]), (17, [0, 4]), (40, [2]), (T - 1, [3, 4])):
        Y[t, ms] = np.nan
    Y[gap, :] = np.nan
    return params, Y
