"""Forecast scores (include/moihgp.h moihgp_forecast_scores): backtest error sums per latent and horizon.  The numpy definition is scores_np below
on top of stream_reference's forecast_np; the CPU tests tie it to the textbook Kalman filter's innovations and to draws from the model's own
prior, the GPU tests hold the library's kernels, Python surface and C entry to it.

Bounds of the GPU tests, from the project's own plane bounds (tau = 1e-9 for fp64 streams, 1e-3 for fp32; sc the latent's h = 0 scale of
forecast_np; fp32 inputs are rounded to fp32 before numpy sees them).  Every scored error e is allowed what test_forecast.py allows a plane
element, tau sc; Cauchy-Schwarz over the n scored origins then gives
    n exact,   |d sum_err| <= n tau sc,   |d sum_sq| <= 2 tau sc sqrt(n sum_sq) + n (tau sc)^2 + 1e-12 sum_sq
the last term for the summation order at n <= 1e4.  Device streams are padded with a finite poison (1e30), not NaN: a read at or past T must
show up as a wrong sum, not hide as an unscored tick.

Calibration figures measured on the CPU while writing this (T 4000, t_first 200, both models, the 8 POOL entries, seeds 100 + index): smse at
h = 1 and h = 5 between 0.934 and 1.035 over all 32 values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rel_err_rows
from parity_support import synth
from stream_reference import forecast_np, forecast_var_np, gain_tables, smooth_np, tables
from stream_support import FP64_TIGHT, HMAX, POOL, env, gaps_ends_run_copy, make_bank, tdt_of, to_dev_poison, tol_of  # noqa: F401  (env: the module's fixture)

HORIZONS = [1, 0, 15, 16, 17, 1023, 1024, HMAX]     # chunk (16) and segment (1024) crossings, h >= T, K = 8


# ------------------------------------------------------------------------------------------------ numpy definition
def scores_np(fc, Ty, horizons, t_first):
    """n, sum_err, sum_sq [K][L] of include/moihgp.h: e = y[t + h] - fc[k][l][t] over the origins t_first <= t < T with t + h < T and y[t + h]
    not NaN."""
    K, L, T = fc.shape
    n = np.zeros((K, L), dtype=np.int64); se = np.zeros((K, L)); sq = np.zeros((K, L))
    for k, h in enumerate(horizons):
        for t in range(t_first, T - h):
            y = Ty[:, t + h]
            ok = ~np.isnan(y)
            with np.errstate(invalid="ignore", over="ignore"):
                e = np.where(ok, y - fc[k, :, t], 0.0)
            n[k] += ok
            se[k] += e
            sq[k] += e * e
    return n, se, sq


def innovations_np(tb, y):
    """v[t] = y[t] - H A xf[t-1] of smooth_np's forward pass (that function keeps v to itself: these are its lines, for one gap-free latent)."""
    A, K = tb["A"], tb["K"]
    x = np.zeros(A.shape[0]); v = np.zeros(len(y))
    for t in range(len(y)):
        xp = A @ x
        v[t] = y[t] - xp[0]
        x = xp + K * v[t]
    return v, x


def prior_draw(tb, T, rng):
    """y[0 .. T) from the model's own prior, the stationary Gaussian process with covariance c[k] = (A^k Pinf)_00 + R delta_k0, drawn through the
    eigendecomposition of the circulant matrix that embeds its T x T Toeplitz covariance (period 2 T; the eigenvectors are the Fourier modes, the
    eigenvalues the transform of its first row).  The embedding is exact where those eigenvalues are non-negative, which is asserted: c has
    decayed to nothing by lag T.  (The state-space model cannot be run forward instead: the Matern-5/2 model's Pinf - A Pinf A^T is indefinite.)"""
    A, Pinf = tb["A"], tb["Pinf"]
    c = np.zeros(T + 1); v = Pinf[:, 0].copy()
    for k in range(T + 1):
        c[k] = v[0]; v = A @ v
    c[0] += tb["R"]
    lam = np.fft.fft(np.concatenate([c, c[-2:0:-1]])).real
    assert lam.min() >= -1e-10 * lam.max(), (lam.min(), lam.max())
    N = len(lam)
    z = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    return np.fft.fft(np.sqrt(np.maximum(lam, 0.0) / N) * z).real[:T]


def summary_of(n, se, sq, pvar, horizons):
    import torch
    from multioutputihgp_amd import streams
    s = streams.score_summary(dict(n=torch.from_numpy(n), sum_err=torch.from_numpy(se), sum_sq=torch.from_numpy(sq),
                                   pvar=None if pvar is None else torch.from_numpy(pvar), horizons=list(horizons)))
    return {k: v.numpy() for k, v in s.items()}


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_forecast_scores():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moihgp.h")).read(), flags=re.S)
    from multioutputihgp_amd import _lib
    assert re.search(r"\bmoihgp_forecast_scores\s*\(", src)
    assert "moihgp_forecast_scores" in _lib.ADDITIVE_SYMBOLS


def test_library_exports_forecast_scores(hip_built):
    assert hasattr(C.CDLL(hip_built), "moihgp_forecast_scores")


def test_python_argument_validation():
    import torch
    from multioutputihgp_amd import streams
    T = 100
    assert streams._first_origin(0, T) == 0 and streams._first_origin(T, T) == T and streams._first_origin(np.int64(7), T) == 7
    for bad in (-1, T + 1, 1.5, True, None, "3"):
        with pytest.raises(ValueError):
            streams._first_origin(bad, T)
    with pytest.raises(ValueError):
        streams._forecast_gains("literal")
    for bad in ([], list(range(9)), [-1], [HMAX + 1], [1.5], [True], 3, None):
        with pytest.raises(ValueError):
            streams._int_list(bad, "horizon", streams.FORECAST_MAX_HORIZONS)
    # the method itself refuses them before anything reaches the library (a CPU tensor is refused first of all)
    bank = streams.LatentBank.__new__(streams.LatentBank)
    bank.L, bank.d, bank.stacked, bank._h, bank._owner = 2, 3, False, None, True
    with pytest.raises(ValueError):
        bank.forecast_scores(torch.zeros((2, T), dtype=torch.float64), [1])
    # score_summary on a hand-made dict: h = 0 and n = 0 give NaN smse / mlpd, the rest is plain arithmetic
    n = np.array([[10, 0], [10, 4]], dtype=np.int64)
    se = np.array([[1.0, 0.0], [-2.0, 0.4]]); sq = np.array([[5.0, 0.0], [20.0, 8.0]]); pvar = np.array([[0.5, 0.5], [2.0, 4.0]])
    s = summary_of(n, se, sq, pvar, [0, 3])
    assert np.isnan(s["smse"][0]).all() and np.isnan(s["mlpd"][0]).all()          # h = 0: in-sample
    assert np.isnan(s["mse"][0, 1]) and np.isnan(s["bias"][0, 1])                  # n = 0
    assert s["mse"][0, 0] == 0.5 and s["bias"][0, 0] == 0.1
    assert np.allclose(s["mse"][1], [2.0, 2.0]) and np.allclose(s["bias"][1], [-0.2, 0.1])
    assert np.allclose(s["smse"][1], [1.0, 0.5])
    assert np.allclose(s["mlpd"][1], [-0.5 * (np.log(2 * np.pi * 2.0) + 1.0), -0.5 * (np.log(2 * np.pi * 4.0) + 0.5)])
    s0 = summary_of(np.array([[0]], dtype=np.int64), np.zeros((1, 1)), np.zeros((1, 1)), np.ones((1, 1)), [2])
    assert np.isnan(s0["smse"]).all() and np.isnan(s0["mlpd"]).all()
    assert set(summary_of(n, se, sq, None, [0, 3])) == {"mse", "bias"}               # gains "handle": no pvar, no smse


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_h1_scores_are_the_kalman_innovations(kern):
    """Gap-free y, zero start, Kalman gains, h = 1, t_first = 0: the scored errors are the filter's innovations v[1 .. T-1], and pvar is their
    steady-state variance S = P_00 + R -- so -n mlpd is the steady-state Kalman negative log likelihood of ticks 1 .. T-1."""
    rng = np.random.default_rng(41)
    T = 700
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    for prm in POOL:
        tb = gain_tables(kern, 0.1, prm, "kalman")
        full = tables(kern, 0.1, prm)
        fc, xe, _ = forecast_np([tb], y[None, :], [1])
        n, se, sq = scores_np(fc, y[None, :], [1], 0)
        v, xv = innovations_np(full, y)
        ys, xs = smooth_np([full], y[None, :])
        assert np.max(np.abs(xv - xs[0])) <= 1e-12 * np.max(np.abs(xs))           # the same forward pass as smooth_np's
        assert n[0, 0] == T - 1
        assert abs(sq[0, 0] - np.sum(v[1:] ** 2)) <= 1e-12 * np.sum(v[1:] ** 2), prm
        assert abs(se[0, 0] - np.sum(v[1:])) <= 1e-12 * np.sum(np.abs(v[1:])), prm
        S = full["P"][0, 0] + full["R"]
        pvar = forecast_var_np(tb, 1) + tb["R"]
        assert abs(pvar - S) <= 1e-12 * S, prm
        s = summary_of(n, se, sq, np.array([[pvar]]), [1])
        nll = 0.5 * np.sum(np.log(2 * np.pi * S) + v[1:] ** 2 / S)
        assert abs(-n[0, 0] * s["mlpd"][0, 0] - nll) <= 1e-12 * abs(nll), prm


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_scores_are_calibrated_on_draws_from_the_prior(kern):
    """y drawn from the model's own prior: sum_sq / (n pvar) is 1 up to sampling error at h = 1 and h = 5.  (h = 50 has too few effective samples
    to assert, h = 0 is in-sample.)"""
    T, t_first, hs = 4000, 200, [1, 5]
    worst = []
    for i, prm in enumerate(POOL):
        tb = gain_tables(kern, 0.1, prm, "kalman")
        y = prior_draw(tb, T, np.random.default_rng(100 + i))
        fc, _, _ = forecast_np([tb], y[None, :], hs)
        n, se, sq = scores_np(fc, y[None, :], hs, t_first)
        pvar = np.array([[forecast_var_np(tb, h) + tb["R"]] for h in hs])
        smse = summary_of(n, se, sq, pvar, hs)["smse"][:, 0]
        print(f"{kern} {prm}: smse h=1 {smse[0]:.3f}, h=5 {smse[1]:.3f}")
        worst.append(np.max(np.abs(smse - 1.0)))
        assert np.all(n[:, 0] == [T - t_first - 1, T - t_first - 5])
    assert max(worst) <= 0.10, worst


# ------------------------------------------------------------------------------------------------ GPU
def round_to(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


def assert_scores(got, ref, scale, tau, what=""):
    """got: the library's dict (or (n, se, sq) arrays); ref: scores_np's triple; the bounds of the module docstring."""
    if isinstance(got, dict):
        got = (got["n"].cpu().numpy(), got["sum_err"].cpu().numpy(), got["sum_sq"].cpu().numpy())
    n, se, sq = ref
    assert np.array_equal(got[0], n), (what, got[0], n)
    b_err = n * tau * scale[None, :]
    b_sq = 2 * tau * scale[None, :] * np.sqrt(n * sq) + n * (tau * scale[None, :]) ** 2 + 1e-12 * sq
    d_err, d_sq = np.abs(got[1] - se), np.abs(got[2] - sq)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what}: sum_err error / bound {np.nanmax(np.where(b_err > 0, d_err / b_err, 0)):.2e}, "
              f"sum_sq error / bound {np.nanmax(np.where(b_sq > 0, d_sq / b_sq, 0)):.2e}")
    assert np.all(d_err <= b_err), (what, float(np.max(d_err - b_err)))
    assert np.all(d_sq <= b_sq), (what, float(np.max(d_sq - b_sq)))


@pytest.mark.gpu
@pytest.mark.parametrize("gains", ["kalman", "handle"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("T", [1, 17, 1023, 1025, 2050])
@pytest.mark.parametrize("L", [1, 9, 70])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scores_parity(env, kern, L, T, dtype, gains):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(L * 100003 + T)
    bank, tbs, _ = make_bank(streams, kern, L, gains)
    x0 = round_to(0.1 * rng.standard_normal((L, bank.d)), dtype)
    x_start = torch.from_numpy(x0).to(tdt).cuda()
    # (a stream of one tick with its tick missing scores nothing: the short streams also run whole)
    for gaps in ((True, False) if T < 63 else (True,)):
        Ty = synth(L, T, rng)
        Ty = round_to(gaps_ends_run_copy(Ty, rng) if gaps else Ty, dtype)
        fc, xref, scale = forecast_np(tbs, Ty, HORIZONS, x0)
        ref = scores_np(fc, Ty, HORIZONS, 0)
        got = bank.forecast_scores(to_dev_poison(torch, Ty, tdt, T), HORIZONS, x_start=x_start, gains=gains)
        torch.cuda.synchronize()
        assert int(got["status"].abs().sum()) == 0
        assert got["horizons"] == HORIZONS and tuple(got["n"].shape) == (8, L) and got["n"].dtype == torch.int64
        assert_scores(got, ref, scale, tol_of(dtype), f"{kern} {gains} {dtype} L={L} T={T} gaps={gaps}")
        assert not ref[0][HORIZONS.index(HMAX)].any() and (T > 1024 or not ref[0][HORIZONS.index(1024)].any())       # h >= T: nothing scored
        assert rel_err_rows(got["x"].double().cpu().numpy(), xref, floor=1e-3) <= tol_of(dtype)
        assert (got["pvar"] is None) == (gains == "handle")
        assert torch.equal(x_start, torch.from_numpy(x0).to(tdt).cuda())


def raw_scores(torch, bank, Ty, T, hs, t_first=0, gains=0, x_in=None, x=None, pad=24, want_err=True, want_pvar=True, n_null=False):
    """The C entry on buffers of the test's own, [K][L] inside slabs filled with sentinels: (rc, n, sum_err, sum_sq, pvar, x, untouched)."""
    K, L = len(hs), bank.L
    p = lambda t: C.c_void_p(t.data_ptr())
    nb = torch.full((K * L + 2 * pad,), 777, dtype=torch.int64, device="cuda")
    db = [torch.full((K * L + 2 * pad,), 12345.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    view = lambda b: b[pad:pad + K * L].view(K, L)
    if x_in is None:
        x_in = torch.zeros((L, bank.d), dtype=Ty.dtype, device="cuda")
    if x is None:
        x = torch.empty_like(x_in)
    hz = (C.c_int * max(K, 1))(*hs) if hs is not None else None
    rc = bank._lib.moihgp_forecast_scores(bank._h, 0 if Ty.dtype == torch.float64 else 1, p(Ty), T, Ty.stride(0), p(x_in), p(x), hz, K, t_first, gains,
                                          None if n_null else p(view(nb)), p(view(db[0])) if want_err else None, p(view(db[1])),
                                          p(view(db[2])) if want_pvar else None, None, None)
    torch.cuda.synchronize()

    def untouched():
        ok = bool((nb[:pad] == 777).all() and (nb[pad + K * L:] == 777).all())
        for b in db:
            ok = ok and bool((b[:pad] == 12345.0).all() and (b[pad + K * L:] == 12345.0).all())
        return ok and (want_err or bool((db[0] == 12345.0).all())) and (want_pvar or bool((db[2] == 12345.0).all()))
    return rc, view(nb).cpu().numpy(), view(db[0]).cpu().numpy(), view(db[1]).cpu().numpy(), view(db[2]).cpu().numpy(), x, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_horizon_groups(env, kern, dtype):
    """K = 1, 2, 3 and 5 at T = 1025: every column of a multi-horizon call is the single-horizon call of that horizon bit for bit (the zero rows
    that pad the last group of the replay stay inside), and nothing outside [K][L] is written."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(51)
    L, T = 9, 1025
    bank, tbs, _ = make_bank(streams, kern, L, "kalman")
    Ty = round_to(gaps_ends_run_copy(synth(L, T, rng), rng), dtype)
    dev = to_dev_poison(torch, Ty, tdt, T)
    hs = [17, 1, 1024, 5, 0]
    single = {}
    for h in hs:
        rc, n, se, sq, pv, _, untouched = raw_scores(torch, bank, dev, T, [h])
        assert rc == 0 and untouched()
        single[h] = (n[0], se[0], sq[0], pv[0])
    fc, _, scale = forecast_np(tbs, Ty, hs)
    assert_scores(tuple(np.stack([single[h][i] for h in hs]) for i in range(3)), scores_np(fc, Ty, hs, 0), scale, tol_of(dtype), f"{kern} {dtype} K=1")
    for K in (2, 3, 5):
        rc, n, se, sq, pv, _, untouched = raw_scores(torch, bank, dev, T, hs[:K])
        assert rc == 0 and untouched(), K
        for k, h in enumerate(hs[:K]):
            for got, one in zip((n[k], se[k], sq[k], pv[k]), single[h]):
                assert np.array_equal(got, one), (K, h)
    # sum_err and pvar are optional: their slabs stay as they were, the others do not change
    rc, n, se, sq, pv, _, untouched = raw_scores(torch, bank, dev, T, hs[:3], want_err=False, want_pvar=False)
    assert rc == 0 and untouched()
    assert all(np.array_equal(n[k], single[h][0]) and np.array_equal(sq[k], single[h][2]) for k, h in enumerate(hs[:3]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_t_first(env, dtype):
    """Origins from t_first on: inside a chunk, on a chunk edge, on a segment edge, the last tick, and T (nothing left to score)."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(52)
    L, T, hs = 9, 2050, [1, 0, 16, 1024]
    bank, tbs, _ = make_bank(streams, "Matern52", L, "kalman")
    Ty = round_to(gaps_ends_run_copy(synth(L, T, rng), rng), dtype)
    dev = to_dev_poison(torch, Ty, tdt, T)
    fc, xref, scale = forecast_np(tbs, Ty, hs)
    for t_first in (0, 5, 16, 1024, T - 1, T):
        got = bank.forecast_scores(dev, hs, t_first=t_first)
        torch.cuda.synchronize()
        assert_scores(got, scores_np(fc, Ty, hs, t_first), scale, tol_of(dtype), f"{dtype} t_first={t_first}")
        assert rel_err_rows(got["x"].double().cpu().numpy(), xref, floor=1e-3) <= tol_of(dtype)       # the state runs over the skipped ticks too
        if t_first == T:
            assert not got["n"].any() and not got["sum_err"].any() and not got["sum_sq"].any()
    for bad in (-1, T + 1, 1.5, True):
        with pytest.raises(ValueError):
            bank.forecast_scores(dev, hs, t_first=bad)
    with pytest.raises(ValueError):
        bank.forecast_scores(dev, hs, gains="literal")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_start_state_and_end_state(env, dtype):
    """A nonzero start state is honoured and left untouched; x may alias it; T = 0 gives zeros and x = x_in."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(53)
    L, T, hs = 9, 1500, [1, 7]
    bank, tbs, _ = make_bank(streams, "Matern32", L, "kalman")
    Ty = round_to(synth(L, T, rng), dtype)
    x0 = round_to(rng.standard_normal((L, bank.d)), dtype)
    dev = to_dev_poison(torch, Ty, tdt, T)
    fc, xref, scale = forecast_np(tbs, Ty, hs, x0)
    ref = scores_np(fc, Ty, hs, 0)
    fc0, _, _ = forecast_np(tbs, Ty, hs)
    assert np.max(np.abs(scores_np(fc0, Ty, hs, 0)[2] - ref[2]) / ref[2]) > 1e-2              # (the start state does matter here)
    x_start = torch.from_numpy(x0).to(tdt).cuda()
    a = bank.forecast_scores(dev, hs, x_start=x_start)
    alias = x_start.clone()
    b = bank.forecast_scores(dev, hs, x=alias)                                                # x_in == x
    torch.cuda.synchronize()
    assert torch.equal(x_start, torch.from_numpy(x0).to(tdt).cuda())
    assert_scores(a, ref, scale, tol_of(dtype), f"{dtype} x_start")
    assert rel_err_rows(a["x"].double().cpu().numpy(), xref, floor=1e-3) <= tol_of(dtype)
    assert b["x"] is alias
    for k in ("n", "sum_err", "sum_sq", "pvar", "x"):
        assert torch.equal(a[k], b[k]), k
    z = bank.forecast_scores(dev, hs, T=0, x_start=x_start)
    torch.cuda.synchronize()
    assert not z["n"].any() and not z["sum_err"].any() and not z["sum_sq"].any() and torch.equal(z["x"], x_start)
    assert torch.equal(z["pvar"], a["pvar"]) and not z["status"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("gains", ["kalman", "handle"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scan_and_serial_paths_agree(env, kern, dtype, gains):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(54)
    L, T, hs = 9, 2050, [0, 1, 7, 300, 1024]
    bank, tbs, _ = make_bank(streams, kern, L, gains)
    Ty = round_to(gaps_ends_run_copy(synth(L, T, rng), rng), dtype)
    dev = to_dev_poison(torch, Ty, tdt, T)
    fc, xref, scale = forecast_np(tbs, Ty, hs)
    ref = scores_np(fc, Ty, hs, 3)
    for path in (0, 1):
        bank.set_option("forecast_path", path)
        got = bank.forecast_scores(dev, hs, t_first=3, gains=gains)
        torch.cuda.synchronize()
        assert_scores(got, ref, scale, tol_of(dtype), f"{kern} {gains} {dtype} path {path}")
        assert rel_err_rows(got["x"].double().cpu().numpy(), xref, floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
def test_growth_bound_fallback(env):
    """The bank of test_forecast.py::test_growth_bound_fallback_kalman: automatic routing sends its bad latents (every fourth) to the serial walk,
    whose columns are then the path-1 call's bit for bit; numpy runs on the device's own tables, as that test does."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(26)
    pool = [(1.0, 0.01, 0.01), (1.0, 1.0, 0.1), (0.7, 0.5, 0.05), (1.0, 0.03, 1e-4)]
    L, T, hs = 8, 3000, [0, 1, 7, 300]
    bank, _, _ = make_bank(streams, "Matern52", L, "kalman", dt=0.01, pool=pool)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev_poison(torch, Ty, torch.float64, T)
    res = {}
    for path in (-1, 1, 0):
        bank.set_option("forecast_path", path)
        res[path] = bank.forecast_scores(dev, hs)
        torch.cuda.synchronize()
        assert not res[path]["status"].any()
    dtb = []
    for l in range(L):
        A, K = bank.latent(l)["A"], bank.smoother(l)["K"]
        dtb.append(dict(A=A, K=K, M=A - np.outer(K, A[0])))
    fc, xref, scale = forecast_np(dtb, Ty, hs)
    assert_scores(res[-1], scores_np(fc, Ty, hs, 0), scale, FP64_TIGHT, "growth bound, automatic")
    for k in ("n", "sum_err", "sum_sq"):
        assert torch.equal(res[-1][k][:, 0::4], res[1][k][:, 0::4]), k
    assert torch.equal(res[-1]["x"][0::4], res[1]["x"][0::4])
    others = [l for l in range(L) if l % 4]
    assert torch.equal(res[-1]["sum_sq"][:, others], res[0]["sum_sq"][:, others])       # the rest took the scan


@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
def test_failed_latent(env, path):
    """A latent whose Kalman DARE cannot converge (NaN magnitude, as test_forecast.py's): status 1, n = 0, NaN sums, NaN pvar, NaN end state;
    the neighbours stay within bounds.  With the handle's gains there is no such DARE: status is all zero."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(55)
    L, T, bad, hs = 7, 2050, 3, [0, 1, 7, 300]
    bank, tbs, prm = make_bank(streams, "Matern52", L, "kalman")
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("forecast_path", path)
    Ty = synth(L, T, rng)
    dev = to_dev_poison(torch, Ty, torch.float64, T)
    got = bank.forecast_scores(dev, hs)
    torch.cuda.synchronize()
    st = got["status"].cpu().numpy()
    keep = [l for l in range(L) if l != bad]
    assert st[bad] == 1 and not st[keep].any()
    assert not got["n"][:, bad].any()
    for k in ("sum_err", "sum_sq", "pvar"):
        assert bool(torch.isnan(got[k][:, bad]).all()), k
        assert bool(torch.isfinite(got[k][:, keep]).all()), k
    assert bool(torch.isnan(got["x"][bad]).all())
    fc, xref, scale = forecast_np([tbs[l] for l in keep], Ty[keep], hs)
    near = tuple(got[k][:, keep].cpu().numpy() for k in ("n", "sum_err", "sum_sq"))
    assert_scores(near, scores_np(fc, Ty[keep], hs, 0), scale, FP64_TIGHT, f"failed latent, path {path}")
    assert rel_err_rows(got["x"][keep].cpu().numpy(), xref, floor=1e-3) <= FP64_TIGHT
    h = bank.forecast_scores(dev, hs, gains="handle")
    torch.cuda.synchronize()
    assert not h["status"].any() and h["pvar"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_pvar_is_the_forecast_variance_plus_noise(env, kern):
    torch, streams = env["torch"], env["streams"]
    hs = [0, 1, 5, 50, 300, HMAX]
    L, T = 16, 64
    bank, tbs, prm = make_bank(streams, kern, L, "kalman")
    dev = to_dev_poison(torch, synth(L, T, np.random.default_rng(56)), torch.float64, T)
    pvar = bank.forecast_scores(dev, hs)["pvar"].cpu().numpy()
    ref = bank.forecast_variances(hs) + prm[None, :, 2]
    assert np.max(np.abs(pvar - ref) / ref) <= 1e-10
    for l in range(L):      # h = 1: S = P_00 + R of the smoother's tables
        S = tables(kern, 0.1, tuple(prm[l]))["S"]
        assert abs(pvar[1, l] - S) <= 1e-9 * S
    rc, *_ = raw_scores(torch, bank, dev, T, hs, gains=1, want_pvar=True)
    assert rc == 1                                                   # the variances belong to the Kalman gains
    rc, n, se, sq, pv, _, untouched = raw_scores(torch, bank, dev, T, hs, gains=1, want_pvar=False)
    assert rc == 0 and untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_calls_give_the_same_bits(env, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    rng = np.random.default_rng(57)
    L, T = 70, 2050
    bank, _, _ = make_bank(streams, "Matern52", L, "kalman")
    dev = to_dev_poison(torch, gaps_ends_run_copy(synth(L, T, rng), rng), tdt, T)
    a = bank.forecast_scores(dev, HORIZONS, t_first=9)
    b = bank.forecast_scores(dev, HORIZONS, t_first=9)
    torch.cuda.synchronize()
    for k in ("n", "sum_err", "sum_sq"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_return_codes(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    L, T = 4, 64
    bank, _, _ = make_bank(streams, "Matern52", L, "kalman")
    dev = to_dev_poison(torch, synth(L, T, np.random.default_rng(58)), torch.float64, T)
    rc, *_, untouched = raw_scores(torch, bank, dev, T, [1, 5])
    assert rc == 0 and untouched()
    for kw in (dict(hs=[1, 5], t_first=T + 1), dict(hs=[]), dict(hs=list(range(9))), dict(hs=[1, -1]), dict(hs=[1, HMAX + 1]), dict(hs=[1, 5], gains=2),
               dict(hs=[1, 5], n_null=True)):
        hs = kw.pop("hs")
        rc, n, se, sq, pv, _, untouched = raw_scores(torch, bank, dev, T, hs, **kw)
        assert rc == 1, (hs, kw)
        assert untouched() and (n == 777).all() and (se == 12345.0).all() and (sq == 12345.0).all() and (pv == 12345.0).all()      # nothing launched
    stacked = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (L, 1)), kernel="Matern32x2")
    for gains in (0, 1):
        rc, *_ = raw_scores(torch, stacked, dev, T, [1], gains=gains, want_pvar=gains == 0)
        assert rc == 3
    with pytest.raises(MoihgpError):
        stacked.forecast_scores(dev, [1])


@pytest.mark.gpu
def test_score_outputs_is_the_scores_of_the_projected_streams(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(59)
    M, L, T, hs = 6, 3, 300, [1, 0, 12]
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05],
                              np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)]).ravel()]))
    Y = np.sin(0.1 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :])) + 0.1 * rng.standard_normal((T, M))
    Y[[3, 50, 51, 299], [0, 2, 2, 5]] = np.nan
    Y[100] = np.nan                                                  # a tick missing as a whole: no target
    Yd = torch.from_numpy(Y).cuda()
    for gains in ("kalman", "handle"):
        a = streams.score_outputs(gp, Yd, hs, t_first=20, gains=gains)
        b = streams.LatentBank.from_handle(gp).forecast_scores(streams.project_stream(gp, Yd), hs, T=T, t_first=20, gains=gains)
        torch.cuda.synchronize()
        for k in ("n", "sum_err", "sum_sq", "x", "status"):
            assert torch.equal(a[k], b[k]), k
        assert (a["pvar"] is None and b["pvar"] is None) if gains == "handle" else torch.equal(a["pvar"], b["pvar"])
        assert a["horizons"] == hs and int(a["n"][0].max()) <= T - 20 - 1 - 1                      # tick 100 is no target
        s = streams.score_summary(a)
        assert tuple(s["mse"].shape) == (3, L) and (("smse" in s) == (gains == "kalman"))
        if gains == "kalman":
            assert bool(torch.isnan(s["smse"][1]).all()) and bool(torch.isfinite(s["smse"][[0, 2]]).all())
