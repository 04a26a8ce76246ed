"""Multi-horizon forecasts (include/moihgp.h moihgp_forecast_stream / _tail / _variances): the numpy definition the GPU is held to, checked
against the dense GP predictive distribution (Kalman-form gains) and a literal loop of the reference's step / prediction-only step (the handle's
gains) on the CPU, then the library's kernels, Python and C++ surfaces against it on the GPU.

Measured on the CPU while writing this (both models, the smoother's 8-entry POOL, dt 0.1, T 600, forecast at tick 400, horizons 0, 1, 5, 50):
Kalman-gain mean vs dense GP <= 7.4e-13 absolute, variance <= 4.4e-10 relative; the bounds below leave room for other seeds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import rel_err, rel_err_rows
from oracle.moihgp_numpy import IHGP
from parity_support import synth
from stream_reference import forecast_np, forecast_var_np, gain_tables, tables
from stream_support import (CASES, FP32_TOL, FP64_TIGHT, HMAX, KMAP, POOL, assert_declared, assert_exported, cxx_fmt, cxx_rows, cxx_run,
                            cxx_test_binary, end_to_end_inputs, env, make_bank, padding_untouched, plane_err, sentinel_out, to_dev,
                            tol_of)  # noqa: F401  (env: the module's fixture)

FORECAST_SYMBOLS = ("moihgp_forecast_stream", "moihgp_forecast_tail", "moihgp_forecast_variances")
HORIZONS = [1, 0, 7, 7, 300, HMAX]      # unsorted, repeated, extreme


# ------------------------------------------------------------------------------------------------ cross-check of the numpy definition
def dense_predictive(tb, y, t0, h):
    """Mean and variance of the latent function at tick t0 + h given y[0..t0] under the stationary GP prior with covariance (A^k Pinf)_00."""
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    n = t0 + h + 1
    c = np.zeros(n); Mk = np.eye(A.shape[0])
    for k in range(n):
        c[k] = (Mk @ Pinf)[0, 0]; Mk = A @ Mk
    i = np.arange(t0 + 1)
    Kd = c[np.abs(i[:, None] - i[None, :])] + R * np.eye(t0 + 1)
    ks = c[np.abs(t0 + h - i)]
    return ks @ np.linalg.solve(Kd, y[:t0 + 1]), c[0] - ks @ np.linalg.solve(Kd, ks)


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_forecast_entries():
    src = assert_declared(FORECAST_SYMBOLS)
    assert re.search(r"#define\s+MOIHGP_FORECAST_MAX_HORIZONS\s+8\b", src)


def test_library_exports_the_forecast_entries(hip_built):
    assert_exported(hip_built, FORECAST_SYMBOLS)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_kalman_forecast_is_the_gp_predictive(kern):
    rng = np.random.default_rng(21)
    T, t0 = 600, 400
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    worst_m, worst_v = 0.0, 0.0
    for prm in POOL:
        tb = gain_tables(kern, 0.1, prm, "kalman")
        hs = [0, 1, 5, 50]
        fc, _, _ = forecast_np([tb], y[None, :], hs)
        for k, h in enumerate(hs):
            mean, var = dense_predictive(tb, y, t0, h)
            worst_m = max(worst_m, abs(fc[k, 0, t0] - mean))
            worst_v = max(worst_v, abs(forecast_var_np(tb, h) - var) / var)
    print(f"{kern}: mean vs dense GP {worst_m:.2e} (abs), variance {worst_v:.2e} (rel)")
    assert worst_m <= 1e-10, worst_m
    assert worst_v <= 1e-8, worst_v


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_handle_forecast_is_the_reference_step_loop(kern):
    """gains "handle": the reference's step(x, y), then h prediction-only step(x) calls, per tick and per horizon (ihgp.h:81-100)."""
    rng = np.random.default_rng(22)
    T, hs = 120, [0, 1, 5, 50]
    y = np.sin(0.05 * np.arange(T)) + 0.1 * rng.standard_normal(T)
    y[[0, 40, 41, 119]] = np.nan
    worst = 0.0
    for prm in POOL:
        g = IHGP(0.1, kern)
        g.update(np.asarray(prm, dtype=np.float64))
        fc, xe, scale = forecast_np([gain_tables(kern, 0.1, prm, "handle")], y[None, :], hs)
        x = np.zeros(g.dim)
        for t in range(T):
            x, yhat = g.step(x, y[t])
            for k, h in enumerate(hs):
                xx, f = x, yhat
                for _ in range(h):
                    xx, f = g.step(xx)
                worst = max(worst, abs(fc[k, 0, t] - f) / scale[0])
        assert np.max(np.abs(xe[0] - x)) <= 1e-12 * max(1.0, np.max(np.abs(x)))
    print(f"{kern}: handle gains vs step loop {worst:.2e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_variance_starts_at_var_filtered_and_rises_to_the_prior(kern):
    for prm in POOL:
        tb = gain_tables(kern, 0.1, prm, "kalman")
        p00 = tb["Pinf"][0, 0]
        v = np.array([forecast_var_np(tb, h) for h in range(400)])
        assert abs(v[0] - tables(kern, 0.1, prm)["var_f"]) <= 1e-12 * p00
        assert np.all(np.diff(v) >= -1e-15 * p00), (prm, float(np.min(np.diff(v))) / p00)
        assert abs(forecast_var_np(tb, HMAX) - p00) <= 1e-15 * p00


def test_python_argument_validation():
    import torch
    from multioutputihgp_amd import streams
    hz, K = streams._int_list(HORIZONS, "horizon", streams.FORECAST_MAX_HORIZONS)
    assert K == 6 and list(hz) == HORIZONS
    for bad in ([], list(range(9)), [-1], [HMAX + 1], [1.5], [True], 3, None):
        with pytest.raises(ValueError):
            streams._int_list(bad, "horizon", streams.FORECAST_MAX_HORIZONS)
    with pytest.raises(ValueError):
        streams._forecast_gains("literal")
    assert streams._forecast_gains("kalman") == 0 and streams._forecast_gains("handle") == 1
    L, T = 4, 100
    slab = torch.zeros(8 * L * 112, dtype=torch.float64)
    Ty = slab[:L * 104].view(L, 104)[:, :T]
    good = torch.as_strided(slab, (2, L, T), (L * 108 + 4, 108, 1), L * 104)
    assert streams._plane_out_strides(good, 2, L, T, Ty) == (108, L * 108 + 4)
    bads = [torch.as_strided(slab, (2, L, T), (L * 108 + 4, 108, 1), 8),             # overlaps Ty
            torch.as_strided(slab, (2, L, T), (L * 108 + 4, 107, 1), L * 104),       # row stride not a multiple of 16 bytes
            torch.as_strided(slab, (2, L, T), (L * 108 + 1, 108, 1), L * 104),       # plane stride not a multiple of 16 bytes
            torch.as_strided(slab, (2, L, T), (3 * 108, 108, 1), L * 104),           # planes overlap: plane stride < L rows
            torch.as_strided(slab, (2, L, T), (L * 98, 98, 1), L * 104),             # rows shorter than T rounded up
            torch.as_strided(slab, (2, L, T), (L * 216, 216, 2), L * 104),           # not unit stride along time
            torch.as_strided(slab, (2, L, T), (L * 108, 108, 1), L * 104 + 1),       # base not 16-byte aligned
            torch.as_strided(slab, (3, L, T), (L * 108, 108, 1), L * 104),           # K planes expected, 3 given
            torch.as_strided(slab, (2, L, T - 1), (L * 108, 108, 1), L * 104),       # shorter than T
            torch.zeros((2, L, 108), dtype=torch.float32)[:, :, :T]]                 # dtype
    for b in bads:
        with pytest.raises(ValueError):
            streams._plane_out_strides(b, 2, L, T, Ty)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gains", ["kalman", "handle"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("L,T", CASES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forecast_parity(env, kern, L, T, dtype, gains):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(L * 100003 + T)
    bank, tbs, _ = make_bank(streams, kern, L, gains)
    Ty = synth(L, T, rng)
    if T >= 63:   # missing ticks at the two ends, a long run, and 1 % scattered (as test_smooth_parity)
        Ty[:, 0] = np.nan; Ty[:, T - 1] = np.nan
        Ty[::3, T // 3:T // 3 + min(300, T // 4)] = np.nan
        Ty[rng.random((L, T)) < 0.01] = np.nan
    if tdt == torch.float32:
        Ty = Ty.astype(np.float32).astype(np.float64)
    x0 = 0.1 * rng.standard_normal((L, bank.d))
    if tdt == torch.float32:
        x0 = x0.astype(np.float32).astype(np.float64)
    ref, xref, scale = forecast_np(tbs, Ty, HORIZONS, x0)
    x_start = torch.from_numpy(x0).to(tdt).cuda()
    x = torch.empty_like(x_start)
    slab, out = sentinel_out(torch, len(HORIZONS), L, T, tdt)     # ld_out != ld_in, plane_stride > L * ld_out
    fc, x, status = bank.forecast(to_dev(torch, Ty, tdt, T), HORIZONS, x=x, x_start=x_start, out=out, gains=gains)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    got = fc.double().cpu().numpy()
    errs = [plane_err(got[k], ref[k], scale) for k in range(len(HORIZONS))]
    ex = rel_err_rows(x.double().cpu().numpy(), xref, floor=1e-3)
    print(f"{kern} {gains} {dtype} L={L} T={T}: plane errors {['%.1e' % e for e in errs]}, end state {ex:.1e}")
    assert max(errs) <= tol_of(dtype), errs
    assert ex <= tol_of(dtype), ex
    assert padding_untouched(torch, slab, out)
    assert np.max(np.abs(got[HORIZONS.index(HMAX)])) <= 1e-30     # A^(2^20) has underflowed: the plane is all but zero


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_handle_gains_h0_is_the_filter(env, kern, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(23)
    L, T = 64, 3000
    bank, _, _ = make_bank(streams, kern, L, "handle")
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, tdt, T)
    yhat, xf, _ = bank.filter(dev, T=T)
    fc, x, status = bank.forecast(dev, [0], gains="handle")
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert rel_err_rows(fc[0].double().cpu().numpy(), yhat[:, :T].double().cpu().numpy()) <= tol_of(dtype)
    assert rel_err_rows(x.double().cpu().numpy(), xf.double().cpu().numpy(), floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_forecast_outputs_handle_gains_is_the_per_tick_abi(env, kern):
    """A tiny full object: forecast_outputs(gains="handle") against step(x, y) followed by h prediction-only step(x) calls through the
    reference's per-tick ABI."""
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(24)
    M, L, T, hs = 4, 2, 50, [0, 1, 3, 12]
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05],
                              np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)]).ravel()]))
    Y = np.sin(0.1 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :])) + 0.1 * rng.standard_normal((T, M))
    Yf, var, Ytail = streams.forecast_outputs(gp, torch.from_numpy(Y).cuda(), hs, tail=5, gains="handle")
    torch.cuda.synchronize()
    Yf, Ytail = Yf.cpu().numpy(), Ytail.cpu().numpy()
    assert Yf.shape == (len(hs), T, M) and var.shape == (len(hs), M) and Ytail.shape == (5, M)
    ref = np.zeros_like(Yf)
    x = np.zeros((L, gp.igp_dim))
    for t in range(T):
        x, yhat = gp.step(x, Y[t])
        for k, h in enumerate(hs):
            xx, f = x, yhat
            for _ in range(h):
                xx, f = gp.step(xx)
            ref[k, t] = np.ravel(f)
    assert rel_err(Yf, ref) <= FP64_TIGHT, rel_err(Yf, ref)
    tail_ref, xx = np.zeros((5, M)), x
    for j in range(5):
        xx, f = gp.step(xx)
        tail_ref[j] = np.ravel(f)
    assert rel_err(Ytail, tail_ref) <= FP64_TIGHT


@pytest.mark.gpu
@pytest.mark.parametrize("gains", ["kalman", "handle"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scan_and_serial_paths_agree(env, kern, dtype, gains):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(25)
    L, T, hs = 64, 5000, [0, 1, 7, 300, 40]
    bank, tbs, _ = make_bank(streams, kern, L, gains)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    if tdt == torch.float32:
        Ty = Ty.astype(np.float32).astype(np.float64)
    dev = to_dev(torch, Ty, tdt, T)
    ref, xref, scale = forecast_np(tbs, Ty, hs)
    res = {}
    for path in (0, 1):
        bank.set_option("forecast_path", path)
        fc, x, _ = bank.forecast(dev, hs, gains=gains)
        torch.cuda.synchronize()
        res[path] = (fc.double().cpu().numpy(), x.double().cpu().numpy())
    for k in range(len(hs)):
        assert plane_err(res[0][0][k], res[1][0][k], scale) <= tol_of(dtype)
        assert plane_err(res[1][0][k], ref[k], scale) <= tol_of(dtype)
        assert plane_err(res[0][0][k], ref[k], scale) <= tol_of(dtype)
    assert rel_err_rows(res[0][1], res[1][1], floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
def test_growth_bound_fallback_kalman(env):
    """The bank of test_smoother.py::test_growth_bound_fallback (Matern-5/2, dt 0.01, lengthscale 0.01: powers of A - K H A reach ~4e4): the
    automatic path walks that latent serially; numpy runs on the device's own tables, as that test does and for its reason."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(26)
    pool = [(1.0, 0.01, 0.01), (1.0, 1.0, 0.1), (0.7, 0.5, 0.05), (1.0, 0.03, 1e-4)]
    L, T, hs = 8, 3000, [0, 1, 7, 300]
    bank, tbs, _ = make_bank(streams, "Matern52", L, "kalman", dt=0.01, pool=pool)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, torch.float64, T)
    bank.set_option("forecast_path", -1)
    fa, xa, sa = bank.forecast(dev, hs)
    fa = fa.clone(); xa = xa.clone()
    bank.set_option("forecast_path", 1)
    fs, xs, _ = bank.forecast(dev, hs)
    torch.cuda.synchronize()
    assert not sa.cpu().numpy().any()
    dtb = []
    for l in range(L):
        A, K = bank.latent(l)["A"], bank.smoother(l)["K"]
        dtb.append(dict(A=A, K=K, M=A - np.outer(K, A[0])))
    ref, xref, scale = forecast_np(dtb, Ty, hs)
    fa, fs = fa.cpu().numpy(), fs.cpu().numpy()
    for k in range(len(hs)):
        assert plane_err(fa[k], ref[k], scale) <= 1e-9, (k, plane_err(fa[k], ref[k], scale))
    assert np.array_equal(fa[:, 0::4], fs[:, 0::4])                  # the fallback latents: the serial walk itself
    assert np.array_equal(xa.cpu().numpy()[0::4], xs.cpu().numpy()[0::4])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,T", [("f64", 200), ("f32", 150)])
def test_unstable_handle_latents_take_the_serial_path(env, dtype, T):
    """The Matern-3/2 draws of test_gpu_parity.py::test_unstable_latents_take_the_sequential_path (rho(AKHA) = 1.47, 1.17, 1.37 with the literal
    DARE, dt 0.1) among tame latents: every row matches numpy while finite; tolerances as that test (1e-9 fp64, 2e-3 fp32)."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    pool = [(99.2440457, 4.06889466, 2.55306111e-03), (1.0, 1.0, 0.1), (0.927049235, 1.63239037, 4.34082530e-04),
            (66.2316497, 5.1761023, 1.51666229e-03), (0.5, 0.6, 0.02), (2.0, 1.7, 0.3)]
    L, hs = 12, [0, 1, 7]
    bank, tbs, _ = make_bank(streams, "Matern32", L, "handle", pool=pool)
    assert max(abs(np.linalg.eigvals(tbs[0]["M"]))) > 1.4
    rng = np.random.default_rng(27)
    Ty = synth(L, T, rng)
    if tdt == torch.float32:
        Ty = Ty.astype(np.float32).astype(np.float64)
    ref, xref, scale = forecast_np(tbs, Ty, hs)
    fc, x, status = bank.forecast(to_dev(torch, Ty, tdt, T), hs, gains="handle")
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    got = fc.double().cpu().numpy()
    tol = 1e-9 if dtype == "f64" else 2e-3
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    low = np.abs(ref) < 1e30 if dtype == "f32" else np.ones(ref.shape, dtype=bool)      # fp32 rows are compared only while below 1e30
    assert low[:, :, :100].all()
    for l in range(L):          # per latent: magnitudes differ by tens of orders
        for k in range(len(hs)):
            m = low[k, l]
            assert rel_err(got[k, l][m], ref[k, l][m]) <= tol, (l, k, rel_err(got[k, l][m], ref[k, l][m]))     # (each row against its own size, as that test)
        assert np.max(np.abs(x.double().cpu().numpy()[l] - xref[l])) <= tol * max(np.max(np.abs(xref[l])), 1e-3), l


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_variances_match_numpy(env, kern):
    streams = env["streams"]
    hs = [0, 1, 5, 50, 300, HMAX]
    bank, tbs, _ = make_bank(streams, kern, 16, "kalman")
    var = bank.forecast_variances(hs)
    assert var.shape == (len(hs), 16)
    vf, _ = bank.latent_variances()
    for l in range(16):
        for k, h in enumerate(hs):
            ref = forecast_var_np(tbs[l], h)
            assert abs(var[k, l] - ref) <= 1e-10 * ref, (l, h, var[k, l], ref)
        assert abs(var[0, l] - vf[l]) <= 1e-10 * vf[l]
        assert np.all(np.diff(var[:, l]) >= -1e-15 * tbs[l]["Pinf"][0, 0])
        assert abs(var[-1, l] - tbs[l]["Pinf"][0, 0]) <= 1e-12 * tbs[l]["Pinf"][0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
def test_failed_latent_kalman_gains(env, path):
    """A latent whose Kalman DARE cannot converge (NaN magnitude, as test_smoother.py's): status 1, NaN rows in every plane, NaN end state and
    NaN variances; the other latents are untouched."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(28)
    L, T, bad, hs = 7, 2500, 3, [0, 1, 7, 300]
    bank, tbs, prm = make_bank(streams, "Matern52", L, "kalman")
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("forecast_path", path)
    Ty = synth(L, T, rng)
    fc, x, status = bank.forecast(to_dev(torch, Ty, torch.float64, T), hs)
    torch.cuda.synchronize()
    st, got, xg = status.cpu().numpy(), fc.cpu().numpy(), x.cpu().numpy()
    assert st[bad] == 1 and np.all(np.isnan(got[:, bad])) and np.all(np.isnan(xg[bad]))
    keep = [l for l in range(L) if l != bad]
    assert not st[keep].any()
    ref, xref, scale = forecast_np([tbs[l] for l in keep], Ty[keep], hs)
    for k in range(len(hs)):
        assert plane_err(got[k][keep], ref[k], scale) <= FP64_TIGHT
    assert rel_err_rows(xg[keep], xref, floor=1e-3) <= FP64_TIGHT
    var = bank.forecast_variances(hs)
    assert np.all(np.isnan(var[:, bad])) and np.all(np.isfinite(var[:, keep]))


@pytest.mark.gpu
def test_failed_latent_handle_gains(env):
    """The same bank under gains "handle": that mode has no DARE of its own to fail, so status is 0 everywhere; the bad latent's rows are what the
    handle's filter gives there, the neighbours are exact."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(29)
    L, T, bad, hs = 7, 2500, 3, [0, 1, 7, 300]
    bank, tbs, prm = make_bank(streams, "Matern52", L, "handle")
    prm[bad, 0] = np.nan
    bank.update(prm)
    Ty = synth(L, T, rng)
    dev = to_dev(torch, Ty, torch.float64, T)
    fc, x, status = bank.forecast(dev, hs, gains="handle")
    yhat, _, _ = bank.filter(dev, T=T)
    torch.cuda.synchronize()
    got = fc.cpu().numpy()
    assert not status.cpu().numpy().any()
    assert np.array_equal(np.isnan(got[0, bad]), np.isnan(yhat[bad, :T].cpu().numpy()))
    assert np.all(np.isnan(got[0, bad]))
    keep = [l for l in range(L) if l != bad]
    ref, xref, scale = forecast_np([tbs[l] for l in keep], Ty[keep], hs)
    for k in range(len(hs)):
        assert plane_err(got[k][keep], ref[k], scale) <= FP64_TIGHT
    assert rel_err_rows(x.cpu().numpy()[keep], xref, floor=1e-3) <= FP64_TIGHT


@pytest.mark.gpu
def test_forecast_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(30)
    M, L, T = 8, 3, 100
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.forecast_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda(), [1, 5])


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tail(env, kern, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(31)
    L = 19
    bank, tbs, _ = make_bank(streams, kern, L, "kalman")
    x0 = rng.standard_normal((L, bank.d))
    if tdt == torch.float32:
        x0 = x0.astype(np.float32).astype(np.float64)
    xd = torch.from_numpy(x0).to(tdt).cuda()
    for n in (1, 17, 4096):
        tail = bank.forecast_tail(xd, n)
        torch.cuda.synchronize()
        assert tuple(tail.shape) == (L, n)
        ref = np.zeros((L, n))
        for l in range(L):
            v = x0[l].copy()
            for j in range(n):
                v = tbs[l]["A"] @ v
                ref[l, j] = v[0]
        scale = np.maximum(np.max(np.abs(ref), axis=1), np.abs(x0[:, 0]))
        assert plane_err(tail.double().cpu().numpy(), ref, scale) <= tol_of(dtype), n
    # consistency: the forecasts made at the last tick with horizons 1 .. 8 are the first 8 tail values from the returned end state
    T = 777
    Ty = synth(L, T, rng)
    if tdt == torch.float32:
        Ty = Ty.astype(np.float32).astype(np.float64)
    fc, x, _ = bank.forecast(to_dev(torch, Ty, tdt, T), list(range(1, 9)))
    tail = bank.forecast_tail(x, 8)
    torch.cuda.synchronize()
    _, _, scale = forecast_np(tbs, Ty, [0])
    assert plane_err(fc[:, :, T - 1].T.double().cpu().numpy(), tail.double().cpu().numpy(), scale) <= tol_of(dtype)


@pytest.mark.gpu
def test_forecast_after_update_uses_the_new_parameters(env):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(32)
    L, T, hs = 7, 1000, [0, 3, 40]
    Ty = synth(L, T, rng)
    for gains in ("kalman", "handle"):
        bank, tbs, prm = make_bank(streams, "Matern52", L, gains)
        f1, _, _ = bank.forecast(to_dev(torch, Ty, torch.float64, T), hs, gains=gains)
        torch.cuda.synchronize()
        ref, _, scale = forecast_np(tbs, Ty, hs)
        assert max(plane_err(f1.cpu().numpy()[k], ref[k], scale) for k in range(3)) <= FP64_TIGHT
        v1 = bank.forecast_variances(hs)
        pool2 = [(p[0] * 1.5, p[1] * 0.7, p[2] * 2.0) for p in POOL]
        bank.update(np.array([pool2[l % len(pool2)] for l in range(L)]))
        f2, _, _ = bank.forecast(to_dev(torch, Ty, torch.float64, T), hs, gains=gains)
        torch.cuda.synchronize()
        tbs2 = [gain_tables("Matern52", 0.1, pool2[l % len(pool2)], gains) for l in range(L)]
        ref2, _, scale2 = forecast_np(tbs2, Ty, hs)
        assert max(plane_err(f2.cpu().numpy()[k], ref2[k], scale2) for k in range(3)) <= FP64_TIGHT
        assert max(plane_err(f2.cpu().numpy()[k], ref[k], scale) for k in range(3)) > 1e-3          # (and they do differ)
        v2 = bank.forecast_variances(hs)
        kt = [gain_tables("Matern52", 0.1, pool2[l % len(pool2)], "kalman") for l in range(L)]
        assert all(abs(v2[k, l] - forecast_var_np(kt[l], h)) <= 1e-10 * v2[k, l] for l in range(L) for k, h in enumerate(hs))
        assert np.max(np.abs(v2 - v1)) > 1e-3


@pytest.mark.gpu
def test_stacked_model_returns_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    bank = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (4, 1)), kernel="Matern32x2")
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    fc = torch.zeros_like(Ty)
    hz = (C.c_int * 1)(1)
    var = np.zeros(4)
    for gains in (0, 1):
        rc = lib.moihgp_forecast_stream(bank._h, 0, C.c_void_p(Ty.data_ptr()), 64, 64, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), hz, 1,
                                        C.c_void_p(fc.data_ptr()), 64, 4 * 64, gains, None, None)
        assert rc == 3
    assert lib.moihgp_forecast_tail(bank._h, 0, C.c_void_p(x.data_ptr()), 64, C.c_void_p(fc.data_ptr()), 64, None) == 3
    assert lib.moihgp_forecast_variances(bank._h, hz, 1, var.ctypes.data_as(C.POINTER(C.c_double))) == 3
    with pytest.raises(MoihgpError):
        bank.forecast(Ty, [1])


@pytest.mark.gpu
def test_invalid_arguments_return_1_and_launch_nothing(env):
    torch, streams = env["torch"], env["streams"]
    bank, _, _ = make_bank(streams, "Matern52", 4, "kalman")
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    fc = torch.full((2, 4, 64), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda hz, K, ld_out=64, plane=256, gains=0, out=fc: lib.moihgp_forecast_stream(bank._h, 0, p(Ty), 64, 64, p(x), p(x), hz, K, p(out), ld_out,
                                                                                           plane, gains, None, None)
    h2 = (C.c_int * 2)(1, 5)
    assert call(h2, 2) == 0
    torch.cuda.synchronize()
    fc.fill_(7.0)
    assert call(h2, 0) == 1 and call((C.c_int * 9)(*range(9)), 9) == 1
    assert call((C.c_int * 2)(1, -1), 2) == 1 and call((C.c_int * 2)(1, HMAX + 1), 2) == 1
    assert call(h2, 2, ld_out=63) == 1 and call(h2, 2, plane=255) == 1 and call(h2, 2, plane=4 * 64 - 2) == 1
    assert call(h2, 2, gains=2) == 1
    assert call(h2, 2, out=Ty) == 1
    assert call(None, 2) == 1
    torch.cuda.synchronize()
    assert bool((fc == 7.0).all())
    var = np.zeros((9, 4))
    assert lib.moihgp_forecast_variances(bank._h, (C.c_int * 9)(*range(9)), 9, var.ctypes.data_as(C.POINTER(C.c_double))) == 1


@pytest.mark.gpu
def test_full_size_c3_fp32_sampled(env):
    """C3's shape: 4096 latents x 10^4 ticks, Matern-5/2, fp32, four horizons; 64 sampled latents against fp64 numpy."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(33)
    L, T, hs = 4096, 10000, [1, 10, 100, 1000]
    pool = [tuple(p) for p in np.column_stack([rng.uniform(0.5, 2, 32), rng.uniform(0.5, 2, 32), rng.uniform(0.02, 0.3, 32)])]
    bank, tbs, _ = make_bank(streams, "Matern52", L, "kalman", pool=pool)
    Ty = torch.randn((L, T), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    fc, _, status = bank.forecast(Ty, hs)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    idx = np.sort(rng.choice(L, 64, replace=False))
    ref, _, scale = forecast_np([tbs[i] for i in idx], Ty[idx].double().cpu().numpy(), hs)
    got = fc[:, idx].double().cpu().numpy()
    errs = [plane_err(got[k], ref[k], scale) for k in range(len(hs))]
    print("full size fp32 plane errors", errs)
    assert max(errs) <= FP32_TOL, errs


# ------------------------------------------------------------------------------------------------ C++ (predictAhead)
def test_cxx_predict_ahead_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "forecast_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_predict_ahead_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(34)
    M, L, T, h = 12, 4, 300, 6
    params, Y = end_to_end_inputs(rng, M, L, T, True)
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {h} {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
    out = cxx_run(cxx_test_binary(hip_built, "forecast_test"), inp)
    got = cxx_rows(out)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yf, _, _ = streams.forecast_outputs(gp, torch.from_numpy(Y).cuda(), [h])
    torch.cuda.synchronize()
    assert got.shape == (T, M)
    assert rel_err(got, Yf[0].cpu().numpy()) <= 1e-12
