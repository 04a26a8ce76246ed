"""Fixed-lag smoother (include/moihgp.h moihgp_lagged_stream / _variances): the numpy definition the GPU is held to -- the direct windowed sum,
pinned against its backward recursion, the dense GP conditional and the RTS smoother (CPU) -- then the library's tables and sweeps against it (GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

from conftest import rel_err, rel_err_rows
from parity_support import synth
from stream_reference import forward_np, lagged_np, lagged_var_np, project_np, smooth_np, tables
from stream_support import (FP32_TOL, KMAP, LAGS8, LMAX, POOL, assert_declared, assert_exported, bank_and_tables, cxx_fmt, cxx_rows, cxx_run,
                            cxx_test_binary, end_to_end_inputs, env, gaps_edges_blocks_inplace, padding_untouched, sentinel_out, to_dev,
                            tol_of)  # noqa: F401  (env: the module's fixture)
from stream_support import FP64_TIGHT as FP64_TOL

LAGGED_SYMBOLS = ("moihgp_lagged_stream", "moihgp_lagged_variances")
LAGS1 = [5]                                       # one lag per replay
LAGS3 = [40, 0, 2]                                # two per replay, and a repeated replay whose second plane is idle


# ------------------------------------------------------------------------------------------------ cross-checks of the numpy definition
def lagged_direct_np(tb, y, lags, x_in=None):
    """The definition, one latent: lag[k][t] = p[t] + (sum_{j=0..l_k, t+j<T} G^j K v[t+j])_0, as a direct sum."""
    p, v, _ = forward_np([tb], y[None, :], None if x_in is None else x_in[None, :])
    p, v = p[0], v[0]
    T = len(y)
    u = np.zeros(T); g = tb["K"].copy()
    for j in range(T):
        u[j] = g[0]; g = tb["G"] @ g
    out = np.zeros((len(lags), T))
    for k, l in enumerate(lags):
        J = min(int(l) + 1, T)
        out[k] = p + np.correlate(np.concatenate([v, np.zeros(J - 1)]), u[:J], "valid")
    return out


def dense_lagged(tb, y, ticks, lags):
    """Mean and variance of the latent function at tick t given y[0 .. t + l] under the stationary GP prior with covariance (A^k Pinf)_00, for
    every t in ticks and l in lags.  One Cholesky factor of the whole covariance serves every conditioning set y[0 .. n): its leading n x n block
    is the factor of the leading block, so with Z = Lc^-1 C and z = Lc^-1 y the conditional mean is Z[:n, t] . z[:n] and the variance
    c_0 - |Z[:n, t]|^2."""
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    T = len(y)
    c = np.zeros(T); M = np.eye(A.shape[0])
    for k in range(T):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    i = np.arange(T)
    Cm = c[np.abs(i[:, None] - i[None, :])]
    Lc = np.linalg.cholesky(Cm + R * np.eye(T))
    z = sl.solve_triangular(Lc, y, lower=True)
    Z = sl.solve_triangular(Lc, Cm[:, ticks], lower=True)                              # [T][len(ticks)]
    cm = np.cumsum(Z * z[:, None], axis=0); cv = np.cumsum(Z * Z, axis=0)
    mean = np.zeros((len(lags), len(ticks))); var = np.zeros_like(mean)
    for k, l in enumerate(lags):
        n = np.asarray(ticks) + l + 1
        mean[k] = cm[n - 1, np.arange(len(ticks))]
        var[k] = c[0] - cv[n - 1, np.arange(len(ticks))]
    return mean, var


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_lagged_entries():
    src = assert_declared(LAGGED_SYMBOLS)
    assert re.search(r"#define\s+MOIHGP_LAGGED_MAX_LAGS\s+8\b", src)


def test_library_exports_the_lagged_entries(hip_built):
    assert_exported(hip_built, LAGGED_SYMBOLS)


def _series(T, rng, gaps):
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    if gaps:
        y[[0, 3, 300, 301, 302, T - 1]] = np.nan
    return y


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_recursion_is_the_direct_sum(kern, gaps):
    rng = np.random.default_rng(1)
    tb = tables(kern, 0.1, [1.3, 0.7, 0.05])
    y = _series(600, rng, gaps)
    lags = [0, 1, 5, 37, 700, LMAX]
    x0 = 0.1 * rng.standard_normal(tb["A"].shape[0])
    direct = lagged_direct_np(tb, y, lags, x0)
    rec, p, _ = lagged_np([tb], y[None, :], lags, x0[None, :])
    for k in range(len(lags)):
        assert np.max(np.abs(rec[k, 0] - direct[k])) <= 1e-12 * np.max(np.abs(direct[k])), lags[k]
    # a lag that reaches past the end is the RTS smoother; lag 0 is the filtered mean p + K_0 v
    ys, _ = smooth_np([tb], y[None, :], x0[None, :])
    for k in (4, 5):
        assert np.max(np.abs(direct[k] - ys[0])) <= 1e-12 * np.max(np.abs(ys))
    v = np.where(np.isnan(y), 0.0, y - p[0])
    assert np.max(np.abs(direct[0] - (p[0] + tb["K"][0] * v))) <= 1e-12 * np.max(np.abs(direct[0]))


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_interior_is_the_gp_conditional(kern):
    """Ticks 500 .. 1000 of a gap-free stream of 1500, conditioning set y[0 .. t + l]: mean and variance of the dense GP conditional."""
    rng = np.random.default_rng(2)
    tb = tables(kern, 0.1, [1.3, 0.7, 0.05])
    T, lags = 1500, [0, 1, 5, 50]
    y = _series(T, rng, False)
    ticks = np.arange(500, 1001)
    mean, var = dense_lagged(tb, y, ticks, lags)
    direct = lagged_direct_np(tb, y, lags)
    for k, l in enumerate(lags):
        assert np.max(np.abs(direct[k][ticks] - mean[k])) <= 1e-9, l
        assert np.max(np.abs(var[k] - lagged_var_np(tb, l))) <= 1e-9, l


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_variance_falls_from_var_filtered_to_var_smoothed(kern):
    for prm in POOL:
        tb = tables(kern, 0.1, prm)
        assert abs(lagged_var_np(tb, 0) - tb["var_f"]) <= 1e-12 * tb["var_f"]
        assert abs(lagged_var_np(tb, LMAX) - tb["var_s"]) <= 1e-12 * tb["var_s"]
        v = np.array([lagged_var_np(tb, l) for l in list(range(0, 200)) + [300, 1000, 10000, LMAX]])
        # non-increasing, up to the rounding of the terms of the sum (each of var_filtered's size at the most)
        assert np.all(np.diff(v) <= 4 * np.finfo(float).eps * tb["var_f"]), prm
        assert v[0] > v[-1]


def test_python_argument_validation():
    from multioutputihgp_amd import streams
    for bad in ([], list(range(9)), [-1], [LMAX + 1], [1.5], [True], 3):
        with pytest.raises(ValueError):
            streams._int_list(bad, "lag", streams.LAGGED_MAX_LAGS)
    arr, K = streams._int_list(np.array([3, 0, LMAX]), "lag", streams.LAGGED_MAX_LAGS)
    assert K == 3 and list(arr) == [3, 0, LMAX]


def test_cxx_predict_lagged_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "lagged_test"))


# ------------------------------------------------------------------------------------------------ GPU
_CASES = {}


def parity_case(kern, L, T, gaps):
    """Stream, start state and numpy reference of one parity case, shared by the dtypes (the data are fp32 numbers) and kept unchanged."""
    key = (kern, L, T, gaps)
    if key not in _CASES:
        rng = np.random.default_rng(L * 100003 + T + (7 if gaps else 0))
        tbs = [tables(kern, 0.1, POOL[l % len(POOL)]) for l in range(len(POOL))]
        tbs = [tbs[l % len(POOL)] for l in range(L)]
        Ty = synth(L, T, rng)
        if gaps:
            Ty = gaps_edges_blocks_inplace(Ty, rng)
        Ty = Ty.astype(np.float32).astype(np.float64)
        x0 = (0.1 * rng.standard_normal((L, tbs[0]["A"].shape[0]))).astype(np.float32).astype(np.float64)
        ref, p, xe = lagged_np(tbs, Ty, LAGS8 + LAGS1 + LAGS3, x0)
        _CASES[key] = dict(Ty=Ty, x0=x0, p=p, xe=xe, ref={"8": ref[:8], "1": ref[8:9], "3": ref[9:]})
    return _CASES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("L", [1, 7, 256])
@pytest.mark.parametrize("T", [1, 2, 63, 1000, 1024, 1025, 2100])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lagged_parity(env, kern, L, T, dtype, gaps):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    case = parity_case(kern, L, T, gaps)
    bank, _, _ = bank_and_tables(streams, kern, L)
    dev = to_dev(torch, case["Ty"], tdt, T)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    for name, lags in (("8", LAGS8), ("1", LAGS1), ("3", LAGS3)):
        K = len(lags)
        slab, out = sentinel_out(torch, K, L, T, tdt)                # ld_out != ld_in, plane_stride > L * ld_out
        ldo = out.stride(1)
        yslab = torch.full((L * ldo + 16,), 12345.0, dtype=tdt, device="cuda")
        yp = torch.as_strided(yslab, (L, T), (ldo, 1), 0)
        x = torch.empty_like(x_start)
        lg, ypred, x, status = bank.lagged(dev, lags, x=x, x_start=x_start, out=out, ypred=yp)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        got = lg.double().cpu().numpy()
        errs = [rel_err_rows(got[k], case["ref"][name][k]) for k in range(K)]
        ep = rel_err_rows(ypred.double().cpu().numpy(), case["p"])
        ex = rel_err_rows(x.double().cpu().numpy(), case["xe"], floor=1e-3)
        print(f"{kern} {dtype} L={L} T={T} gaps={gaps} lags={lags}: planes {['%.1e' % e for e in errs]}, ypred {ep:.1e}, end state {ex:.1e}")
        assert max(errs) <= tol_of(dtype), errs
        assert ep <= tol_of(dtype) and ex <= tol_of(dtype), (ep, ex)
        assert padding_untouched(torch, slab, out) and padding_untouched(torch, yslab, yp)
        assert ypred.data_ptr() == yp.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ypred_on_another_row_stride_than_out(env, dtype):
    """The C entry takes one row stride for both buffers, so lagged() sweeps into a buffer of the planes' stride and copies it into a caller's `ypred`
    of another stride: the caller's tensor comes back, bit-equal to a call without the copy, and nothing between its rows is written.  L = 3 (one
    latent has no row stride), T = 17: one ragged 16-tick chunk."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    L, T, lags, vec = 3, 17, [0, 3], 16 // (8 if dtype == "f64" else 4)
    ld = streams.padded_len(T, tdt)
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    dev = to_dev(torch, synth(L, T, np.random.default_rng(23)), tdt, T)

    def carve(K, ldo):
        slab = torch.full((K * L * ldo + 16,), 12345.0, dtype=tdt, device="cuda")
        return slab, torch.as_strided(slab, (K, L, T), (L * ldo, ldo, 1), 0)
    res = []
    for ld_yp in (ld + 2 * vec, ld + vec):          # ypred rows two vectors longer than T rounded up, then of out's stride: one more
        oslab, out = carve(len(lags), ld + vec)
        yslab, yp3 = carve(1, ld_yp)
        lg, ypred, _, status = bank.lagged(dev, lags, out=out, ypred=yp3[0])
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        assert lg.data_ptr() == out.data_ptr() and ypred.data_ptr() == yp3.data_ptr() and ypred.stride(0) == ld_yp
        assert padding_untouched(torch, oslab, out) and padding_untouched(torch, yslab, yp3)
        res.append((ypred.cpu().numpy(), lg.cpu().numpy()))
    assert np.isfinite(res[0][0]).all() and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_family_identities_on_the_device(env, kern, dtype):
    """Lag 0 is the filtered mean of forecast([0]), a lag >= T is smooth(), and ypred is the one-step forecast."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(21)
    L, T = 7, 2100
    bank, _, _ = bank_and_tables(streams, kern, L)
    Ty = gaps_edges_blocks_inplace(synth(L, T, rng), rng)
    dev = to_dev(torch, Ty, tdt, T)
    lg, ypred, xl, _ = bank.lagged(dev, [0, T, LMAX])
    fc, xf, _ = bank.forecast(dev, [0, 1], gains="kalman")
    ys, xs, _ = bank.smooth(dev)
    torch.cuda.synchronize()
    n = lambda t: t.double().cpu().numpy()
    assert rel_err_rows(n(lg[0]), n(fc[0])) <= tol_of(dtype)
    assert rel_err_rows(n(lg[1]), n(ys)) <= tol_of(dtype) and rel_err_rows(n(lg[2]), n(ys)) <= tol_of(dtype)
    assert rel_err_rows(n(ypred[:, 1:]), n(fc[1][:, :-1])) <= tol_of(dtype)
    assert rel_err_rows(n(xl), n(xs), floor=1e-3) <= tol_of(dtype) and rel_err_rows(n(xl), n(xf), floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scan_and_serial_paths_agree(env, kern, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    case = parity_case(kern, 7, 2100, True)
    bank, _, _ = bank_and_tables(streams, kern, 7)
    dev = to_dev(torch, case["Ty"], tdt, 2100)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    res = []
    for path in (0, 1):
        bank.set_option("lagged_path", path)
        lg, yp, x, st = bank.lagged(dev, LAGS8, x_start=x_start)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        res.append((lg.double().cpu().numpy(), yp.double().cpu().numpy(), x.double().cpu().numpy()))
    between = 1e-11 if dtype == "f64" else FP32_TOL
    for k in range(len(LAGS8)):
        assert rel_err_rows(res[0][0][k], res[1][0][k]) <= between, (k, rel_err_rows(res[0][0][k], res[1][0][k]))
        for r in res:
            assert rel_err_rows(r[0][k], case["ref"]["8"][k]) <= tol_of(dtype)
    assert rel_err_rows(res[0][1], res[1][1]) <= between and rel_err_rows(res[0][2], res[1][2], floor=1e-3) <= between
    for r in res:
        assert rel_err_rows(r[1], case["p"]) <= tol_of(dtype) and rel_err_rows(r[2], case["xe"], floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
def test_growth_bound_fallback(env):
    """The latent of test_smoother.test_growth_bound_fallback (Matern-5/2, lengthscale 0.01 at dt 0.01) fails the scan kernels' growth bound: the
    automatic path walks it serially (bit for bit the all-serial result), the others take the scan; all match numpy on the device's own tables."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(22)
    pool = [(1.0, 0.01, 0.01), (1.0, 1.0, 0.1), (0.7, 0.5, 0.05), (1.0, 0.03, 1e-4)]
    L, T, lags = 8, 2100, [0, 3, 40, 1024, LMAX]
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L, dt=0.01, pool=pool)
    t = tbs[0]
    G, F = t["G"], t["A"] - np.outer(t["K"], t["A"][0])
    assert max(np.abs(np.linalg.matrix_power(M, k)).sum(1).max() for M in (G, F) for k in range(1, 33)) > 1e4   # the fallback is reached
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, torch.float64, T)
    res = {}
    for path in (-1, 0, 1):
        bank.set_option("lagged_path", path)
        lg, yp, x, st = bank.lagged(dev, lags, state_at=1500)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        res[path] = (lg.cpu().numpy(), yp.cpu().numpy(), x.cpu().numpy())
    dtb = [dict(A=bank.latent(l)["A"], **{k: v for k, v in bank.smoother(l).items() if k in ("K", "G")}) for l in range(L)]
    ref, p, xe = lagged_np(dtb, Ty, lags, state_at=1500)
    for k in range(len(lags)):
        assert rel_err_rows(res[-1][0][k], ref[k]) <= 1e-9, (k, rel_err_rows(res[-1][0][k], ref[k]))
    assert rel_err_rows(res[-1][1], p) <= 1e-9 and rel_err_rows(res[-1][2], xe, floor=1e-3) <= 1e-9
    # the growth figure of every latent (inf-norm of the powers of G and A - K H A up to 32): well above the bound of 1e4 the automatic path is the
    # serial walk itself, well below it the scan kernels' result, bit for bit
    growth = [max(np.abs(np.linalg.matrix_power(M, k)).sum(1).max() for M in (t["G"], t["A"] - np.outer(t["K"], t["A"][0])) for k in range(1, 33))
              for t in dtb]
    serial = [l for l in range(L) if growth[l] > 2e4]
    scan = [l for l in range(L) if growth[l] < 5e3]
    assert 0 in serial and 4 in serial and len(scan) >= 4, growth
    for i in range(3):
        assert np.array_equal(res[-1][i][..., serial, :], res[1][i][..., serial, :])
        assert np.array_equal(res[-1][i][..., scan, :], res[0][i][..., scan, :])


@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_latent_gives_nan_rows_and_status_1(env, path, dtype):
    """A latent whose DARE cannot converge (NaN magnitude): status 1, NaN in all K rows, in ypred and in x; the other latents are untouched."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(23)
    L, T, bad, lags = 7, 2100, 3, [0, 7, 2000]
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("lagged_path", path)
    Ty = synth(L, T, rng).astype(np.float32).astype(np.float64)
    lg, yp, x, status = bank.lagged(to_dev(torch, Ty, tdt, T), lags)
    torch.cuda.synchronize()
    st, got, gp, xg = status.cpu().numpy(), lg.double().cpu().numpy(), yp.double().cpu().numpy(), x.double().cpu().numpy()
    assert st[bad] == 1 and np.all(np.isnan(got[:, bad])) and np.all(np.isnan(gp[bad])) and np.all(np.isnan(xg[bad]))
    keep = [l for l in range(L) if l != bad]
    assert not st[keep].any()
    ref, p, xe = lagged_np([tbs[l] for l in keep], Ty[keep], lags)
    for k in range(len(lags)):
        assert rel_err_rows(got[k][keep], ref[k]) <= tol_of(dtype)
    assert rel_err_rows(gp[keep], p) <= tol_of(dtype) and rel_err_rows(xg[keep], xe, floor=1e-3) <= tol_of(dtype)
    var = bank.lagged_variances(lags)
    assert np.all(np.isnan(var[:, bad])) and np.all(np.isfinite(var[:, keep]))


@pytest.mark.gpu
def test_lagged_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(24)
    M, L, T = 8, 3, 100
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.lagged_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda(), [2])


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_variances_match_numpy(env, kern):
    bank, tbs, _ = bank_and_tables(env["streams"], kern, 8)
    lags = [0, 1, 2, 5, 37, 700, 4096, LMAX]
    var = bank.lagged_variances(lags)
    vf, vs = bank.latent_variances()
    assert var.shape == (8, 8)
    for l in range(8):
        for k, lag in enumerate(lags):
            ref = lagged_var_np(tbs[l], lag)
            assert abs(var[k, l] - ref) <= 1e-10 * ref, (l, lag)
        assert abs(var[0, l] - vf[l]) <= 1e-10 * vf[l] and abs(var[-1, l] - vs[l]) <= 1e-10 * vs[l]
        assert np.all(np.diff(var[:, l]) <= 4 * np.finfo(float).eps * vf[l]) and var[0, l] > var[-1, l]


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_slabs_reproduce_the_whole_stream(env, kern, dtype):
    """A stream of 2100 ticks in slabs of 700 with lags [3, 40]: each call sees its slab and max(lags) ticks of lookahead, starts from the carried
    state and returns the state at the slab's end; the kept ticks are the whole-stream call's."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    case = parity_case(kern, 7, 2100, True)
    L, T, slab, lags = 7, 2100, 700, [3, 40]
    Ty, x0 = case["Ty"], case["x0"]
    tbs = [tables(kern, 0.1, POOL[l % len(POOL)]) for l in range(L)]
    bank, _, _ = bank_and_tables(streams, kern, L)
    dev = to_dev(torch, Ty, tdt, T)
    whole, wp, wx, _ = bank.lagged(dev, lags, x_start=torch.from_numpy(x0).to(tdt).cuda())
    ref, p, _ = lagged_np(tbs, Ty, lags, x0)
    carry = torch.from_numpy(x0).to(tdt).cuda()
    parts, pparts = [], []
    for t0 in range(0, T, slab):
        t1 = t0 + slab
        hi = min(t1 + max(lags), T)
        piece = to_dev(torch, Ty[:, t0:hi], tdt, hi - t0)
        lg, yp, carry, st = bank.lagged(piece, lags, x_start=carry, state_at=t1 - t0)
        carry = carry.clone()
        parts.append(lg[:, :, :t1 - t0].clone()); pparts.append(yp[:, :t1 - t0].clone())
        _, _, xref = forward_np(tbs, Ty, x0, state_at=t1)            # a walk of the whole stream to that tick
        torch.cuda.synchronize()
        assert rel_err_rows(carry.double().cpu().numpy(), xref, floor=1e-3) <= tol_of(dtype), t1
    torch.cuda.synchronize()
    got = torch.cat(parts, dim=2).double().cpu().numpy()
    gp = torch.cat(pparts, dim=1).double().cpu().numpy()
    for k in range(len(lags)):
        assert rel_err_rows(got[k], whole[k].double().cpu().numpy()) <= tol_of(dtype)
        assert rel_err_rows(got[k], ref[k]) <= tol_of(dtype)
    assert rel_err_rows(gp, wp.double().cpu().numpy()) <= tol_of(dtype) and rel_err_rows(gp, p) <= tol_of(dtype)
    assert rel_err_rows(carry.double().cpu().numpy(), wx.double().cpu().numpy(), floor=1e-3) <= tol_of(dtype)


@pytest.mark.gpu
def test_state_at_zero_returns_the_start_state(env):
    torch, streams = env["torch"], env["streams"]
    bank, _, _ = bank_and_tables(streams, "Matern52", 7)
    rng = np.random.default_rng(25)
    x0 = torch.from_numpy(rng.standard_normal((7, bank.d))).cuda()
    for path in (0, 1):
        bank.set_option("lagged_path", path)
        _, _, x, _ = bank.lagged(to_dev(torch, synth(7, 100, rng), torch.float64, 100), [2], x_start=x0, state_at=0)
        torch.cuda.synchronize()
        assert torch.equal(x, x0)


@pytest.mark.gpu
def test_invalid_arguments_return_1_and_write_nothing(env):
    torch, streams = env["torch"], env["streams"]
    bank, _, _ = bank_and_tables(streams, "Matern52", 4)
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    both = torch.full((3, 4, 64), 7.0, dtype=torch.float64, device="cuda")
    out, yp = both[:2], both[2]
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda lg, K, ld_out=64, plane=256, out=out, ypred=yp, T_state=64: lib.moihgp_lagged_stream(
        bank._h, 0, p(Ty), 64, 64, p(x), p(x), T_state, lg, K, p(ypred), p(out), ld_out, plane, None, None)
    l2 = (C.c_int * 2)(1, 5)
    assert call(l2, 2) == 0
    torch.cuda.synchronize()
    both.fill_(7.0)
    assert call(l2, 0) == 1 and call((C.c_int * 9)(*range(9)), 9) == 1
    assert call((C.c_int * 2)(1, -1), 2) == 1 and call((C.c_int * 2)(1, LMAX + 1), 2) == 1
    assert call(l2, 2, ld_out=63) == 1 and call(l2, 2, plane=255) == 1 and call(l2, 2, plane=4 * 64 - 2) == 1
    assert call(l2, 2, out=Ty) == 1 and call(l2, 2, ypred=Ty) == 1 and call(l2, 2, ypred=out[1]) == 1
    assert call(l2, 2, T_state=65) == 1
    assert call(None, 2) == 1
    torch.cuda.synchronize()
    assert bool((both == 7.0).all()) and bool((Ty == 0.0).all())
    var = np.zeros((9, 4))
    assert lib.moihgp_lagged_variances(bank._h, (C.c_int * 9)(*range(9)), 9, var.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert lib.moihgp_set_option(bank._h, b"lagged_path", 2) == 1
    with pytest.raises(ValueError):
        bank.lagged(Ty, [1], state_at=65)
    from multioutputihgp_amd import MoihgpError
    with pytest.raises(MoihgpError, match="must not overlap"):
        bank.lagged(Ty, [1], out=both[:1], ypred=both[0])


@pytest.mark.gpu
def test_stacked_model_returns_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    bank = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (4, 1)), kernel="Matern32x2")
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    out, yp = torch.zeros_like(Ty), torch.zeros_like(Ty)
    lg = (C.c_int * 1)(1)
    var = np.zeros(4)
    rc = lib.moihgp_lagged_stream(bank._h, 0, C.c_void_p(Ty.data_ptr()), 64, 64, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 64, lg, 1,
                                  C.c_void_p(yp.data_ptr()), C.c_void_p(out.data_ptr()), 64, 4 * 64, None, None)
    assert rc == 3
    assert lib.moihgp_lagged_variances(bank._h, lg, 1, var.ctypes.data_as(C.POINTER(C.c_double))) == 3
    with pytest.raises(MoihgpError):
        bank.lagged(Ty, [1])


@pytest.mark.gpu
def test_lagged_after_update_uses_the_new_parameters(env):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(26)
    L, T, lags = 7, 1000, [0, 3, 40]
    Ty = synth(L, T, rng)
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L)
    l1, _, _, _ = bank.lagged(to_dev(torch, Ty, torch.float64, T), lags)
    torch.cuda.synchronize()
    ref, _, _ = lagged_np(tbs, Ty, lags)
    assert max(rel_err_rows(l1.cpu().numpy()[k], ref[k]) for k in range(3)) <= FP64_TOL
    v1 = bank.lagged_variances(lags)
    pool2 = [(p[0] * 1.5, p[1] * 0.7, p[2] * 2.0) for p in POOL]
    bank.update(np.array([pool2[l % len(pool2)] for l in range(L)]))
    l2, _, _, _ = bank.lagged(to_dev(torch, Ty, torch.float64, T), lags)
    torch.cuda.synchronize()
    tbs2 = [tables("Matern52", 0.1, pool2[l % len(pool2)]) for l in range(L)]
    ref2, _, _ = lagged_np(tbs2, Ty, lags)
    assert max(rel_err_rows(l2.cpu().numpy()[k], ref2[k]) for k in range(3)) <= FP64_TOL
    assert max(rel_err_rows(l2.cpu().numpy()[k], ref[k]) for k in range(3)) > 1e-3            # (and they do differ)
    v2 = bank.lagged_variances(lags)
    # (1e-9: the scaled pool's R = 2e-6 entry has var_filtered = P_00 R / S, which P - K H P loses S / R = 1e6 of fp64's 1e-16 on, in scipy's
    # tables as on the device; the 1e-10 of the tables is asserted on POOL itself in test_variances_match_numpy)
    assert all(abs(v2[k, l] - lagged_var_np(tbs2[l], h)) <= 1e-9 * v2[k, l] for l in range(L) for k, h in enumerate(lags))
    assert np.max(np.abs(v2 - v1)) > 1e-3


@pytest.mark.gpu
def test_calls_on_two_streams_keep_their_own_tables(env):
    """A call on a second stream right after one on the first, with other lags: the second rewrites the handle's per-call tables only after the
    first has finished with them (the tables' event), so both match their references."""
    torch, streams = env["torch"], env["streams"]
    case = parity_case("Matern52", 256, 2100, True)
    bank, _, _ = bank_and_tables(streams, "Matern52", 256)
    dev = to_dev(torch, case["Ty"], torch.float64, 2100)
    x_start = torch.from_numpy(case["x0"]).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = bank.lagged(dev, LAGS8, x_start=x_start, stream=s1)
    b = bank.lagged(dev, LAGS3, x_start=x_start, stream=s2)
    c = bank.lagged(dev, LAGS8, x_start=x_start, stream=s2)
    torch.cuda.synchronize()
    for k in range(8):
        assert rel_err_rows(a[0][k].cpu().numpy(), case["ref"]["8"][k]) <= FP64_TOL
        assert torch.equal(a[0][k], c[0][k])
    for k in range(3):
        assert rel_err_rows(b[0][k].cpu().numpy(), case["ref"]["3"][k]) <= FP64_TOL


def _lagged_outputs_np(gp, Y, kern, lags):
    U, S, igp, Ty = project_np(gp, Y, nan_below_L=True)
    tbs = [tables(kern, 0.1, igp[l]) for l in range(len(igp))]
    lg, _, _ = lagged_np(tbs, Ty, lags)
    var = np.array([[lagged_var_np(tb, l) for tb in tbs] for l in lags])
    return np.einsum("ml,klt->ktm", U * np.sqrt(S), lg), (S[None, :] * var) @ (U ** 2).T


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("missing", [False, True])
def test_lagged_outputs_end_to_end(env, kern, missing):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(27)
    M, L, T, lags = 6, 3, 300, [0, 4, 25, 300]
    params, Y = end_to_end_inputs(rng, M, L, T, missing)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yl, var = streams.lagged_outputs(gp, torch.from_numpy(Y).cuda(), lags)
    torch.cuda.synchronize()
    ref, vref = _lagged_outputs_np(gp, Y, kern, lags)
    assert tuple(Yl.shape) == (len(lags), T, M) and var.shape == (len(lags), M)
    for k in range(len(lags)):
        assert rel_err(Yl[k].cpu().numpy(), ref[k]) <= FP64_TOL, (k, rel_err(Yl[k].cpu().numpy(), ref[k]))
    assert rel_err(var, vref) <= 1e-10
    Ys, _ = streams.smooth_outputs(gp, torch.from_numpy(Y).cuda())
    assert rel_err(Yl[3].cpu().numpy(), Ys.cpu().numpy()) <= FP64_TOL


# ------------------------------------------------------------------------------------------------ C++ (predictLagged)
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_predict_lagged_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(28)
    M, L, T, lag = 12, 4, 300, 6
    params, Y = end_to_end_inputs(rng, M, L, T, True)
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {lag} {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
    out = cxx_run(cxx_test_binary(hip_built, "lagged_test"), inp)
    got = cxx_rows(out)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yl, _ = streams.lagged_outputs(gp, torch.from_numpy(Y).cuda(), [lag])
    torch.cuda.synchronize()
    assert got.shape == (T, M)
    assert rel_err(got, Yl[0].cpu().numpy()) <= 1e-12
