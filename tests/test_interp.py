"""Off-grid smoother (include/moihgp.h moihgp_interp_stream / _variances): the numpy definition the GPU is held to -- the RTS smoother with an
unobserved point inserted between two ticks, pinned against the dense GP posterior on a refined grid and against the smoother itself (CPU) -- then
the library's tables and sweeps against it (GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

from conftest import rel_err, rel_err_rows
from parity_support import synth
from stream_reference import F_of, interp_np, interp_rows_np, project_np, smooth_np, tables
from stream_support import (DT, FRACS1, FRACS3, FRACS8, KMAP, POOL, VAR_EDGE, VAR_INNER, assert_declared, assert_exported, bank_and_tables,
                            cxx_fmt, cxx_rows, cxx_run, cxx_test_binary, end_to_end_inputs, env, gaps_edges_inplace, padding_untouched, pool_models,
                            sentinel_out, to_dev, tol_of)  # noqa: F401  (env: the module's fixture)
from stream_support import FP64_TIGHT as FP64_TOL

INTERP_SYMBOLS = ("moihgp_interp_stream", "moihgp_interp_variances")


def var_edge_bound(tb, var):
    return max(1e-10, float(np.finfo(np.float64).eps * np.linalg.cond(tb["P"]) * tb["P"][0, 0] / var))


# ------------------------------------------------------------------------------------------------ cross-check of the numpy definition
def dense_refined(tb, F, dt, y, n, ticks):
    """Mean and variance of the latent function on the grid dt / n at the points (t + j / n) dt, t in ticks, 0 <= j < n, given y observed at every
    n-th point, under the stationary GP prior with covariance (expm(F tau) Pinf)_00.  Returns (mean [n][len(ticks)], var [n][len(ticks)])."""
    T = len(y)
    N = n * T
    Af = sl.expm(F * (dt / n))
    c = np.zeros(N); M = np.eye(F.shape[0])
    for k in range(N):
        c[k] = (M @ tb["Pinf"])[0, 0]; M = Af @ M
    obs = n * np.arange(T)
    Kd = c[np.abs(obs[:, None] - obs[None, :])] + tb["R"] * np.eye(T)
    Lc = np.linalg.cholesky(Kd)
    z = sl.solve_triangular(Lc, y, lower=True)
    mean = np.zeros((n, len(ticks))); var = np.zeros_like(mean)
    for j in range(n):
        pts = n * np.asarray(ticks) + j
        Z = sl.solve_triangular(Lc, c[np.abs(obs[:, None] - pts[None, :])], lower=True)
        mean[j] = Z.T @ z
        var[j] = c[0] - np.sum(Z * Z, axis=0)
    return mean, var


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_interp_entries():
    src = assert_declared(INTERP_SYMBOLS)
    assert re.search(r"#define\s+MOIHGP_INTERP_MAX_POINTS\s+8\b", src)


def test_library_exports_the_interp_entries(hip_built):
    assert_exported(hip_built, INTERP_SYMBOLS)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_interior_is_the_gp_posterior_on_a_refined_grid(kern):
    """T = 400 ticks observed on every fourth point of a dt / 4 grid, the whole POOL, offsets 1/4, 1/2, 3/4, ticks 150 .. 250."""
    rng = np.random.default_rng(1)
    T, fracs, ticks = 400, [0.25, 0.5, 0.75], np.arange(150, 251)
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    for prm in POOL:
        tb, F = tables(kern, DT, prm), F_of(kern, DT, prm)
        fine, ys, _, var = interp_np([tb], [F], DT, fracs, y[None, :])
        mean, dvar = dense_refined(tb, F, DT, y, 4, ticks)
        em = max(np.max(np.abs(fine[k, 0, ticks] - mean[k + 1])) for k in range(3))
        ev = max(np.max(np.abs(dvar[k + 1] - var[k, 0])) / var[k, 0] for k in range(3))
        print(f"{kern} {prm}: mean {em:.1e}, variance {ev:.1e}")
        assert np.max(np.abs(ys[0, ticks] - mean[0])) <= 1e-9, prm
        assert em <= 1e-9, (prm, em)
        assert ev <= 1e-9, (prm, ev)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_offset_zero_is_the_smoother_and_the_last_tick_a_forecast(kern):
    rng = np.random.default_rng(2)
    T = 600
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    y[[0, 3, 300, 301, 302, T - 1]] = np.nan
    for prm in POOL:
        tb, F = tables(kern, DT, prm), F_of(kern, DT, prm)
        x0 = 0.1 * rng.standard_normal((1, F.shape[0]))
        fine, ys, xe, var = interp_np([tb], [F], DT, [0.0, 0.5], y[None, :], x0)
        ref, xref = smooth_np([tb], y[None, :], x0)
        scale = np.max(np.abs(ref))
        assert np.max(np.abs(fine[0] - ref)) <= 1e-12 * scale and np.max(np.abs(ys - ref)) <= 1e-12 * scale
        assert np.max(np.abs(xe - xref)) <= 1e-12 * np.max(np.abs(xref))
        assert abs(fine[1, 0, T - 1] - (sl.expm(F * DT / 2) @ xe[0])[0]) <= 1e-12 * scale
        assert abs(var[0, 0] - tb["var_s"]) <= 1e-10 * tb["var_s"]


def _expm_ld(M):
    """expm in np.longdouble: scaling and squaring of the Taylor series."""
    LD = np.longdouble
    M = M.astype(LD)
    n = float(np.max(np.abs(M).sum(1)))
    sq = max(0, int(np.ceil(np.log2(n))) + 4) if n > 0 else 0
    X = M / LD(2 ** sq)
    E = np.eye(M.shape[0], dtype=LD); term = np.eye(M.shape[0], dtype=LD)
    for k in range(1, 40):
        term = term @ X / LD(k); E = E + term
    for _ in range(sq):
        E = E @ E
    return E


def _inv_ld(A):
    LD = np.longdouble
    n = A.shape[0]
    M = np.concatenate([A.astype(LD), np.eye(n, dtype=LD)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, n:]


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_variance_rounding_error(kern):
    """What the fp64 variance of interp_rows_np is worth: against the same formula in 80-bit arithmetic on the same tables it is within 1e-11 at
    VAR_INNER over the whole POOL (so a 1e-10 comparison there tests the library, not the reference) and within var_edge_bound at VAR_EDGE."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18
    for prm in POOL:
        tb, F = tables(kern, DT, prm), F_of(kern, DT, prm)
        PF, Pinf, P, Ps = [tb[k].astype(LD) for k in ("PF", "Pinf", "P", "Ps")]
        for phi in VAR_INNER + VAR_EDGE:
            Ap, Bp = _expm_ld(F.astype(LD) * LD(phi) * LD(DT)), _expm_ld(F.astype(LD) * (LD(1) - LD(phi)) * LD(DT))
            Pp = Ap @ PF @ Ap.T + Pinf - Ap @ Pinf @ Ap.T
            Gp = Pp @ Bp.T @ _inv_ld(P)
            exact = float((Pp + Gp @ (Ps - P) @ Gp.T)[0, 0])
            err = abs(interp_rows_np(tb, F, DT, phi)[2] - exact) / exact
            assert err <= (1e-11 if phi in VAR_INNER else var_edge_bound(tb, exact)), (prm, phi, err)


def test_python_argument_validation():
    from multioutputihgp_amd import streams
    assert streams.INTERP_MAX_POINTS == 8
    for ok in ([0], [0.999], np.array([0.25, 0.5]), [0.0] * 8):
        arr, K = streams._frac_list(ok)
        assert K == len(ok) and list(arr) == [float(v) for v in ok]
    for bad in ([], [0.1] * 9, [1.0], [-0.1], [float("nan")], [float("inf")], "0.5", ["0.5"], [True], 0.5):
        with pytest.raises(ValueError):
            streams._frac_list(bad)


def test_cxx_predict_between_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "interp_test"))


# ------------------------------------------------------------------------------------------------ GPU
_CASES = {}


def parity_case(kern, L, T):
    """Stream, start state and numpy reference of one parity case, shared by the dtypes (the data are fp32 numbers) and kept unchanged."""
    key = (kern, L, T)
    if key not in _CASES:
        rng = np.random.default_rng(L * 100003 + T)
        tbs, Fs = pool_models(kern, L)
        Ty = synth(L, T, rng)
        if T >= 16:
            Ty = gaps_edges_inplace(Ty, rng)
        Ty = Ty.astype(np.float32).astype(np.float64)
        x0 = (0.1 * rng.standard_normal((L, Fs[0].shape[0]))).astype(np.float32).astype(np.float64)
        sets = [("1", FRACS1), ("3", FRACS3)] + ([("8", FRACS8)] if L == 7 else [])
        fine, ys, xe, _ = interp_np(tbs, Fs, DT, sum((f for _, f in sets), []), Ty, x0)
        ref, k = {}, 0
        for name, f in sets:
            ref[name] = fine[k:k + len(f)]; k += len(f)
        _CASES[key] = dict(Ty=Ty, x0=x0, ys=ys, xe=xe, ref=ref, sets=sets)
    return _CASES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("L", [1, 7, 256])
@pytest.mark.parametrize("T", [1, 2, 16, 17, 1024, 1025, 2065])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_interp_parity(env, kern, L, T, dtype):
    """One chunk, the chunk edge, the segment edge, two segments plus a chunk; one, three and (L = 7) eight offsets; a non-zero start state;
    `out` and `ysmooth` on other row strides than the stream's; missing ticks at the ends and on both sides of the edges."""
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    case = parity_case(kern, L, T)
    bank, _, _ = bank_and_tables(streams, kern, L)
    dev = to_dev(torch, case["Ty"], tdt, T)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    for name, fracs in case["sets"]:
        K = len(fracs)
        slab, out = sentinel_out(torch, K, L, T, tdt)                # ld_out != ld_in, plane_stride > L * ld_out
        ldo = out.stride(1)
        yslab = torch.full((L * ldo + 16,), 12345.0, dtype=tdt, device="cuda")
        ysm = torch.as_strided(yslab, (L, T), (ldo, 1), 0)
        x = torch.empty_like(x_start)
        fine, ys, x, status = bank.interpolate(dev, fracs, x=x, x_start=x_start, out=out, ysmooth=ysm)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        got = fine.double().cpu().numpy()
        errs = [rel_err_rows(got[k], case["ref"][name][k]) for k in range(K)]
        ey = rel_err_rows(ys.double().cpu().numpy(), case["ys"])
        ex = rel_err_rows(x.double().cpu().numpy(), case["xe"], floor=1e-3)
        print(f"{kern} {dtype} L={L} T={T} fracs={fracs}: planes {['%.1e' % e for e in errs]}, ysmooth {ey:.1e}, end state {ex:.1e}")
        assert max(errs) <= tol_of(dtype), errs
        assert ey <= tol_of(dtype) and ex <= tol_of(dtype), (ey, ex)
        assert padding_untouched(torch, slab, out) and padding_untouched(torch, yslab, ysm)
        assert fine.data_ptr() == out.data_ptr() and ys.data_ptr() == ysm.data_ptr()


@pytest.mark.gpu
def test_ysmooth_on_another_row_stride_than_out(env):
    """The C entry takes one row stride for both buffers: a caller's `ysmooth` of another stride than `out` comes back filled, equal to a call
    without the copy."""
    torch, streams = env["torch"], env["streams"]
    L, T = 3, 17
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    dev = to_dev(torch, synth(L, T, np.random.default_rng(3)), torch.float64, T)
    slab, out = sentinel_out(torch, 2, L, T, torch.float64)
    mine = torch.full((L, 64), 12345.0, dtype=torch.float64, device="cuda")
    fine, ys, _, status = bank.interpolate(dev, [0.0, 0.5], out=out, ysmooth=mine[:, :T])
    f2, y2, _, _ = bank.interpolate(dev, [0.0, 0.5])
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and ys.data_ptr() == mine.data_ptr()
    assert torch.equal(ys, y2) and torch.equal(fine, f2) and bool((mine[:, T:] == 12345.0).all())
    assert padding_untouched(torch, slab, out)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_identities_on_the_device(env, kern):
    """Plane phi = 0 and the returned ysmooth are smooth(); the last column of a plane is the forecast phi dt past the end, a_phi . x_end."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(4)
    L, T, fracs = 64, 3000, [0.0, 0.3, 0.75]
    bank, tbs, _ = bank_and_tables(streams, kern, L)
    _, Fs = pool_models(kern, L)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    Ty[:, T - 1] = 0.5
    dev = to_dev(torch, Ty, torch.float64, T)
    fine, ys, x, status = bank.interpolate(dev, fracs)
    ref, xs, _ = bank.smooth(dev)
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()
    assert int(status.abs().sum()) == 0
    assert rel_err_rows(n(fine[0]), n(ref)) <= 1e-11 and rel_err_rows(n(ys), n(ref)) <= 1e-11
    assert rel_err_rows(n(x), n(xs), floor=1e-3) <= 1e-11
    for k, phi in enumerate(fracs):
        end = np.array([(sl.expm(Fs[l] * phi * DT) @ n(x)[l])[0] for l in range(L)])
        assert rel_err_rows(n(fine[k])[:, T - 1:], end[:, None]) <= 1e-9, phi


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_scan_and_serial_paths_agree(env, kern):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(5)
    L, T = 64, 5000
    bank, tbs, _ = bank_and_tables(streams, kern, L)
    _, Fs = pool_models(kern, L)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, torch.float64, T)
    res = []
    for path in (0, 1):
        bank.set_option("interp_path", path)
        f, y, x, st = bank.interpolate(dev, FRACS3)
        res.append((f.clone().cpu().numpy(), y.clone().cpu().numpy(), x.clone().cpu().numpy()))
        assert not st.cpu().numpy().any()
    torch.cuda.synchronize()
    for k in range(3):
        assert rel_err_rows(res[0][0][k], res[1][0][k]) <= 1e-11
    assert rel_err_rows(res[0][1], res[1][1]) <= 1e-11
    assert rel_err_rows(res[0][2], res[1][2], floor=1e-3) <= 1e-11
    fine, ys, xe, _ = interp_np(tbs, Fs, DT, FRACS3, Ty)
    for path in (0, 1):
        assert max(rel_err_rows(res[path][0][k], fine[k]) for k in range(3)) <= FP64_TOL
        assert rel_err_rows(res[path][1], ys) <= FP64_TOL and rel_err_rows(res[path][2], xe, floor=1e-3) <= FP64_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_variances_match_numpy(env, kern):
    """1e-10 relative (test_tables_match_scipy's tolerance) over the POOL at VAR_INNER, the offsets where the fp64 reference itself is good to
    1e-11 (test_numpy_variance_rounding_error); var_edge_bound at VAR_EDGE, where it is not.  Measured on the device against numpy, worst of both models:
    1.0e-11 at VAR_INNER (Matern-5/2, (1.3, 0.8, 1e-6), offset 1/8); at VAR_EDGE 5.1e-10 (Matern-3/2, the same draw, offset 0.999; bound 2.7e-9) and
    4.4e-10 (Matern-5/2, bound 3.0e-8), 2.2e-10 at offset 1e-3, and below 1e-10 on every other draw."""
    torch, streams = env["torch"], env["streams"]
    L = len(POOL)
    bank, tbs, _ = bank_and_tables(streams, kern, L)
    _, Fs = pool_models(kern, L)
    fracs = VAR_INNER + VAR_EDGE
    var = bank.interp_variances(fracs)
    assert var.shape == (8, L)
    for k, phi in enumerate(fracs):
        for l in range(L):
            ref = interp_rows_np(tbs[l], Fs[l], DT, phi)[2]
            err, tol = abs(var[k, l] - ref) / ref, 1e-10 if phi in VAR_INNER else var_edge_bound(tbs[l], ref)
            print(f"{kern} offset {phi} draw {POOL[l]}: {err:.1e} (bound {tol:.1e})")
            assert err <= tol, (phi, l, var[k, l], ref)
    vs = bank.latent_variances()[1]
    v0 = bank.interp_variances([0.0])[0]                        # offset 0 is the smoother's own variance
    assert all(abs(v0[l] - vs[l]) / vs[l] <= var_edge_bound(tbs[l], vs[l]) for l in range(L)), (v0, vs)
    assert np.all(var >= v0 * (1 - 1e-7))                       # between the ticks the function is known no better than on them


@pytest.mark.gpu
def test_interior_is_the_gp_posterior_on_the_device(env):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(6)
    T, prm, ticks = 1500, (1.3, 0.7, 0.05), np.arange(500, 1001)
    bank, tbs, _ = bank_and_tables(streams, "Matern52", 1, pool=[prm])
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    fine, ys, _, _ = bank.interpolate(to_dev(torch, y[None, :], torch.float64, T), [0.5])
    torch.cuda.synchronize()
    mean, var = dense_refined(tbs[0], F_of("Matern52", DT, prm), DT, y, 2, ticks)
    assert np.max(np.abs(fine.cpu().numpy()[0, 0, ticks] - mean[1])) <= 1e-9
    assert np.max(np.abs(ys.cpu().numpy()[0, ticks] - mean[0])) <= 1e-9
    assert np.max(np.abs(bank.interp_variances([0.5])[0, 0] - var[1])) <= 1e-9


@pytest.mark.gpu
def test_stacked_model_returns_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    bank = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (4, 1)), kernel="Matern32x2")
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    out, ysm = torch.zeros_like(Ty), torch.zeros_like(Ty)
    fr = (C.c_double * 1)(0.5)
    var = np.zeros(4)
    rc = lib.moihgp_interp_stream(bank._h, 0, C.c_void_p(Ty.data_ptr()), 64, 64, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), fr, 1,
                                  C.c_void_p(ysm.data_ptr()), C.c_void_p(out.data_ptr()), 64, 4 * 64, None, None)
    assert rc == 3
    assert lib.moihgp_interp_variances(bank._h, fr, 1, var.ctypes.data_as(C.POINTER(C.c_double))) == 3
    with pytest.raises(MoihgpError):
        bank.interpolate(Ty, [0.5])


@pytest.mark.gpu
def test_bad_calls_launch_nothing(env):
    """rc 1 from the C entry for a bad count or offset, T = 0 writes the end state and the status words, an `out` over the input stream is refused."""
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    L, T = 4, 64
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    lib = bank._lib
    Ty = torch.zeros((L, T), dtype=torch.float64, device="cuda")
    x = torch.zeros((L, bank.d), dtype=torch.float64, device="cuda")
    out, ysm = torch.full_like(Ty, 7.0), torch.full_like(Ty, 7.0)
    var = np.zeros((9, L))

    def call(fr, K):
        return lib.moihgp_interp_stream(bank._h, 0, C.c_void_p(Ty.data_ptr()), T, T, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                        (C.c_double * len(fr))(*fr), K, C.c_void_p(ysm.data_ptr()), C.c_void_p(out.data_ptr()), T, L * T, None, None)
    for fr, K in (([0.5], 0), ([0.1] * 9, 9), ([1.0], 1), ([-0.1], 1), ([float("nan")], 1), ([float("inf")], 1)):
        assert call(fr, K) == 1, (fr, K)
        assert lib.moihgp_interp_variances(bank._h, (C.c_double * len(fr))(*fr), K, var.ctypes.data_as(C.POINTER(C.c_double))) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ysm == 7.0).all())
    assert lib.moihgp_set_option(bank._h, b"interp_path", 2) == 1
    x0 = torch.full((L, bank.d), 0.25, dtype=torch.float64, device="cuda")
    _, _, xe, status = bank.interpolate(Ty, [0.5], T=0, x_start=x0)
    torch.cuda.synchronize()
    assert torch.equal(xe, x0) and int(status.abs().sum()) == 0
    with pytest.raises(ValueError, match="must not overlap"):
        bank.interpolate(Ty, [0.5], out=Ty[None])
    both = torch.zeros((2, L, T), dtype=torch.float64, device="cuda")
    with pytest.raises(MoihgpError, match="must not overlap"):
        bank.interpolate(Ty, [0.5], out=both[:1], ysmooth=both[0])


@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
def test_failed_latent_gives_nan_rows_and_status_1(env, path):
    """A latent whose DARE cannot converge (NaN magnitude): status 1, NaN rows, end state and variances; the other latents are untouched."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(12)
    L, T, bad = 7, 2500, 3
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L)
    _, Fs = pool_models("Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("interp_path", path)
    Ty = synth(L, T, rng)
    fine, ys, x, status = bank.interpolate(to_dev(torch, Ty, torch.float64, T), FRACS3)
    torch.cuda.synchronize()
    st, got, gy, xg = status.cpu().numpy(), fine.cpu().numpy(), ys.cpu().numpy(), x.cpu().numpy()
    var = bank.interp_variances(FRACS3)
    assert st[bad] == 1 and np.all(np.isnan(got[:, bad])) and np.all(np.isnan(gy[bad])) and np.all(np.isnan(xg[bad])) and np.all(np.isnan(var[:, bad]))
    keep = [l for l in range(L) if l != bad]
    assert not st[keep].any() and np.all(np.isfinite(var[:, keep]))
    ref, yref, xref, _ = interp_np([tbs[l] for l in keep], [Fs[l] for l in keep], DT, FRACS3, Ty[keep])
    for k in range(3):
        assert rel_err_rows(got[k][keep], ref[k]) <= FP64_TOL
    assert rel_err_rows(gy[keep], yref) <= FP64_TOL
    assert rel_err_rows(xg[keep], xref, floor=1e-3) <= FP64_TOL


@pytest.mark.gpu
def test_calls_on_two_streams_keep_their_own_tables(env):
    """A call on a second stream right after one on the first, with other offsets: the second rewrites the handle's per-call tables only after the
    first has finished with them (the tables' event), so both match their references."""
    torch, streams = env["torch"], env["streams"]
    L, T = 256, 2065
    case = parity_case("Matern52", L, T)
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L)
    _, Fs = pool_models("Matern52", L)
    ref8 = interp_np(tbs, Fs, DT, FRACS8, case["Ty"], case["x0"])[0]
    case = dict(case, ref={"8": ref8, "3": case["ref"]["3"]})
    dev = to_dev(torch, case["Ty"], torch.float64, T)
    x_start = torch.from_numpy(case["x0"]).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = bank.interpolate(dev, FRACS8, x_start=x_start, stream=s1)
    b = bank.interpolate(dev, FRACS3, x_start=x_start, stream=s2)
    c = bank.interpolate(dev, FRACS8, x_start=x_start, stream=s2)
    torch.cuda.synchronize()
    for k in range(8):
        assert rel_err_rows(a[0][k].cpu().numpy(), case["ref"]["8"][k]) <= FP64_TOL
        assert torch.equal(a[0][k], c[0][k])
    for k in range(3):
        assert rel_err_rows(b[0][k].cpu().numpy(), case["ref"]["3"][k]) <= FP64_TOL


def _interp_outputs_np(gp, Y, kern, fracs):
    U, S, igp, Ty = project_np(gp, Y, nan_below_L=True)
    L = len(igp)
    tbs = [tables(kern, DT, igp[l]) for l in range(L)]
    fine, ys, _, var = interp_np(tbs, [F_of(kern, DT, igp[l]) for l in range(L)], DT, fracs, Ty)
    mix = U * np.sqrt(S)
    return (np.einsum("ml,klt->ktm", mix, fine), (mix @ ys).T, (S[None, :] * var) @ (U ** 2).T,
            (U ** 2) @ (S * np.array([t["var_s"] for t in tbs])))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("missing", [False, True])
def test_interpolate_and_upsample_outputs_end_to_end(env, kern, missing):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(27)
    M, L, T, factor = 12, 4, 600, 4
    fracs = [j / factor for j in range(1, factor)]
    params, Y = end_to_end_inputs(rng, M, L, T, missing)
    gp = MOIHGP(DT, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yd = torch.from_numpy(Y).cuda()
    Yfine, Ys, var_fine, var_Y = streams.interpolate_outputs(gp, Yd, fracs)
    Yup, var_up = streams.upsample_outputs(gp, Yd, factor)
    Ysm, var_sm = streams.smooth_outputs(gp, Yd)
    torch.cuda.synchronize()
    ref, yref, vref, vyref = _interp_outputs_np(gp, Y, kern, fracs)
    assert tuple(Yfine.shape) == (3, T, M) and tuple(Ys.shape) == (T, M) and var_fine.shape == (3, M) and var_Y.shape == (M,)
    assert tuple(Yup.shape) == ((T - 1) * factor + 1, M) and var_up.shape == (factor, M)
    for k in range(3):
        assert rel_err(Yfine[k].cpu().numpy(), ref[k]) <= 1e-8, (k, rel_err(Yfine[k].cpu().numpy(), ref[k]))
    assert rel_err(Ys.cpu().numpy(), yref) <= 1e-8
    assert rel_err(var_fine, vref) <= 1e-8 and rel_err(var_Y, vyref) <= 1e-8
    up = Yup.cpu().numpy()
    assert rel_err(up[::factor], Ysm.cpu().numpy()) <= 1e-11
    for j in range(1, factor):
        assert np.array_equal(up[j::factor], Yfine[j - 1].cpu().numpy()[:T - 1])
    assert np.array_equal(var_up[0], var_Y) and np.array_equal(var_up[1:], var_fine) and rel_err(var_up[0], var_sm) <= 1e-11
    for bad in (1, 10, 2.0, True):
        with pytest.raises(ValueError):
            streams.upsample_outputs(gp, Yd, bad)


@pytest.mark.gpu
def test_interpolate_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(14)
    M, L, T = 8, 3, 100
    gp = MOIHGP(DT, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.interpolate_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda(), [0.5])


# ------------------------------------------------------------------------------------------------ C++ (predictBetween)
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_predict_between_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(28)
    M, L, T, frac = 12, 4, 300, 0.375
    params, Y = end_to_end_inputs(rng, M, L, T, True)
    exe = cxx_test_binary(hip_built, "interp_test")

    def run(fr):
        inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {fr!r} {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
        return cxx_run(exe, inp)
    got = cxx_rows(run(frac))
    gp = MOIHGP(DT, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yfine, _, _, _ = streams.interpolate_outputs(gp, torch.from_numpy(Y).cuda(), [frac])
    torch.cuda.synchronize()
    assert got.shape == (T, M)
    assert rel_err(got, Yfine[0].cpu().numpy()) <= 1e-9
    assert run(1.0) == ["invalid_argument"] and run(-0.25) == ["invalid_argument"]
