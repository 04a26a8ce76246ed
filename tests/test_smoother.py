"""Steady-state RTS smoother (include/moihgp.h moihgp_smooth_stream): the numpy definition the GPU is held to, checked against the textbook
RTS loop, the dense GP posterior and scipy's Kalman DARE (CPU), then the library's tables and sweeps against it (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rel_err, rel_err_rows
from parity_support import synth
from stream_reference import smooth_np, smooth_outputs_np, tables
from stream_support import (CASES, KMAP, POOL, assert_declared, assert_exported, bank_and_tables, cxx_fmt, cxx_rows, cxx_run, cxx_test_binary,
                            end_to_end_inputs, env, to_dev)  # noqa: F401  (env: the module's fixture)

SMOOTH_SYMBOLS = ("moihgp_smooth_stream", "moihgp_get_smoother", "moihgp_latent_variances")


# ------------------------------------------------------------------------------------------------ cross-checks of the numpy definition
def rts_textbook(tb, y):
    A, K, G = tb["A"], tb["K"], tb["G"]
    x = np.zeros(A.shape[0]); xf = []
    for yt in y:
        xp = A @ x
        x = xp if np.isnan(yt) else xp + K * (yt - xp[0])
        xf.append(x)
    xs = xf[-1]; out = [xs[0]]
    for t in range(len(y) - 2, -1, -1):
        xs = xf[t] + G @ (xs - A @ xf[t])
        out.append(xs[0])
    return np.array(out[::-1])


def dense_posterior(tb, y):
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    T = len(y)
    c = np.zeros(T); M = np.eye(A.shape[0])
    for k in range(T):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    i = np.arange(T)
    Cm = c[np.abs(i[:, None] - i[None, :])]
    Kd = Cm + R * np.eye(T)
    return Cm @ np.linalg.solve(Kd, y), np.diag(Cm - Cm @ np.linalg.solve(Kd, Cm))


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_smoother():
    assert_declared(SMOOTH_SYMBOLS)


def test_library_exports_the_smoother(hip_built):
    assert_exported(hip_built, SMOOTH_SYMBOLS)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_smoother_is_the_rts_smoother(kern):
    rng = np.random.default_rng(1)
    tb = tables(kern, 0.1, [1.3, 0.7, 0.05])
    y = np.sin(0.03 * np.arange(1500)) + 0.2 * rng.standard_normal(1500)
    y[[0, 3, 700, 701, 702, 1499]] = np.nan
    ys, _ = smooth_np([tb], y[None, :])
    assert np.max(np.abs(ys[0] - rts_textbook(tb, y))) <= 1e-12 * np.max(np.abs(ys))


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_smoother_interior_is_the_gp_posterior(kern):
    rng = np.random.default_rng(2)
    tb = tables(kern, 0.1, [1.3, 0.7, 0.05])
    y = np.sin(0.03 * np.arange(1500)) + 0.2 * rng.standard_normal(1500)
    mean, var = dense_posterior(tb, y)
    ys, _ = smooth_np([tb], y[None, :])
    assert np.max(np.abs(ys[0] - mean)[500:1000]) <= 1e-10
    assert np.max(np.abs(var[500:1000] - tb["var_s"])) <= 1e-9


def test_smoother_gain_is_contractive_over_the_learners_box():
    """rho(G) < 1 with the Kalman DARE over the learners' parameter box (moihgp_regression.h: 1e-4 .. 1e2); draws where scipy's DARE solver
    fails (near-singular Q at extreme lengthscales) are skipped -- on the device they are what status = 1 is for."""
    rng = np.random.default_rng(3)
    worst, used = 0.0, 0
    for i in range(400):
        kern = ("Matern32", "Matern52")[i % 2]
        dt = (1e-3, 1e-2, 0.1, 1.0)[(i // 2) % 4]
        tb = tables(kern, dt, 10.0 ** rng.uniform(-4, 2, 3))
        if tb is None:
            continue
        used += 1
        worst = max(worst, float(np.max(np.abs(np.linalg.eigvals(tb["G"])))))
    assert used >= 300 and worst < 1.0, (used, worst)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_tables_match_scipy(env, kern):
    bank, tbs, _ = bank_and_tables(env["streams"], kern, 8)
    vf, vs = bank.latent_variances()
    for l in range(8):
        got, ref = bank.smoother(l), tbs[l]
        for k in ("P", "K", "G", "Ps"):
            assert rel_err(got[k], ref[k]) <= 1e-10, (l, k, rel_err(got[k], ref[k]))
        assert abs(got["var_smoothed"] - ref["var_s"]) <= 1e-10 * ref["var_s"] and abs(vs[l] - ref["var_s"]) <= 1e-10 * ref["var_s"]
        assert abs(got["var_filtered"] - ref["var_f"]) <= 1e-10 * ref["var_f"] and abs(vf[l] - ref["var_f"]) <= 1e-10 * ref["var_f"]


@pytest.mark.gpu
def test_smooth_after_update_uses_the_new_parameters(env):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(4)
    L, T = 7, 1000
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L)
    Ty = synth(L, T, rng)
    y1, _, _ = bank.smooth(to_dev(torch, Ty, torch.float64, T))
    torch.cuda.synchronize()
    assert rel_err(y1.cpu().numpy(), smooth_np(tbs, Ty)[0]) <= 1e-9
    pool2 = [(p[0] * 1.5, p[1] * 0.7, p[2] * 2.0) for p in POOL]
    prm2 = np.array([pool2[l % len(pool2)] for l in range(L)])
    bank.update(prm2)
    y2, _, _ = bank.smooth(to_dev(torch, Ty, torch.float64, T))
    torch.cuda.synchronize()
    tbs2 = [tables("Matern52", 0.1, pool2[l % len(pool2)]) for l in range(L)]
    assert rel_err(y2.cpu().numpy(), smooth_np(tbs2, Ty)[0]) <= 1e-9


@pytest.mark.gpu
def test_stacked_model_returns_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    bank = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (4, 1)), kernel="Matern32x2")
    lib = bank._lib
    Ty = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    x = torch.zeros((4, bank.d), dtype=torch.float64, device="cuda")
    ys = torch.zeros_like(Ty)
    rc = lib.moihgp_smooth_stream(bank._h, 0, C.c_void_p(Ty.data_ptr()), 64, 64, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                  C.c_void_p(ys.data_ptr()), 64, None, None)
    assert rc == 3
    assert lib.moihgp_latent_variances(bank._h, None, None) == 3
    with pytest.raises(MoihgpError):
        bank.smooth(Ty)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("L,T", CASES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_smooth_parity(env, kern, L, T, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(L * 100003 + T)
    bank, tbs, _ = bank_and_tables(streams, kern, L)
    Ty = synth(L, T, rng)
    if T >= 63:   # missing ticks at the two ends, a long run, and 1 % scattered
        Ty[:, 0] = np.nan; Ty[:, T - 1] = np.nan
        Ty[::3, T // 3:T // 3 + min(300, T // 4)] = np.nan
        Ty[rng.random((L, T)) < 0.01] = np.nan
    if tdt == torch.float32:
        Ty = Ty.astype(np.float32).astype(np.float64)
    x0 = 0.1 * rng.standard_normal((L, bank.d))
    ref, xref = smooth_np(tbs, Ty, x0)
    x_start = torch.from_numpy(x0).to(tdt).cuda()
    x = torch.empty_like(x_start)
    out = torch.full((L, (T + 3) // 4 * 4 + 8), float("nan"), dtype=tdt, device="cuda")   # ld_out != ld_in
    ys, x, status = bank.smooth(to_dev(torch, Ty, tdt, T), x=x, x_start=x_start, ysmooth=out[:, :T])
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    got = ys.double().cpu().numpy()
    if dtype == "f64":
        assert rel_err_rows(got, ref) <= 1e-9, rel_err_rows(got, ref)
        assert rel_err_rows(x.cpu().numpy(), xref, floor=1e-3) <= 1e-9
    else:
        assert rel_err_rows(got, ref) <= 1e-3, rel_err_rows(got, ref)
        assert rel_err_rows(x.double().cpu().numpy(), xref, floor=1e-3) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_scan_and_serial_paths_agree(env, kern):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(5)
    L, T = 64, 5000
    bank, tbs, _ = bank_and_tables(streams, kern, L)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, torch.float64, T)
    bank.set_option("smoother_path", 0)
    y0, x0, _ = bank.smooth(dev)
    y0 = y0.clone(); x0 = x0.clone()
    bank.set_option("smoother_path", 1)
    y1, x1, _ = bank.smooth(dev)
    torch.cuda.synchronize()
    assert rel_err_rows(y0.cpu().numpy(), y1.cpu().numpy()) <= 1e-11
    assert rel_err_rows(x0.cpu().numpy(), x1.cpu().numpy(), floor=1e-3) <= 1e-11
    assert rel_err_rows(y1.cpu().numpy(), smooth_np(tbs, Ty)[0]) <= 1e-9


@pytest.mark.gpu
def test_interior_is_the_gp_posterior_on_the_device(env):
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(6)
    T = 1500
    bank, tbs, _ = bank_and_tables(streams, "Matern52", 1, pool=[(1.3, 0.7, 0.05)])
    y = np.sin(0.03 * np.arange(T)) + 0.2 * rng.standard_normal(T)
    ys, _, _ = bank.smooth(to_dev(torch, y[None, :], torch.float64, T))
    torch.cuda.synchronize()
    mean, var = dense_posterior(tbs[0], y)
    assert np.max(np.abs(ys.cpu().numpy()[0] - mean)[500:1000]) <= 1e-9
    assert abs(bank.smoother(0)["var_smoothed"] - var[750]) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("missing", [False, True])
def test_smooth_outputs_end_to_end(env, missing):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(7)
    M, L, T = 64, 16, 2000
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    params, Y = end_to_end_inputs(rng, M, L, T, missing)
    gp.update(params)
    Ys, var = streams.smooth_outputs(gp, torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    ref, vref = smooth_outputs_np(gp, Y, "Matern52")
    assert rel_err(Ys.T.cpu().numpy(), ref) <= 1e-9
    assert rel_err(var, vref) <= 1e-10


@pytest.mark.gpu
def test_full_size_c3_fp32_sampled(env):
    """C3's shape: 4096 latents x 10^4 ticks, Matern-5/2, fp32; 64 sampled latents against fp64 numpy."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(8)
    L, T = 4096, 10000
    pool = [tuple(p) for p in np.column_stack([rng.uniform(0.5, 2, 32), rng.uniform(0.5, 2, 32), rng.uniform(0.02, 0.3, 32)])]
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L, pool=pool)
    Ty = torch.randn((L, T), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    ys, _, status = bank.smooth(Ty)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    idx = np.sort(rng.choice(L, 64, replace=False))
    Tn = Ty[idx].double().cpu().numpy()
    ref, _ = smooth_np([tbs[i] for i in idx], Tn)
    assert rel_err_rows(ys[idx].double().cpu().numpy(), ref) <= 1e-3


# ------------------------------------------------------------------------------------------------ C++ (predictSmoothed)
def test_cxx_predict_smoothed_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "smoother_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_predict_smoothed_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    rng = np.random.default_rng(10)
    M, L, T = 12, 4, 300
    params, Y = end_to_end_inputs(rng, M, L, T, True)
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
    out = cxx_run(cxx_test_binary(hip_built, "smoother_test"), inp)
    got = cxx_rows(out)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Ys, _ = streams.smooth_outputs(gp, torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    assert got.shape == (T, M)
    assert rel_err(got, Ys.cpu().numpy()) <= 1e-12


# ------------------------------------------------------------------------------------------------ status and fallback paths
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_status_zero_wherever_scipy_solves_the_dare(env, kern):
    """A few thousand draws over the learners' box (1e-4 .. 1e2, four dt): the device DARE (doubling + Newton refinement) converges wherever
    scipy's does; and on the bench's own draw (Matern-5/2, dt 0.1, [0.5, 2] x [0.5, 2] x [0.02, 0.3]) for every latent."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(11)
    draws = []
    for dt in (1e-3, 1e-2, 0.1, 1.0):
        draws.append((dt, 10.0 ** rng.uniform(-4, 2, (512, 3))))
    if kern == "Matern52":
        r0 = np.random.default_rng(0)
        draws.append((0.1, np.column_stack([r0.uniform(0.5, 2, 4096), r0.uniform(0.5, 2, 4096), r0.uniform(0.02, 0.3, 4096)])))
    for dt, prm in draws:
        bank = streams.LatentBank(dt, prm, kernel=KMAP[kern])
        T = 8
        _, _, status = bank.smooth(torch.zeros((prm.shape[0], T), dtype=torch.float64, device="cuda"))
        st = status.cpu().numpy()
        solvable = np.array([tables(kern, dt, p) is not None for p in prm])
        bad = np.nonzero((st != 0) & solvable)[0]
        assert bad.size == 0, (dt, bad[:8], prm[bad[:8]])
        if dt == 0.1 and prm.shape[0] == 4096:
            assert not st.any()


@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
def test_failed_latent_gives_nan_row_and_status_1(env, path):
    """A latent whose DARE cannot converge (NaN magnitude): status 1, NaN row and end state; the other latents are untouched."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(12)
    L, T, bad = 7, 2500, 3
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("smoother_path", path)
    Ty = synth(L, T, rng)
    ys, x, status = bank.smooth(to_dev(torch, Ty, torch.float64, T))
    torch.cuda.synchronize()
    st, got, xg = status.cpu().numpy(), ys.cpu().numpy(), x.cpu().numpy()
    assert st[bad] == 1 and np.all(np.isnan(got[bad])) and np.all(np.isnan(xg[bad]))
    keep = [l for l in range(L) if l != bad]
    assert not st[keep].any()
    ref, xref = smooth_np([tbs[l] for l in keep], Ty[keep])
    assert rel_err_rows(got[keep], ref) <= 1e-9
    assert rel_err_rows(xg[keep], xref, floor=1e-3) <= 1e-9


@pytest.mark.gpu
def test_growth_bound_fallback(env):
    """Matern-5/2 with lengthscale 0.01 at dt 0.01: powers of G / A - K H A up to 32 reach ~4e4 in the inf-norm, above the scan kernels'
    growth bound, so the automatic path walks that latent serially.  It matches numpy and the all-serial path; the other latents take the scan."""
    torch, streams = env["torch"], env["streams"]
    rng = np.random.default_rng(13)
    pool = [(1.0, 0.01, 0.01), (1.0, 1.0, 0.1), (0.7, 0.5, 0.05), (1.0, 0.03, 1e-4)]
    L, T = 8, 3000
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L, dt=0.01, pool=pool)
    t = tbs[0]
    G, F = t["G"], t["A"] - np.outer(t["K"], t["A"][0])
    assert max(np.abs(np.linalg.matrix_power(M, k)).sum(1).max() for M in (G, F) for k in range(1, 33)) > 1e4   # the fallback is reached
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.01] = np.nan
    dev = to_dev(torch, Ty, torch.float64, T)
    bank.set_option("smoother_path", -1)
    ya, xa, sa = bank.smooth(dev)
    ya = ya.clone(); xa = xa.clone()
    bank.set_option("smoother_path", 1)
    ys, xs, _ = bank.smooth(dev)
    torch.cuda.synchronize()
    assert not sa.cpu().numpy().any()
    # the sweeps against numpy on the device's own tables (at lengthscale 0.01 the state's scales span ~9 decades, and scipy's and the device's
    # DARE solutions agree to ~1e-8 only; the tables themselves are checked elsewhere on ordinary parameters)
    dtb = [dict(A=bank.latent(l)["A"], **{k: v for k, v in bank.smoother(l).items() if k in ("K", "G")}) for l in range(L)]
    ref, _ = smooth_np(dtb, Ty)
    assert rel_err_rows(ya.cpu().numpy(), ref) <= 1e-9
    assert rel_err_rows(ya.cpu().numpy(), smooth_np(tbs, Ty)[0]) <= 1e-7
    assert np.array_equal(ya.cpu().numpy()[0::4], ys.cpu().numpy()[0::4])       # the fallback latents: the serial walk itself
    assert np.array_equal(xa.cpu().numpy()[0::4], xs.cpu().numpy()[0::4])


@pytest.mark.gpu
def test_smooth_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(14)
    M, L, T = 8, 3, 100
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.smooth_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda())
