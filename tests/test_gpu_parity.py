"""GPU suite (-m gpu): the HIP path, called through the C ABI (ctypes -> libmoihgp.so), against the CPU
oracle on the same seeded inputs, the committed golden vectors, and size-independent properties at
BASELINE.json's full sizes.

Tolerances (BASELINE.json north_star): 1e-6 relative for fp64, 1e-3 for fp32 on filtered means and NLL.
The asserts below use tighter bars where the arithmetic allows, and say so."""
import re
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, rel_err_rows
from parity_support import FP32_TOL, FP64_TIGHT, FP64_TOL, KMAP, STACKED, env, synth, synth_params, synth_params_stacked, to_dev  # noqa: F401  (env: fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ A7
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_stationary_matrices_vs_golden(env, kern):
    g = load_golden(f"stationary_{kern}.npz")
    worst, seen = 0.0, 0
    for dt in np.unique(g["dt"]):                          # one bank per time step of the file: every row is compared
        same_dt = g["dt"] == dt
        bank = env["streams"].LatentBank(float(dt), g["params"][same_dt], kernel=KMAP[kern])
        for j, i in enumerate(np.nonzero(same_dt)[0]):
            lat = bank.latent(j)
            for k in ("A", "K", "HA", "AKHA", "dA", "dS", "dK", "dAKHA", "HdA"):
                ref = g[k][i]
                if np.max(np.abs(ref)) == 0:
                    assert np.max(np.abs(lat[k])) == 0
                else:
                    e = rel_err(lat[k], ref); worst = max(worst, e)
                    assert e < FP64_TIGHT, (k, i, e)
            assert abs(lat["S"] - g["S"][i]) / g["S"][i] < FP64_TIGHT
            assert lat["iters"] == list(g["iters"][i])     # DARE / DLyap iteration counts (utils/dare.h)
            seen += 1
    assert seen == len(g["dt"])
    print(f"stationary {kern}: worst rel err {worst:.2e}")


# ------------------------------------------------------------------------------------------ A1-A6, A8 per-tick ABI
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("ML", [(2, 1), (4, 2), (6, 6), (8, 4)])
def test_reference_abi_vs_golden(env, kern, ML):
    M, L = ML
    g = load_golden(f"moihgp_{kern}_M{M}_L{L}.npz")
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    assert gp.num_param == M * L + L + 1 + 3 * L and gp.num_igp_param == 3 and gp.igp_dim == (2 if kern == "Matern32" else 3)
    gp.update(g["params_in"])
    assert rel_err(gp.params, g["params_out"]) < FP64_TIGHT
    a = gp.step(g["x"], g["y"], g["dx"])
    assert rel_err(a[0], g["s1_xnew"]) < FP64_TIGHT and rel_err(a[1], g["s1_yhat"]) < FP64_TIGHT and rel_err(a[2], g["s1_dxnew"]) < FP64_TIGHT
    b = gp.step_no_yhat(g["x"], g["y"], g["dx"])
    assert rel_err(b[0], g["s1_xnew"]) < FP64_TIGHT and rel_err(b[1], g["s1_dxnew"]) < FP64_TIGHT
    a = gp.step(g["x"], g["y"])
    assert rel_err(a[0], g["s3_xnew"]) < FP64_TIGHT and rel_err(a[1], g["s3_yhat"]) < FP64_TIGHT
    a = gp.step(g["x"])
    assert rel_err(a[0], g["s4_xnew"]) < FP64_TIGHT and rel_err(a[1], g["s4_yhat"]) < FP64_TIGHT
    assert abs(gp.negLogLikelihood(g["x"], g["y"]) - g["lik2"]) < FP64_TIGHT * abs(g["lik2"])
    l1, g1 = gp.negLogLikelihood(g["x"], g["y"], g["dx"])
    assert abs(l1 - g["lik1"]) < FP64_TIGHT * abs(g["lik1"])
    assert rel_err(g1, g["grad"]) < 1e-8     # closed-form U-gradient vs the literal SVD loop of the golden
    if "y_missing" in g:                      # least-squares projection over observed rows, moihgp.h:167-178
        a = gp.step(g["x"], g["y_missing"])
        assert rel_err(a[0], g["m3_xnew"]) < FP64_TIGHT and rel_err(a[1], g["m3_yhat"]) < FP64_TIGHT
        assert np.isnan(gp.negLogLikelihood(g["x"], g["y_missing"]))   # moihgp.h:651 does not guard NaN


# ------------------------------------------------------------------------------------------ A6: the `threading` flag is observable
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("ML", [(2, 1), (4, 2), (6, 6), (8, 4), (200, 150)])       # (200, 150): beyond the fused one-workgroup kernels
def test_lik1_follows_the_threading_flag(env, kern, ML):
    """moihgp.h:565-607: the gradient overload of negLogLikelihood adds the per-latent losses sum_l 1/2 (v_l^2/S_l + log S_l)
    (A4, ihgp.h:204-209) only in its threaded branch (:590); the serial branch (:597-607) drops them.  threading=False is the
    default everywhere (pywrapper.py:12) and is forced for L < 2 (:128-135).  So:
        lik1(threading=False) == lik2 - sum_l A4      lik1(threading=True) == lik2      gradient identical."""
    M, L = ML
    rng = np.random.default_rng(17 * M + L)
    if M <= 8:
        g = load_golden(f"moihgp_{kern}_M{M}_L{L}.npz")
        params, x, y, dx = g["params_in"], g["x"], g["y"], g["dx"]
    else:
        d = 2 if kern == "Matern32" else 3
        params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
        x, y, dx = rng.standard_normal((L, d)), rng.standard_normal(M), rng.standard_normal((L, 3, d))
    off = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern]); off.update(params)                      # default: threading off
    on = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern], threading=True); on.update(params)
    assert env["lib"].moihgp_get_threading(off.handle) == 0 and env["lib"].moihgp_get_threading(on.handle) == (1 if L >= 2 else 0)
    ref_off = env["cref"].GP(0.1, M, L, kern); ref_off.update(params); ref_off.set_literal_ugrad(0)
    ref_on = env["cref"].GP(0.1, M, L, kern, threading=True); ref_on.update(params); ref_on.set_literal_ugrad(0)
    lik2 = off.negLogLikelihood(x, y)
    assert abs(on.negLogLikelihood(x, y) - lik2) <= 1e-15 * abs(lik2)                         # lik2 (:654-686) adds them in both branches
    l_off, g_off = off.negLogLikelihood(x, y, dx)
    l_on, g_on = on.negLogLikelihood(x, y, dx)
    assert np.array_equal(g_off, g_on)
    # sum_l A4 from the oracle's per-latent function on the projected observation
    Ty = ref_off.project(y)
    sum_a4 = sum(env["cref"].lib().orc_ihgp_nll(ref_off.latent(l), x[l].ctypes.data_as(env["cref"]._dp), float(Ty[l]), None, None) for l in range(L))
    scale = max(abs(lik2), abs(sum_a4))
    if L >= 2:
        assert abs(l_on - lik2) < FP64_TIGHT * scale
        assert abs(l_off - (lik2 - sum_a4)) < FP64_TIGHT * scale
        assert abs(sum_a4) > 1e-3 * scale                      # the two values really differ
    else:
        assert l_on == l_off                                   # :128-135
    assert abs(l_off - ref_off.negLogLikelihood(x, y, dx)[0]) < FP64_TIGHT * scale
    assert abs(l_on - ref_on.negLogLikelihood(x, y, dx)[0]) < FP64_TIGHT * scale
    if M <= 8:
        assert abs(l_off - g["lik1"]) < FP64_TIGHT * scale and abs(l_on - g["lik1_threaded"]) < FP64_TIGHT * scale
    # the windowed objective sums what lik1 returns per tick, so it follows the flag too
    W = 6
    Y = 0.5 * rng.standard_normal((W, M))
    for gp, ref in ((off, ref_off), (on, ref_on)):
        loss, grad, _, _ = gp.window_objective(Y, x, dx)
        grad = grad.copy()
        xr, dxr, lref, gref = x, dx, 0.0, np.zeros(gp.num_param)
        for t in range(W):
            l1, g1 = ref.negLogLikelihood(xr, Y[t], dxr)
            xr, _, dxr = ref.step(xr, Y[t], dxr)
            lref += l1; gref += g1
        assert abs(loss - lref) < 1e-9 * max(abs(lref), scale) and rel_err(grad, gref) < 1e-8
    # the additive setter applies the same L < 2 override
    env["lib"].moihgp_set_threading(off.handle, 1)
    assert env["lib"].moihgp_get_threading(off.handle) == (1 if L >= 2 else 0)
    assert abs(off.negLogLikelihood(x, y, dx)[0] - l_on) <= 1e-15 * scale


def test_lik1_full_loss_opt_in(env, monkeypatch):
    """MOIHGP_LIK1_FULL_LOSS=1 (read at construction): the summed form regardless of the flag."""
    g = load_golden("moihgp_Matern32_M8_L4.npz")
    monkeypatch.setenv("MOIHGP_LIK1_FULL_LOSS", "1")
    gp = env["MOIHGP"](0.1, 8, 4, kernel="Matern32"); gp.update(g["params_in"])
    monkeypatch.delenv("MOIHGP_LIK1_FULL_LOSS")
    l1, g1 = gp.negLogLikelihood(g["x"], g["y"], g["dx"])
    assert abs(l1 - g["lik1_threaded"]) < FP64_TIGHT * abs(g["lik1_threaded"]) and rel_err(g1, g["grad"]) < 1e-8


@pytest.mark.parametrize("kern,M,L", [("Matern32", 64, 32), ("Matern52", 96, 96), ("Matern52", 300, 40)])
def test_reference_abi_vs_oracle_larger(env, kern, M, L):
    rng = np.random.default_rng(M * 1000 + L)
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    ref = env["cref"].GP(0.1, M, L, kern)
    ref.set_literal_ugrad(0)
    d, P = gp.igp_dim, 3
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
    gp.update(params); ref.update(params)
    assert rel_err(gp.params, ref.params) < FP64_TIGHT
    x, dx = rng.standard_normal((L, d)), rng.standard_normal((L, P, d))
    for _ in range(3):                        # a short closed loop: feed states forward like the callers do
        y = rng.standard_normal(M)
        l1, g1 = gp.negLogLikelihood(x, y, dx); l2, g2 = ref.negLogLikelihood(x, y, dx)
        assert abs(l1 - l2) < FP64_TIGHT * abs(l2) and rel_err(g1, g2) < FP64_TIGHT
        a = gp.step(x, y, dx); b = ref.step(x, y, dx)
        for u, v in zip(a, b):
            assert rel_err(u, v) < FP64_TIGHT
        x, dx = a[0], a[2]
    ym = y.copy(); ym[rng.choice(M, size=max(1, (M - L) // 2), replace=False)] = np.nan
    if M > L:
        a = gp.step(x, ym); b = ref.step(x, ym)
        assert rel_err(a[0], b[0]) < 1e-8 and rel_err(a[1], b[1]) < 1e-8


def test_gp52_alias_and_ctor_state(env):
    # wrapper.cpp:22: GP52 is a typedef of the Matern-3/2 model; kept by default
    gp = env["MOIHGP"](0.1, 5, 2, kernel="Matern52")
    assert gp.igp_dim == 2
    p = gp.params
    M, L = 5, 2
    U = p[:M * L].reshape(M, L)
    assert np.max(np.abs(U.T @ U - np.eye(L))) < 1e-13 and np.max(np.abs(U - np.eye(M, L))) < 0.02   # moihgp.h:103-125
    assert np.all(p[M * L:M * L + L] == 1.0) and p[M * L + L] == 1e-2                                  # moihgp.h:126-127
    assert np.allclose(p[M * L + L + 1:].reshape(L, 3), [1.0, 1.0, 0.1])                               # matern32ss.h:34-36
    gp.update(p)
    assert rel_err(gp.params, p) < 1e-13       # get_params / update round trip (checkpoint = params)


# ------------------------------------------------------------------------------------------ A1/A4 streams
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("tag", ["dense", "nan5"])
def test_stream_vs_golden_fp64(env, kern, tag):
    g = load_golden(f"stream_{kern}_{tag}.npz")
    bank = env["streams"].LatentBank(float(g["dt"]), g["params"], kernel=KMAP[kern])
    T = g["Ty"].shape[1]
    Ty = to_dev(g["Ty"], torch.float64)
    x = torch.from_numpy(g["x0"]).cuda()
    yhat, xT, nll = bank.filter(Ty, T=T, x=x)
    torch.cuda.synchronize()
    e = (rel_err_rows(yhat[:, :T].cpu().numpy(), g["yhat"]), rel_err(xT.cpu().numpy(), g["xT"]), rel_err(nll.cpu().numpy(), g["nll"]))
    print(f"stream fp64 {kern} {tag}: yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e}")
    assert max(e) < FP64_TIGHT and max(e) < FP64_TOL


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("tag", ["dense", "nan5"])
def test_stream_vs_golden_fp32(env, kern, tag):
    g = load_golden(f"stream_{kern}_{tag}.npz")
    bank = env["streams"].LatentBank(float(g["dt"]), g["params"], kernel=KMAP[kern])
    T = g["Ty"].shape[1]
    Ty = to_dev(g["Ty"], torch.float32)
    x = torch.from_numpy(g["x0"]).float().cuda()
    yhat, xT, nll = bank.filter(Ty, T=T, x=x)
    torch.cuda.synchronize()
    e = (rel_err_rows(yhat[:, :T].cpu().numpy(), g["yhat"]), rel_err(xT.cpu().numpy(), g["xT"]), rel_err(nll.cpu().numpy(), g["nll"]))
    print(f"stream fp32 {kern} {tag}: yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e}")
    assert max(e) < FP32_TOL


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T", [(1, 1), (3, 3), (4, 511), (5, 512), (67, 513), (2, 1023), (9, 1024), (6, 1025), (130, 2600), (3, 0)])
def test_stream_ragged_shapes_vs_oracle(env, dtype, L, T):
    rng = np.random.default_rng(1000 * L + T)
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern52ss")
    igps = env["cref"].ihgp_array("Matern52", 0.1, prm)
    Ty = synth(L, T, rng)
    x0 = 0.2 * rng.standard_normal((L, 3))
    if T == 0:
        Tyd = torch.zeros((L, 4), dtype=dtype, device="cuda")
        yhat, xT, nll = bank.filter(Tyd, T=0, x=torch.from_numpy(x0).to(dtype).cuda())
        torch.cuda.synchronize()
        assert rel_err(xT.cpu().numpy(), x0) < 1e-6 and float(nll.abs().sum()) == 0.0
        return
    o = env["cref"].filter_stream(igps, Ty, x0=x0)
    Tyd = to_dev(Ty, dtype)
    sentinel = 12345.0
    yh = torch.full_like(Tyd, sentinel)
    yhat, xT, nll = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), yhat=yh)
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    assert rel_err_rows(yhat[:, :T].cpu().numpy(), o["yhat"]) < tol
    assert rel_err(xT.cpu().numpy(), o["x"]) < tol
    assert rel_err(nll.cpu().numpy(), o["nll_per_latent"]) < tol
    # nll-only and yhat-only variants agree with the fused one
    _, x2, nll2 = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_yhat=False)
    yh3, x3, _ = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_nll=False)
    torch.cuda.synchronize()
    assert torch.equal(nll2, nll) and torch.equal(x2, xT) and torch.equal(x3, xT) and torch.equal(yh3[:, :T], yhat[:, :T])


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,nanf", [(513, 1, 0.0), (514, 15, 0.0), (520, 1024, 0.0), (517, 1025, 0.0), (600, 3000, 0.0), (515, 5007, 0.0),
                                      (530, 2048, 0.02), (519, 777, 0.3), (1025, 4100, 0.001)])
def test_many_latent_sweep_vs_oracle(env, kern, dtype, L, T, nanf):
    """More than 512 latents take the one-wavefront-per-latent sweep whose stream is staged by LDS-DMA (filter_dma_kernel, csrc/recursion.hip):
    a ring of 1 KB pieces with hand-counted waits, clamped pieces past the end of the stream, two forms of the ragged last segment (chunk-
    aligned and not: fp32 chunks are 16 ticks, fp64 8), the missing-data segment path on top of the swizzled ring.  Against the oracle on
    every latent: one tick, less than a chunk, exactly one segment, one tick more, many segments, dense and sparse gaps; nothing is written
    past tick T of a row; both layouts."""
    S = env["streams"]
    rng = np.random.default_rng(17 * L + T)
    prm = synth_params(L, rng)
    bank = S.LatentBank(0.1, prm, kernel=KMAP[kern])
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    Ty = synth(L, T, rng, nanf)
    x0 = 0.2 * rng.standard_normal((L, bank.d))
    o = env["cref"].filter_stream(igps, Ty, x0=x0, nthreads=8)
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6            # (the literal DARE leaves a few draws unstable)
    assert tame.sum() > L // 2
    Tyd = to_dev(Ty, dtype)
    sentinel = 12345.0
    yh = torch.full((L, Tyd.shape[1] + 8), sentinel, dtype=dtype, device="cuda")   # wider than the stream: the row's own tail must survive
    yhat, xT, nll = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), yhat=yh)
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    got = yhat[:, :T].cpu().numpy()
    assert rel_err_rows(np.nan_to_num(got[tame]), np.nan_to_num(o["yhat"][tame])) < tol
    assert rel_err(xT.cpu().numpy()[tame], o["x"][tame]) < tol
    assert rel_err(nll.cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol
    epv = 2 if dtype == torch.float64 else 4
    assert bool((yh[:, (T + epv - 1) // epv * epv:] == sentinel).all()), "the sweep wrote past the padded end of a row"
    # segment-major: ALWAYS the LDS-DMA sweep (series-major, Matern-5/2 at up to 1024 latents and 2 .. 8 segments takes the eight-wavefront team
    # kernel of recursion_x.hip instead): against the oracle in its own right, and bit for bit where both layouts run the same kernel
    yt, xb, nb = bank.filter_tiled(S.tile_stream(Tyd, T), T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    got_t = S.untile_stream(yt, T)[:, :T].cpu().numpy()
    assert rel_err_rows(np.nan_to_num(got_t[tame]), np.nan_to_num(o["yhat"][tame])) < tol
    assert rel_err(xb.cpu().numpy()[tame], o["x"][tame]) < tol and rel_err(nb.cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol
    if kern == "Matern32" or L > 1024:
        assert np.array_equal(got_t, got, equal_nan=True)
        assert np.array_equal(xb.cpu().numpy(), xT.cpu().numpy(), equal_nan=True) and np.array_equal(nb.cpu().numpy(), nll.cpu().numpy(), equal_nan=True)


def test_stream_all_missing_and_inf(env):
    rng = np.random.default_rng(4)
    L, T = 4, 1500
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern32")
    igps = env["cref"].ihgp_array("Matern32", 0.1, prm)
    Ty = synth(L, T, rng)
    Ty[0, :] = np.nan                 # a fully missing series: pure prediction x <- A x, NLL 0
    Ty[1, 100:1400] = np.nan          # a long gap spanning whole segments
    Ty[2, ::2] = np.nan               # every other tick missing
    x0 = rng.standard_normal((L, 2))
    o = env["cref"].filter_stream(igps, Ty, x0=x0)
    yhat, xT, nll = bank.filter(to_dev(Ty, torch.float64), T=T, x=torch.from_numpy(x0).cuda())
    torch.cuda.synchronize()
    assert rel_err(yhat[:, :T].cpu().numpy(), o["yhat"]) < FP64_TIGHT
    assert rel_err(nll.cpu().numpy(), o["nll_per_latent"]) < FP64_TIGHT and nll[0].item() == 0.0


def test_stream_argument_errors(env):
    bank = env["streams"].LatentBank(0.1, [[1, 1, 0.1]] * 4, kernel="Matern32")
    from multioutputihgp_amd import MoihgpError
    bad = torch.zeros((4, 10), dtype=torch.float32, device="cuda")      # ld = 10 is not a multiple of 4
    with pytest.raises(MoihgpError):
        bank.filter(bad, T=10)
    with pytest.raises(ValueError):
        bank.filter(torch.zeros((3, 12), dtype=torch.float32, device="cuda"))   # wrong L


# ------------------------------------------------------------------------------------------ full-size properties
@pytest.mark.parametrize("dtype,L,T", [(torch.float32, 4096, 10000), (torch.float64, 256, 10000), (torch.float64, 4096, 10000)])
def test_full_size_properties(env, dtype, L, T):
    """BASELINE configs C2/C3 shapes: checks that do not need a full-size oracle run --
    (1) a 64-latent subset against the oracle, (2) linearity of the filter, (3) slab consistency
    (one sweep == two sweeps carrying the state), (4) NLL additivity over slabs."""
    rng = np.random.default_rng(7)
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern52ss")
    Ty = synth(L, T, rng)
    tol = 1e-8 if dtype == torch.float64 else FP32_TOL
    Tyd = to_dev(Ty, dtype)
    yhat, xT, nll = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    sub = np.sort(rng.choice(L, size=64, replace=False))
    o = env["cref"].filter_stream(env["cref"].ihgp_array("Matern52", 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=4)
    e = (rel_err_rows(yhat[sub][:, :T].cpu().numpy(), o["yhat"]), rel_err(xT[sub].cpu().numpy(), o["x"]), rel_err(nll[sub].cpu().numpy(), o["nll_per_latent"]))
    print(f"full-size {dtype} L={L}: subset vs oracle yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e}")
    assert max(e) < (FP64_TOL if dtype == torch.float64 else FP32_TOL)
    # linearity (zero initial state): f(a y1 + b y2) = a f(y1) + b f(y2)
    Y2 = to_dev(synth(L, T, rng), dtype)
    f1 = yhat
    f2, _, _ = bank.filter(Y2, T=T, want_nll=False)
    f12, _, _ = bank.filter(2.0 * Tyd - 0.5 * Y2, T=T, want_nll=False)
    torch.cuda.synchronize()
    lin = (f12 - (2.0 * f1 - 0.5 * f2))[:, :T].abs().max().item() / f12[:, :T].abs().max().item()
    assert lin < (1e-11 if dtype == torch.float64 else 2e-5), lin
    # slab consistency + NLL additivity
    cut = 4096 + 4 * 37
    ya, xa, na = bank.filter(Tyd[:, :cut], T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:], T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    d1 = (torch.cat([ya[:, :cut], yb[:, :T - cut]], 1) - yhat[:, :T]).abs().max().item() / yhat[:, :T].abs().max().item()
    d2 = ((na + nb) - nll).abs().max().item() / nll.abs().max().item()
    d3 = (xb - xT).abs().max().item() / xT.abs().max().item()
    assert max(d1, d2, d3) < tol, (d1, d2, d3)


# ------------------------------------------------------------------------------------------ A2/A5 gradient sweep
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gradstream_vs_golden(env, kern, dtype):
    g = load_golden(f"gradstream_{kern}.npz")
    bank = env["streams"].LatentBank(float(g["dt"]), g["params"], kernel=KMAP[kern])
    T = g["Ty"].shape[1]
    r = bank.grad(to_dev(g["Ty"], dtype), T=T, x=torch.from_numpy(g["x0"]).to(dtype).cuda(),
                  dx=torch.from_numpy(g["dx0"]).to(dtype).cuda(), want_yhat=True)
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    assert rel_err_rows(r["yhat"][:, :T].cpu().numpy(), g["yhat"]) < tol
    assert rel_err(r["x"].cpu().numpy(), g["xT"]) < tol and rel_err(r["dx"].cpu().numpy(), g["dxT"]) < tol * 10
    assert rel_err(r["nll"].cpu().numpy(), g["nll"]) < tol and rel_err(r["grad"].cpu().numpy(), g["grad"]) < tol * 10


# ------------------------------------------------------------------------------------------ A3 projection over streams
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M,L,T", [(8, 4, 50), (100, 70, 333), (256, 256, 1000)])
def test_project_unproject_stream(env, dtype, M, L, T):
    rng = np.random.default_rng(M + L + T)
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
    gp.update(params)
    p = gp.params
    U = p[:M * L].reshape(M, L); S = p[M * L:M * L + L]
    Y = rng.standard_normal((T, M))
    Ty = env["streams"].project_stream(gp, torch.from_numpy(Y).to(dtype).cuda())
    ref = (Y @ U / np.sqrt(S)).T
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert rel_err(Ty[:, :T].cpu().numpy(), ref) < tol
    Yh = env["streams"].unproject_stream(gp, Ty, T)
    ref2 = (ref.T * np.sqrt(S)) @ U.T
    assert rel_err(Yh.cpu().numpy(), ref2) < tol * 10
    # per-tick ABI and stream path agree: project -> filter -> unproject over the stream equals
    # calling gp.step(x, y_t) tick by tick (the reference's caller loop, example.py:40-42)
    bank = env["streams"].LatentBank.from_handle(gp)
    yhat, xT, nll = bank.filter(Ty, T=T)
    Yhat_f = env["streams"].unproject_stream(gp, yhat, T)
    torch.cuda.synchronize()
    x = np.zeros((L, gp.igp_dim))
    nt = min(T, 20)
    for t in range(nt):
        x, yh = gp.step(x, Y[t])
        assert rel_err(yh, Yhat_f[t].cpu().numpy()) < (1e-10 if dtype == torch.float64 else 1e-4)


# ------------------------------------------------------------------------------------------ time split (small L)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,nan", [(3, 5000, 0.0), (16, 10000, 0.0), (7, 4097, 0.03), (256, 10000, 0.0), (5, 2047, 0.0), (9, 16384, 0.001), (4, 16000, 0.0),
                                     (6, 1025, 0.0), (5, 9000, 1.0)])
def test_time_split_matches_unsplit(env, dtype, L, T, nan, monkeypatch):
    """With few latents the filter splits each stream into slices handled by different wavefronts (slice
    affine maps + carry).  Results must equal the unsplit sweep to rounding, and the oracle."""
    rng = np.random.default_rng(L * 7 + T)
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern52ss")
    Ty = synth(L, T, rng, nan)
    x0 = 0.3 * rng.standard_normal((L, 3))
    o = env["cref"].filter_stream(env["cref"].ihgp_array("Matern52", 0.1, prm), Ty, x0=x0)
    Tyd = to_dev(Ty, dtype)
    res = {}
    for split in ("1", "0", "5"):                  # off, automatic (slices of uneven length: the same number of segments per SIMD), forced 5 equal slices
        bank.set_option("filter_split", int(split))        # per-handle hook (include/moihgp.h moihgp_set_option)
        yhat, xT, nll = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda())
        _, xT2, _ = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_yhat=False, want_nll=False)
        torch.cuda.synchronize()
        res[split] = (yhat[:, :T].cpu().numpy(), xT.cpu().numpy(), nll.cpu().numpy())
        tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
        assert rel_err_rows(res[split][0], o["yhat"]) < tol and rel_err(res[split][1], o["x"]) < tol
        assert rel_err(res[split][2], o["nll_per_latent"]) < tol
        assert rel_err(xT2.cpu().numpy(), o["x"]) < tol
    tight = 1e-11 if dtype == torch.float64 else 2e-4
    for split in ("0", "5"):
        assert rel_err(res[split][0], res["1"][0]) < tight and rel_err(res[split][2], res["1"][2]) < tight


# ------------------------------------------------------------------------------------------ A8: polar factor on the device
@pytest.mark.parametrize("M,L,noise", [(8, 4, 0.3), (100, 70, 0.2), (300, 300, 0.05), (1024, 512, 0.02), (64, 64, 2.0),
                                       (64, 16, 0.5), (128, 32, 0.2), (1000, 4, 1.0), (40, 20, 2.0), (5, 5, 0.4), (3, 1, 0.0),
                                       (140, 129, 0.2), (300, 257, 0.05)])     # the last two: odd L over more than one tile (scalar fetches, the mirror)
def test_polar_factor_device_vs_svd(env, M, L, noise, monkeypatch):
    """MOIHGP::update (moihgp.h:433-447) forms U = svdU svdV^T.  On the device it is Newton-Schulz: one workgroup in LDS for
    small matrices (M L <= 4096, L <= 32), MFMA GEMMs otherwise (MOIHGP_POLAR=gemm forces those)."""
    rng = np.random.default_rng(M + L)
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    A = np.eye(M, L) + noise * rng.standard_normal((M, L))
    params = np.concatenate([A.ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
    u, _, vt = np.linalg.svd(A, full_matrices=False)
    for mode in ("", "gemm"):
        if mode:
            monkeypatch.setenv("MOIHGP_POLAR", mode)
        gp.update(params)
        U = gp.params[:M * L].reshape(M, L)
        assert rel_err(U, u @ vt) < 1e-11, mode
        assert np.max(np.abs(U.T @ U - np.eye(L))) < 1e-12


@pytest.mark.parametrize("M,L", [(300, 300), (700, 260), (1024, 512)])
@pytest.mark.parametrize("shape", ["learner", "learner_many", "one_small", "dominant_orthogonal_to_ones", "wide"])
def test_polar_factor_spectra_with_outliers(env, M, L, shape, monkeypatch):
    """The polar factor (moihgp.h:433-447) for spectra that the plain Newton-Schulz iteration handles badly or wrongly:
      learner / learner_many: an orthonormal matrix whose singular values have drifted in a few (8 / 60) directions, one of them far
        (sigma_1 = 4.7): what the online learner hands to update() after some ticks (profiles/r04/learner_spectrum.log).  The outliers are
        deflated exactly (csrc/polar_deflate.hip) and the iteration finishes in <= 3 steps (nine without);
      one_small: an outlier BELOW 1 (sigma = 0.05);
      dominant_orthogonal_to_ones: sigma_1 = 3 along a right singular vector orthogonal to the all-ones vector, from which the power
        iteration for lambda_max starts: the scale must still put every singular value inside (0, sqrt 3);
      wide: singular values uniform in [0.5, 1.5]: nothing to deflate, the attempt is abandoned.
    Against LAPACK's svdU svdV^T, with MOIHGP_POLAR=gemm forcing the multi-kernel path for every size."""
    monkeypatch.setenv("MOIHGP_POLAR", "gemm")
    rng = np.random.default_rng(M * 7 + L + len(shape))
    Q1, _ = np.linalg.qr(rng.standard_normal((M, L))); Q2, _ = np.linalg.qr(rng.standard_normal((L, L)))
    sig = np.ones(L) + 3e-11 * rng.standard_normal(L)
    if shape == "learner":
        sig[:9] = [4.684, 1.2004, 1.081, 1.0364, 1.0213, 1.0125, 1.0075, 1.0036, 0.99947]
    elif shape == "learner_many":
        sig[:60] = np.concatenate([[4.684, 2.2], 1.0 + np.logspace(-0.5, -7, 58)])
    elif shape == "one_small":
        sig[0] = 0.05
    elif shape == "dominant_orthogonal_to_ones":
        v = np.zeros(L); v[0], v[1] = 1 / np.sqrt(2), -1 / np.sqrt(2)            # orthogonal to the all-ones start vector
        Q2, _ = np.linalg.qr(np.column_stack([v, rng.standard_normal((L, L - 1))]))
        sig = np.ones(L); sig[0] = 3.0
    else:
        sig = rng.uniform(0.5, 1.5, L)
    A = (Q1 * sig) @ Q2.T
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    params = np.concatenate([A.ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
    gp.update(params)
    U = gp.params[:M * L].reshape(M, L)
    its = env["lib"].moihgp_polar_iterations(gp.handle)
    u, _, vt = np.linalg.svd(A, full_matrices=False)
    assert np.max(np.abs(U.T @ U - np.eye(L))) < 1e-12
    assert rel_err(U, u @ vt) < 1e-10, (shape, its)
    if shape in ("learner", "one_small"):
        assert 0 < its <= 3, its
    # (the same without the deflation -- MOIHGP_POLAR_DEFLATE=0, read once per process -- runs in a child process of test_polar_factor.py:
    # test_plain_newton_schulz_on_the_same_spectra)


def test_polar_factor_rank_deficient_input_is_reported(env, capfd):
    gp = env["MOIHGP"](0.1, 6, 3, kernel="Matern32")
    p = gp.params.copy()
    A = np.ones((6, 3))                               # rank 1
    p[:18] = A.ravel()
    gp.update(p)
    assert np.all(np.isnan(gp.params[:18]))
    assert b"rank deficient" in env["lib"].moihgp_last_error()


# ------------------------------------------------------------------------------------------ A2/A5 scan-structured gradient sweep
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kern,L,T,nan", [("Matern52", 5, 16, 0.0), ("Matern32", 9, 128, 0.0), ("Matern52", 3, 129, 0.0),
                                         ("Matern52", 6, 1500, 0.0), ("Matern32", 4, 2600, 0.0), ("Matern52", 70, 1030, 0.0),
                                         ("Matern52", 8, 700, 0.01)])
def test_gradstream_vs_oracle(env, dtype, kern, L, T, nan):
    rng = np.random.default_rng(L * 31 + T)
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=KMAP[kern])
    d = bank.d
    Ty = synth(L, T, rng, nan)
    if nan:
        Ty[:L // 2] = np.nan_to_num(Ty[:L // 2], nan=0.1)        # half of the latents clean: mixes scan and fallback paths
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, 3, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=True)
    torch.cuda.synchronize()
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    assert rel_err_rows(r["yhat"][:, :T].cpu().numpy(), o["yhat"]) < tol
    assert rel_err(r["x"].cpu().numpy(), o["x"]) < tol and rel_err(r["dx"].cpu().numpy(), o["dx"]) < tol * 10
    assert rel_err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol
    assert rel_err(r["grad"].cpu().numpy(), o["grad"]) < tol * 10
    r2 = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=False)
    torch.cuda.synchronize()
    assert torch.equal(r2["grad"], r["grad"]) and torch.equal(r2["nll"], r["nll"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("T", [513, 1023, 1024, 1025, 2048, 2049, 3071])
def test_gradstream_segment_boundaries_of_the_long_stream_kernels(env, dtype, kern, T):
    """Streams one tick short of, exactly at and one tick past whole segments of the long-stream instantiations (512 ticks in fp64,
    1024 in fp32): full segments run the unrolled single replay, the ragged rest the rolled one, and the carried (x, dx) and the
    split gradient sums must join seamlessly."""
    L = 3
    rng = np.random.default_rng(T * 7 + (1 if kern == "Matern52" else 0))
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=KMAP[kern])
    d = bank.d
    Ty = synth(L, T, rng)
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, 3, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=True)
    torch.cuda.synchronize()
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    assert rel_err_rows(r["yhat"][:, :T].cpu().numpy(), o["yhat"]) < tol
    assert rel_err(r["x"].cpu().numpy(), o["x"]) < tol and rel_err(r["dx"].cpu().numpy(), o["dx"]) < tol * 10
    assert rel_err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol
    assert rel_err(r["grad"].cpu().numpy(), o["grad"]) < tol * 10


# ------------------------------------------------------------------------------------------ windowed objective in one call
@pytest.mark.parametrize("kern,M,L,W", [("Matern32", 6, 3, 5), ("Matern52", 8, 8, 16), ("Matern52", 70, 33, 128), ("Matern32", 300, 200, 40),
                                        ("Matern52", 6, 4, 1100),      # predicted means out of full 512-tick segments
                                        ("Matern32", 130, 129, 70)])   # a 2 x 2 tile U-gradient with two full k tiles and a tail
def test_window_objective_vs_oracle_loop(env, kern, M, L, W):
    """moihgp_window_set/eval == the learners' loop (moihgp_online.h:61-70): step with sensitivities, NLL + gradient on the
    pre-step state, summed over the window; checked against the oracle's per-tick calls and against our own per-tick ABI."""
    rng = np.random.default_rng(M + 3 * L + W)
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    ref = env["cref"].GP(0.1, M, L, kern); ref.set_literal_ugrad(0)
    d, P = gp.igp_dim, 3
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.04], synth_params(L, rng).ravel()])
    gp.update(params); ref.update(params)
    Y = rng.standard_normal((W, M)) * 0.5
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, P, d))
    loss, grad, xT, dxT = gp.window_objective(Y, x0, dx0)
    x, dx, lref, gref = x0, dx0, 0.0, np.zeros(gp.num_param)
    for t in range(W):
        l1, g1 = ref.negLogLikelihood(x, Y[t], dx)
        xn, _, dxn = ref.step(x, Y[t], dx)
        lref += l1; gref += g1; x, dx = xn, dxn
    assert abs(loss - lref) < 1e-9 * abs(lref)
    assert rel_err(grad, gref) < 1e-8
    assert rel_err(xT, x) < 1e-9 and rel_err(dxT, dx) < 1e-8
    # the same through our own per-tick ABI for the first ticks (consistency of the two product paths)
    x, dx, lp = x0, dx0, 0.0
    for t in range(min(W, 4)):
        l1, _ = gp.negLogLikelihood(x, Y[t], dx)
        xn, _, dxn = gp.step(x, Y[t], dx)
        lp += l1; x, dx = xn, dxn
    l4, _, x4, _ = gp.window_objective(Y[:min(W, 4)], x0, dx0)
    assert abs(l4 - lp) < 1e-10 * abs(lp) and rel_err(x4, x) < 1e-10
    # missing outputs: least-squares projection of the affected ticks on the device (moihgp.h:485-494); the loss and the mixing part of
    # the gradient are NaN as in the reference (dense products with a y that holds NaN, moihgp.h:499-563), the per-latent part and the
    # carried state finite: all of it equal to the oracle's tick loop
    if M - 3 >= L:
        Yn = Y.copy(); Yn[0, 0] = np.nan; Yn[W // 2, [1, M - 1, M // 2]] = np.nan
        loss_n, grad_n, xTn, dxTn = gp.window_objective(Yn, x0, dx0)
        x, dx, lref, gref = x0, dx0, 0.0, np.zeros(gp.num_param)
        for t in range(W):
            l1, g1 = ref.negLogLikelihood(x, Yn[t], dx)
            xn, _, dxn = ref.step(x, Yn[t], dx)
            lref += l1; gref += g1; x, dx = xn, dxn
        assert np.isnan(lref) and np.isnan(loss_n)
        assert np.array_equal(np.isnan(grad_n), np.isnan(gref))
        fin = ~np.isnan(gref)
        assert fin[M * L + L + 1:].all() and not fin[:M * L + L + 1].any()
        assert rel_err(grad_n[fin], gref[fin]) < 1e-8
        assert rel_err(xTn, x) < 1e-9 and rel_err(dxTn, dx) < 1e-8
    else:                                               # fewer observed outputs than latents: refused (rc 3), the caller loops per tick
        from multioutputihgp_amd import MoihgpError
        Yn = Y.copy(); Yn[0, :M - L + 1] = np.nan          # L - 1 observed outputs
        with pytest.raises(MoihgpError) as ei:
            gp.window_objective(Yn, x0, dx0)
        assert ei.value.rc == 3


# ------------------------------------------------------------------------------------------ N1: sharded real-data pipeline
def _sharded_worker(rank, world, port, M, L, T, q):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)       # 2 ranks share the one GPU of the test box: exchange on gloo
    torch.cuda.set_device(0)
    from multioutputihgp_amd.sharded import ShardedMOIHGP
    rng = np.random.default_rng(99)
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.04], synth_params(L, rng).ravel()])
    Y = rng.standard_normal((T, M))
    sh = ShardedMOIHGP(0.1, M, L, kernel="Matern32")
    sh.update(params)
    Yd = torch.from_numpy(Y).cuda()
    Yhat, nll = sh.filter(Yd)
    # reduce-scatter form: every rank keeps its time slice of the prediction, the residual term is formed on the local rows
    Ys, nll_s = sh.filter(Yd, scatter=True)
    # freshly constructed objects (no update()): the constructor's random U is re-drawn from a fixed seed, so the ranks agree
    sh0 = ShardedMOIHGP(0.1, M, L, kernel="Matern32")
    Y0, nll0 = sh0.filter(Yd)
    torch.cuda.synchronize()
    q.put((rank, Yhat.cpu().numpy(), nll, params, Y, Ys.cpu().numpy(), nll_s, sh0.params.copy(), Y0.cpu().numpy(), nll0))
    dist.destroy_process_group()


@pytest.mark.parametrize("M,L,T", [(12, 7, 40), (96, 64, 300)])
def test_sharded_pipeline_two_ranks_vs_oracle(env, M, L, T):
    """project -> sweep -> unproject with the latents split over 2 ranks (partial predictions all-reduced) equals the
    oracle's tick-by-tick MOIHGP::step / negLogLikelihood on the full model."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, M, L, T, q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs: p.join(timeout=60)
    (_, Yhat0, nll0, params, Y, Ys0, nlls0, p00, Y00, n00), (_, Yhat1, nll1, _, _, Ys1, nlls1, p01, Y01, n01) = res
    assert np.array_equal(Yhat0, Yhat1) and nll0 == nll1
    from multioutputihgp_amd.sharded import time_slice_bounds
    a0, b0 = time_slice_bounds(T, 2, 0); a1, b1 = time_slice_bounds(T, 2, 1)
    assert Ys0.shape == (b0 - a0, M) and Ys1.shape == (b1 - a1, M)
    assert rel_err(np.concatenate([Ys0, Ys1]), Yhat0) < 1e-13 and nlls0 == nlls1 and abs(nlls0 - nll0) < 1e-12 * abs(nll0)
    assert np.array_equal(p00, p01) and np.array_equal(Y00, Y01) and n00 == n01      # same seeded U on both ranks before any update()
    ref = env["cref"].GP(0.1, M, L, "Matern32"); ref.update(params)
    x = np.zeros((L, 2)); yh = np.zeros((T, M)); nll = 0.0
    for t in range(T):
        nll += ref.negLogLikelihood(x, Y[t])
        x, yh[t] = ref.step(x, Y[t])
    assert rel_err(Yhat0, yh) < 1e-9 and abs(nll0 - nll) < 1e-9 * abs(nll)


def _sharded_missing_worker(rank, world, port, M, L, T, q):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from multioutputihgp_amd.sharded import ShardedMOIHGP
    rng = np.random.default_rng(5)
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.04], synth_params(L, rng).ravel()])
    Y = rng.standard_normal((T, M))
    Y[rng.random((T, M)) < 0.03] = np.nan                               # a few outputs missing here and there
    Y[3, :min(5, M - L)] = np.nan                                        # a tick with several missing at once
    Y[T // 2] = rng.standard_normal(M)                                   # (and fully observed ticks in between)
    sh = ShardedMOIHGP(0.1, M, L, kernel="Matern32")
    sh.update(params)
    Yd = torch.from_numpy(Y).cuda()
    Yhat, nll = sh.filter(Yd)
    Ys, _ = sh.filter(Yd, scatter=True)
    torch.cuda.synchronize()
    q.put((rank, Yhat.cpu().numpy(), nll, params, Y, Ys.cpu().numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("M,L,T", [(12, 7, 40), (96, 64, 120)])
def test_sharded_pipeline_with_missing_outputs(env, M, L, T):
    """Partially observed ticks with the latents split over 2 ranks: the least-squares projection (moihgp.h:167-178) couples all
    latents; the shards exchange the k x k Gram matrix and right-hand side of the missing rows (one small all-reduce for the whole
    stream) and must reproduce the oracle's tick-by-tick MOIHGP::step on the full model.  The NLL of such a stream is NaN in the
    reference (moihgp.h:651 takes the norm of a vector with NaN entries), and here."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_missing_worker, args=(r, 2, port, M, L, T, q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs: p.join(timeout=60)
    (_, Yhat0, nll0, params, Y, Ys0), (_, Yhat1, nll1, _, _, Ys1) = res
    assert np.array_equal(Yhat0, Yhat1) and np.isnan(nll0) and np.isnan(nll1)
    assert rel_err(np.concatenate([Ys0, Ys1]), Yhat0) < 1e-13
    ref = env["cref"].GP(0.1, M, L, "Matern32"); ref.update(params)
    x = np.zeros((L, 2)); yh = np.zeros((T, M))
    for t in range(T):
        x, yh[t] = ref.step(x, Y[t])
    assert np.isfinite(Yhat0).all() and rel_err(Yhat0, yh) < 1e-9


# ------------------------------------------------------------------------------------------ unstable latents (literal DARE quirk)
@pytest.mark.parametrize("dtype,T", [(torch.float64, 1500), (torch.float32, 150)])
@pytest.mark.parametrize("split", ["1", "0"])
def test_unstable_latents_take_the_sequential_path(env, dtype, T, split, monkeypatch):
    """With the reference's literal DARE (utils/dare.h:23, A un-transposed) parts of the learner's own parameter box give
    rho(AKHA) > 1.  The recursion then grows like rho^t; the scan tables would overflow, so such latents are flagged at
    update() and filtered sequentially.  Results must still equal the oracle's tick loop while they are finite."""
    monkeypatch.delenv("MOIHGP_FILTER_SPLIT", raising=False)
    prm = np.array([[99.2440457, 4.06889466, 2.55306111e-03],      # rho(AKHA) = 1.47 (Matern-3/2, dt = 0.1)
                    [1.0, 1.0, 0.1],                                 # stable
                    [0.927049235, 1.63239037, 4.34082530e-04],      # rho = 1.17
                    [66.2316497, 5.1761023, 1.51666229e-03]])       # rho = 1.37
    L = prm.shape[0]
    igps = env["cref"].ihgp_array("Matern32", 0.1, prm)
    assert max(abs(np.linalg.eigvals(igps[0].mat("AKHA")))) > 1.4
    rng = np.random.default_rng(3)
    Ty = synth(L, T, rng, 0.02)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern32")
    bank.set_option("filter_split", int(split))
    o = env["cref"].filter_stream(igps, Ty)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T)
    torch.cuda.synchronize()
    yh = yhat[:, :T].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(yh)) and np.all(np.isfinite(o["yhat"]))
    tol = 1e-9 if dtype == torch.float64 else 2e-3
    for l in range(L):          # per latent: magnitudes differ by hundreds of orders
        assert rel_err(yh[l], o["yhat"][l]) < tol, l
        a, b = nll[l].item(), o["nll_per_latent"][l]
        assert (np.isinf(a) and np.isinf(b)) or abs(a - b) < tol * abs(b), l      # v^2 overflows for rho^t ~ 1e250: inf on both sides
    # gradient sweep: unstable latents go to the sequential kernel
    og = env["cref"].grad_stream(igps, Ty[:, :120])
    r = bank.grad(to_dev(Ty[:, :120], dtype), T=120)
    torch.cuda.synchronize()
    g = r["grad"].cpu().numpy()
    for l in range(L):
        assert rel_err(g[l], og["grad"][l]) < (1e-8 if dtype == torch.float64 else 5e-3), l


# ------------------------------------------------------------------------------------------ stacked (sum-of-Matern) latents
@pytest.mark.parametrize("kern", ["Matern32x2", "Matern52x2", "Matern52x3", "Matern52x4"])
def test_stacked_vs_golden(env, kern):
    g = load_golden(f"stacked_{kern}.npz")
    bank = env["streams"].LatentBank(float(g["dt"]), g["params"], kernel=kern)
    for l in range(bank.L):
        m = bank.latent(l)
        for k in ("A", "K", "HA", "AKHA"):
            assert rel_err(m[k], g[k][l]) < 1e-10, (k, rel_err(m[k], g[k][l]))
        assert abs(m["S"] - g["S"][l]) < 1e-10 * g["S"][l] and m["iters"][0] == int(g["dare_iters"][l])
    Tg = g["grad_Ty"].shape[1]
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, FP32_TOL)):          # gradient sweep golden
        r = bank.grad(to_dev(g["grad_Ty"], dtype), T=Tg, x=torch.from_numpy(g["grad_x0"]).to(dtype).cuda(),
                      dx=torch.from_numpy(g["grad_dx0"]).to(dtype).cuda(), want_yhat=True)
        torch.cuda.synchronize()
        assert rel_err(r["yhat"][:, :Tg].cpu().numpy(), g["grad_yhat"]) < tol and rel_err(r["dx"].cpu().numpy(), g["grad_dxT"]) < tol * 10
        assert rel_err(r["grad"].cpu().numpy(), g["grad_grad"]) < tol * 10 and rel_err(r["nll"].cpu().numpy(), g["grad_nll"]) < tol * 10
    for l in range(bank.L):
        m = bank.latent(l)
        for k in ("dA", "dAKHA", "dK", "dS", "HdA"):
            assert rel_err(m[k], g[k][l]) < 1e-10, (k, rel_err(m[k], g[k][l]))
        assert list(m["iters"][1:]) == list(g["dlyap_iters"][l])
    for tag in ("dense", "nan5"):
        T = g[f"{tag}_Ty"].shape[1]
        for dtype, tol in ((torch.float64, FP64_TIGHT), (torch.float32, FP32_TOL)):
            yhat, xT, nll = bank.filter(to_dev(g[f"{tag}_Ty"], dtype), T=T, x=torch.from_numpy(g[f"{tag}_x0"]).to(dtype).cuda())
            torch.cuda.synchronize()
            e = (rel_err_rows(yhat[:, :T].cpu().numpy(), g[f"{tag}_yhat"]), rel_err(xT.cpu().numpy(), g[f"{tag}_xT"]), rel_err(nll.cpu().numpy(), g[f"{tag}_nll"]))
            assert max(e) < tol, (kern, tag, dtype, e)


@pytest.mark.parametrize("kern", STACKED)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T", [(1, 1), (3, 15), (2, 16), (5, 17), (4, 1023), (3, 1024), (6, 1025), (1030, 2100), (3, 0)])
def test_stacked_ragged_shapes_vs_oracle(env, kern, dtype, L, T):
    J = int(kern[-1])
    rng = np.random.default_rng(77 * L + T + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    d = bank.d
    x0 = 0.2 * rng.standard_normal((L, d))
    if T == 0:
        _, xT, nll = bank.filter(torch.zeros((L, 4), dtype=dtype, device="cuda"), T=0, x=torch.from_numpy(x0).to(dtype).cuda())
        torch.cuda.synchronize()
        assert rel_err(xT.cpu().numpy(), x0) < 1e-6 and float(nll.abs().sum()) == 0.0
        return
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    Ty = synth(L, T, rng)
    o = env["cref"].filter_stream(igps, Ty, x0=x0, nthreads=4)
    Tyd = to_dev(Ty, dtype)
    yhat, xT, nll = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    # latents the literal DARE leaves unstable (rho(AKHA) > 1, seen for stacked Matern-3/2) grow without bound: compare those
    # on the scale of their own trajectory
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    for l in range(L):
        scale = max(np.abs(o["yhat"][l]).max(), 1e-300)
        if not np.isfinite(scale) or scale > (1e250 if dtype == torch.float64 else 1e30):
            continue                              # overflows the stream's precision: nothing to compare
        assert np.abs(yhat[l, :T].cpu().numpy() - o["yhat"][l]).max() / scale < tol * 10, (l, scale)
    ok = np.isfinite(o["nll_per_latent"]) & (np.abs(o["yhat"]).max(axis=1) < (1e120 if dtype == torch.float64 else 1e15))
    assert rel_err(nll.cpu().numpy()[ok], o["nll_per_latent"][ok]) < tol * 10
    _, x2, nll2 = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_yhat=False)
    yh3, x3, _ = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_nll=False)
    _, x4, _ = bank.filter(Tyd, T=T, x=torch.from_numpy(x0).to(dtype).cuda(), want_yhat=False, want_nll=False)   # state only
    torch.cuda.synchronize()
    # the nll-only / yhat-only instantiations agree with the fused one to rounding (overflowed latents hold inf / NaN in all)
    rt = 1e-12 if dtype == torch.float64 else 1e-5
    same = lambda a, b: torch.allclose(a, b, rtol=rt, atol=rt * float(torch.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).abs().max()), equal_nan=True)
    assert same(nll2, nll) and same(x2, xT) and same(x3, xT) and same(x4, xT) and same(yh3[:, :T], yhat[:, :T])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kern,L,T", [("Matern52x2", 3, 2047), ("Matern52x2", 3, 2048), ("Matern52x4", 2, 2049), ("Matern32x3", 3, 4096), ("Matern52x3", 2, 4097),
                                      ("Matern52x4", 1024, 2048), ("Matern32x2", 1024, 4097), ("Matern52x2", 1030, 6144)])
def test_stacked_segment_boundaries(env, kern, dtype, L, T):
    """Streams ending exactly at, one tick short of and one tick past a 2048-tick segment, in the time-split kernels (few latents)
    and in the four-waves-per-block kernels (L >= 1024): the single replay takes its carry-out at the tick where the stream ends."""
    J = int(kern[-1])
    rng = np.random.default_rng(13 * L + T + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    x0 = 0.2 * rng.standard_normal((L, bank.d))
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    Ty = synth(L, T, rng)
    o = env["cref"].filter_stream(igps, Ty, x0=x0, nthreads=8)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    got, gx, gn = yhat[:, :T].cpu().numpy(), xT.cpu().numpy(), nll.cpu().numpy()
    lim = 1e120 if dtype == torch.float64 else 1e15
    ok = np.isfinite(o["nll_per_latent"]) & (np.abs(o["yhat"]).max(axis=1) < lim)      # latents the literal DARE leaves unstable: elsewhere
    assert ok.sum() >= max(1, L // 2)
    scale = np.abs(o["yhat"][ok]).max(axis=1, keepdims=True)
    assert (np.abs(got[ok] - o["yhat"][ok]) / scale).max() < tol
    assert rel_err(gn[ok], o["nll_per_latent"][ok]) < tol
    assert (np.abs(gx[ok] - o["x"][ok]).max(axis=1) / np.maximum(np.abs(o["x"][ok]).max(axis=1), 1e-3 * scale[:, 0])).max() < tol * 10


def test_stacked_mildly_unstable_latents_stay_on_the_scan_path(env):
    """The literal DARE (dare.h:23) leaves some stacked Matern-3/2 latents with rho(AKHA) slightly above 1 (these parameter
    sets come from the bench's own draw).  Their trajectories grow like rho^t but stay far inside fp64's range, and the
    segment solve must follow them tick for tick (error measured against the trajectory's running magnitude)."""
    prm = np.array([[1.42962333, 1.59788413, 1.91620496, 1.66245887, 0.05233625],
                    [0.7227578, 1.71853154, 1.59357212, 1.81934245, 0.05206774],
                    [0.85943105, 1.84330571, 1.96285317, 1.72411971, 0.0601299],
                    [1.0, 1.0, 1.0, 1.0, 0.1]])
    kern, T = "Matern32x2", 4500
    rng = np.random.default_rng(5)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    rho = [np.max(np.abs(np.linalg.eigvals(g.mat("AKHA")))) for g in igps]
    assert max(rho[:3]) > 1.0 and min(rho[:3]) > 1.0 and rho[3] < 1.0, rho
    Ty = synth(4, T, rng)
    o = env["cref"].filter_stream(igps, Ty, nthreads=2)
    yhat, xT, nll = bank.filter(to_dev(Ty, torch.float64), T=T)
    torch.cuda.synchronize()
    got = yhat[:, :T].cpu().numpy()
    assert np.isfinite(got).all() and np.abs(o["yhat"][:3]).max() > 1e20           # they did grow
    running = np.maximum.accumulate(np.abs(o["yhat"]), axis=1) + 1e-300
    assert (np.abs(got - o["yhat"]) / running).max() < 1e-8
    assert rel_err(nll.cpu().numpy(), o["nll_per_latent"]) < 1e-8
    assert rel_err(xT.cpu().numpy(), o["x"]) < 1e-8


@pytest.mark.parametrize("kern", ["Matern52x2", "Matern52x4"])
def test_stacked_missing_data_and_slabs(env, kern):
    J = int(kern[-1])
    rng = np.random.default_rng(5 + J)
    L, T = 9, 3000
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    Ty = synth(L, T, rng, nan_frac=0.03)
    Ty[0, :] = np.nan
    Ty[1, 500:2500] = np.nan
    Ty[2, :] = synth(1, T, rng)[0]                   # one dense series among gappy ones
    o = env["cref"].filter_stream(igps, Ty, nthreads=4)
    Tyd = to_dev(Ty, torch.float64)
    yhat, xT, nll = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    assert rel_err(yhat[:, :T].cpu().numpy(), o["yhat"]) < FP64_TIGHT and rel_err(xT.cpu().numpy(), o["x"]) < FP64_TIGHT
    assert rel_err(nll.cpu().numpy(), o["nll_per_latent"]) < FP64_TIGHT and nll[0].item() == 0.0
    cut = 1024 + 16 * 3 + 4                          # slab boundary inside a segment and inside a chunk
    ya, xa, na = bank.filter(Tyd[:, :cut], T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:], T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    assert rel_err(torch.cat([ya[:, :cut], yb[:, :T - cut]], 1).cpu().numpy(), o["yhat"]) < FP64_TIGHT
    assert rel_err((na + nb).cpu().numpy(), o["nll_per_latent"]) < FP64_TIGHT and rel_err(xb.cpu().numpy(), o["x"]) < FP64_TIGHT


@pytest.mark.parametrize("kern", ["Matern32x2", "Matern52x2", "Matern52x3", "Matern52x4"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stacked_filter_gaps_as_broken_links(env, kern, dtype):
    """With >= 1024 latents the stacked filter handles a segment with few gaps in a second pass that treats the chunks holding them as
    broken links of the scan (csrc/recursion_x.hip: scan of the gap-free run, gap-aware replay up to and including the chunk with
    the gap, its end state carried into the next run) instead of walking the segment tick by tick.  Gaps are placed where the
    stages meet: first and last tick of the stream, first / last tick of a chunk, neighbouring chunks, a whole chunk missing, the
    ragged last segment, more chunks with a gap than the second pass takes (walked), a series without any observation."""
    J = int(kern[-1])
    L, T = 1030, 4500
    rng = np.random.default_rng(17 + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng)
    Ty[1, 0] = np.nan; Ty[2, T - 1] = np.nan
    Ty[3, [31, 32, 63, 64]] = np.nan                      # chunk ends and starts: neighbouring chunks with a gap
    Ty[4, 96:128] = np.nan                                # a whole chunk
    Ty[5, [700, 2100, 2200, 4300, 4490]] = np.nan         # one or two per segment, the ragged one too
    Ty[6, ::50] = np.nan                                  # 41 chunks with a gap per segment: walked
    Ty[7, :] = np.nan
    Ty[8, 2048 - 1] = np.nan; Ty[8, 2048] = np.nan        # both sides of a segment boundary
    Ty[9, 5::512] = np.nan
    Ty[100:, :][rng.random((L - 100, T)) < 0.0004] = np.nan          # here and there in most of the others
    sub = np.concatenate([np.arange(12), np.sort(rng.choice(np.arange(100, L), size=20, replace=False))])
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=4)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T)
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6                 # literal-DARE unstable latents aside
    yg = yhat[sub][:, :T].cpu().numpy().astype(np.float64)
    assert rel_err_rows(yg[tame], o["yhat"][tame]) < tol * 10
    assert rel_err(xT[sub].cpu().numpy()[tame], o["x"][tame]) < tol * 10
    assert rel_err(nll[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol * 10 and nll[7].item() == 0.0
    # the same stream in two slabs that carry the state (cut inside a chunk)
    cut = 2048 + 32 * 5 + 8
    Tyd = to_dev(Ty, dtype)
    ya, xa, na = bank.filter(Tyd[:, :cut].contiguous(), T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:].contiguous(), T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    assert rel_err_rows(torch.cat([ya[:, :cut], yb[:, :T - cut]], 1)[sub].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]) < tol * 10
    assert rel_err((na + nb)[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol * 10


@pytest.mark.parametrize("kern", ["Matern32x2", "Matern52x2", "Matern32x4", "Matern52x3", "Matern52x4"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("nanf", [0.01, 0.05, 0.3])
def test_stacked_gaps_by_imputation(env, kern, dtype, nanf, monkeypatch, capfd):
    """Many latents, a stacked state: latents whose stream holds missing ticks are swept by EXACT IMPUTATION (csrc/gaps_x.hip; automatic from
    d = 8 on, forced here for every d): a gap-free sweep with the gaps as zeros, the scalar triangular recursion w_p = HA x'_p + sum_q s_(p-q-1) w_q
    over each latent's gaps, a second gap-free sweep with the gaps filled by their own predictions.  ihgp.h:83-87 / :204-209 semantics (x <- A x,
    no likelihood term) against the oracle: dense random gaps (1 %, 5 %, 30 % of the ticks), gaps at both ends, runs of gaps, a series with no
    observation at all and one with more gaps inside the filter's memory than the recursion's window holds (both left to the second pass),
    gap-free latents in between, and the stream in two slabs that carry the state."""
    J = int(kern[-1])
    L, T = 1040, 4500
    rng = np.random.default_rng(23 + J + int(100 * nanf))
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    bank.set_option("filter_impute", 1)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < nanf] = np.nan
    Ty[0:40] = synth(40, T, rng)                           # some latents without any gap
    Ty[41, 0] = np.nan; Ty[42, T - 1] = np.nan; Ty[43, :5] = np.nan; Ty[44, T - 7:] = np.nan
    Ty[45, 1000:1400] = np.nan                             # a long run
    Ty[46, :] = np.nan                                     # nothing observed
    Ty[47, ::2] = np.nan                                   # every other tick: more gaps inside the decay than the window holds
    sub = np.concatenate([np.arange(36, 60), np.sort(rng.choice(np.arange(60, L), size=24, replace=False))])
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=8)
    Tyd = to_dev(Ty, dtype)
    monkeypatch.setenv("MOIHGP_GAP_TRACE", "1")
    capfd.readouterr()
    yhat, xT, nll = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    monkeypatch.delenv("MOIHGP_GAP_TRACE")
    trace = re.search(r"gap imputation: (\d+) latents handed over, (\d+) solved, (\d+) gaps", capfd.readouterr().err)
    assert trace, "the imputation path did not run"
    handed, solved = int(trace.group(1)), int(trace.group(2))
    assert handed >= ((L - 41) * 9) // 10 and solved >= (handed * 3) // 4, (handed, solved)             # (a filter without scan tables, or a slowly forgetting one, stays with the second pass)
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6                 # literal-DARE unstable latents aside
    assert tame.sum() > len(sub) // 2
    yg = yhat[sub][:, :T].cpu().numpy().astype(np.float64)
    assert rel_err_rows(yg[tame], o["yhat"][tame]) < tol
    assert rel_err(xT[sub].cpu().numpy()[tame], o["x"][tame]) < tol
    assert rel_err(nll[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol and nll[46].item() == 0.0
    # NLL-only and means-only sweeps, and the same stream in two slabs
    _, x2, n2 = bank.filter(Tyd, T=T, want_yhat=False)
    y3, x3, _ = bank.filter(Tyd, T=T, want_nll=False)
    cut = 2048 + 32 * 5 + 8
    ya, xa, na = bank.filter(Tyd[:, :cut].contiguous(), T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:].contiguous(), T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    assert rel_err(n2[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol and rel_err(x3[sub].cpu().numpy()[tame], o["x"][tame]) < tol
    assert rel_err_rows(y3[sub][:, :T].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]) < tol
    assert rel_err_rows(torch.cat([ya[:, :cut], yb[:, :T - cut]], 1)[sub].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]) < tol
    assert rel_err((na + nb)[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol
    # the second pass of recursion_x.hip on the same stream (imputation off): the two treatments of a gap agree
    bank.set_option("filter_impute", 0)
    y0, x0_, n0 = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    assert rel_err_rows(y0[sub][:, :T].cpu().numpy().astype(np.float64)[tame], yg[tame]) < tol
    assert rel_err(n0[sub].cpu().numpy()[tame], nll[sub].cpu().numpy()[tame]) < tol


@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 64, 2047, 2048, 2049, 4113])
@pytest.mark.parametrize("kern,dtype", [("Matern52x4", torch.float64), ("Matern52x3", torch.float32), ("Matern32x4", torch.float64)])
def test_imputation_at_awkward_lengths(env, kern, dtype, T):
    """The imputation sweeps at stream lengths around the chunk (32 ticks) and segment (2048) boundaries, down to a single tick: 10 % of the ticks
    missing, a gap at the first and at the last tick, one series without any observation, one that is all gaps but its last tick; the stream
    continued from a carried state; against the oracle and against the second pass alone (filter_impute = 0)."""
    J = int(kern[-1])
    L = 1024
    rng = np.random.default_rng(7 * T + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    bank.set_option("filter_impute", 1)
    Ty = synth(L, T, rng)
    Ty[rng.random((L, T)) < 0.1] = np.nan
    Ty[0, :] = synth(1, T, rng)[0]                        # a gap-free latent
    Ty[1, 0] = np.nan; Ty[2, T - 1] = np.nan
    Ty[3, :] = np.nan
    Ty[4, :T - 1] = np.nan; Ty[4, T - 1] = 0.3
    sub = np.concatenate([np.arange(8), np.sort(rng.choice(np.arange(8, L), size=24, replace=False))])
    igps = env["cref"].ihgp_array(kern, 0.1, prm[sub])
    x0 = 0.1 * rng.standard_normal((L, bank.d))
    o = env["cref"].filter_stream(igps, np.ascontiguousarray(Ty[sub]), x0=np.ascontiguousarray(x0[sub]), nthreads=4)
    xs = torch.from_numpy(x0).to(device="cuda", dtype=dtype)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T, x_start=xs)
    torch.cuda.synchronize()
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6
    yg = yhat[sub][:, :T].cpu().numpy().astype(np.float64)
    assert rel_err_rows(yg[tame], o["yhat"][tame]) < tol
    assert rel_err(xT[sub].cpu().numpy()[tame], o["x"][tame]) < tol
    a, b = nll[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1.0)) and nll[3].item() == 0.0
    bank.set_option("filter_impute", 0)
    y0, x0_, n0 = bank.filter(to_dev(Ty, dtype), T=T, x_start=xs)
    torch.cuda.synchronize()
    assert rel_err_rows(y0[sub][:, :T].cpu().numpy().astype(np.float64)[tame], yg[tame]) < tol
    assert rel_err(x0_[sub].cpu().numpy()[tame], xT[sub].cpu().numpy()[tame]) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_imputation_leaves_unstable_filters_alone(env, dtype, monkeypatch, capfd):
    """The literal DARE (dare.h:23) returns gains with rho(AKHA) a fraction of a per cent above 1 for a few per cent of the stacked Matern-3/2 draws.
    Imputation is not for them: the sweep with zeros at the gaps departs from the true one like rho^t (rho = 1.0026 over 16384 ticks: 3e18), and
    x = x' + e cancels it all -- found by tools/fuzz_campaign.py (seed 401: NLL 3e27 where the oracle has -4e3) on a latent whose growing mode is so
    weakly observed that its impulse response still decays over the table.  The sweeps read the growth off AKHA^4096 and leave such latents to the
    second pass; every latent's row against the oracle, row by row."""
    kern, L, T, seed = "Matern32x4", 1097, 16384, 1634409831
    rng = np.random.default_rng(seed)
    prm = synth_params_stacked(L, 4, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    x0 = 0.3 * rng.standard_normal((L, bank.d))
    Ty = synth(L, T, rng, nan_frac=0.3)
    o = env["cref"].filter_stream(igps, Ty, x0=x0, nthreads=8)
    monkeypatch.setenv("MOIHGP_GAP_TRACE", "1")
    capfd.readouterr()
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    monkeypatch.delenv("MOIHGP_GAP_TRACE")
    trace = re.search(r"gap imputation: (\d+) latents handed over, (\d+) solved, .*not solved: (\d+) response not finite or growing", capfd.readouterr().err)
    assert trace and int(trace.group(2)) >= 1000 and int(trace.group(3)) >= 5, trace and trace.groups()
    big = np.nan_to_num(np.abs(o["yhat"]), nan=0.0, posinf=np.inf).max(axis=1)
    calm = big < 1e3                                              # (the unstable latents that have grown large are compared loosely below)
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    yg = yhat[:, :T].cpu().numpy().astype(np.float64)
    assert rel_err_rows(yg[calm], o["yhat"][calm]) < tol
    a, b = nll.cpu().numpy()[calm], o["nll_per_latent"][calm]
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1.0))
    wild = (big >= 1e3) & (big < (1e100 if dtype == torch.float64 else 1e18))
    if wild.any():
        assert rel_err_rows(yg[wild], o["yhat"][wild]) < (1e-6 if dtype == torch.float64 else 1e-2)


def test_fp32_bank_sweeps_unscannable_latents_in_fp64(env, monkeypatch, capfd):
    """Many latents, fp32 streams: a mildly unstable latent (the literal DARE of dare.h:23 returns such gains: rho(AKHA) of 1.04 .. 1.4) has scan tables
    that leave the fp32 range but not the fp64 one.  Tick by tick in the fp32 kernel one of them holds the whole launch (BASELINE-sized Matern32x2
    bank: 7 of 4096, 302 us against 80); they are listed at update(), left alone by the many-latent kernel and swept in fp64 beside it
    (csrc/capi.cpp).  Their rows against the oracle while the values fit fp32, the other latents as before, with and without gaps in the stream."""
    from bench import synth_params, SEED
    kern, L = "Matern32x2", 4096
    prm = synth_params(L, 0, np.random.default_rng(SEED), kern)
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    rho = np.array([max(abs(np.linalg.eigvals(g.mat("AKHA")))) for g in igps])
    wild = np.flatnonzero((rho > 1.045) & (rho < 1.3))           # rho^1024 beyond 1e18 (fp32 tables unusable), below 1e150 (fp64 ones fine)
    assert len(wild) >= 1, ("the synthetic bank holds no mildly unstable latent", np.sort(rho)[-10:])
    T = int(min(1400, 60.0 / np.log(rho[wild].max())))           # while rho^T fits fp32 with room to spare
    rng = np.random.default_rng(5)
    Ty = synth(L, T, rng)
    Ty[wild[0], [7, T // 3, T // 3 + 1, T - 1]] = np.nan          # the side sweep takes gaps the way the fp64 kernels do
    sub = np.concatenate([wild, np.sort(rng.choice(np.flatnonzero(rho < 0.999), size=24, replace=False))])
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=8)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    monkeypatch.setenv("MOIHGP_GAP_TRACE", "1")
    capfd.readouterr()
    yhat, xT, nll = bank.filter(to_dev(Ty, torch.float32), T=T)
    torch.cuda.synchronize()
    monkeypatch.delenv("MOIHGP_GAP_TRACE")
    trace = re.search(r"side sweep: (\d+) latents", capfd.readouterr().err)
    assert trace and int(trace.group(1)) >= len(wild), "the fp64 side sweep did not run"
    yg = yhat[sub][:, :T].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(o["yhat"])) and np.all(np.isfinite(yg))
    assert rel_err_rows(yg, o["yhat"]) < FP32_TOL
    assert rel_err(xT[sub].cpu().numpy(), o["x"]) < FP32_TOL
    a, b = nll[sub].cpu().numpy(), o["nll_per_latent"]
    assert np.all(np.abs(a - b) <= FP32_TOL * np.abs(b))
    # NLL-only sweep, and the running total over all latents
    _, x2, n2 = bank.filter(to_dev(Ty, torch.float32), T=T, want_yhat=False)
    torch.cuda.synchronize()
    assert np.all(np.abs(n2[sub].cpu().numpy() - b) <= FP32_TOL * np.abs(b)) and rel_err(x2[sub].cpu().numpy(), o["x"]) < FP32_TOL


@pytest.mark.parametrize("kern,M,L", [("Matern32x2", 6, 3), ("Matern52x2", 8, 8), ("Matern52x4", 9, 4), ("Matern52x3", 150, 70)])
def test_stacked_full_objects_vs_oracle(env, kern, M, L):
    """BASELINE.json's d = 6 / d = 12 configurations behind the whole MOIHGP surface: a stacked StateSpace in the template slot of
    moihgp::MOIHGP<SS> (moihgp.h:76): update / getParams with P = 2J + 1 per-latent parameters, the four step overloads, both
    negLogLikelihood overloads (gradient incl. the per-latent block), missing outputs, and the windowed objective."""
    rng = np.random.default_rng(M * 31 + L)
    J = int(kern[-1]); P = 2 * J + 1
    gp = env["MOIHGP"](0.1, M, L, kernel=kern)
    ref = env["cref"].GP(0.1, M, L, kern); ref.set_literal_ugrad(0)
    d = gp.igp_dim
    assert d == (2 if kern.startswith("Matern32") else 3) * J and gp.num_igp_param == P and gp.num_param == M * L + L + 1 + L * P
    assert ref.igp_dim == d and ref.num_igp_param == P
    assert rel_err(gp.params[M * L:], ref.params[M * L:]) < 1e-15        # constructor state: S = 1, sigma = 1e-2, default per-latent parameters
    igp = synth_params_stacked(L, J, rng)
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.04], igp.ravel()])
    gp.update(params); ref.update(params)
    assert rel_err(gp.params, ref.params) < FP64_TIGHT
    x, dx = 0.3 * rng.standard_normal((L, d)), 0.1 * rng.standard_normal((L, P, d))
    for it in range(3):
        y = rng.standard_normal(M)
        l2a, l2b = gp.negLogLikelihood(x, y), ref.negLogLikelihood(x, y)
        assert abs(l2a - l2b) < FP64_TIGHT * max(1.0, abs(l2b))
        l1a, g1a = gp.negLogLikelihood(x, y, dx); l1b, g1b = ref.negLogLikelihood(x, y, dx)
        assert abs(l1a - l1b) < FP64_TIGHT * max(1.0, abs(l1b)) and rel_err(g1a, g1b) < 1e-8
        a3, b3 = gp.step(x, y), ref.step(x, y)
        a4, b4 = gp.step(x), ref.step(x)
        a2, b2 = gp.step_no_yhat(x, y, dx), ref.step2(x, y, dx)
        a1, b1 = gp.step(x, y, dx), ref.step(x, y, dx)
        for u, v in list(zip(a3, b3)) + list(zip(a4, b4)) + list(zip(a2, b2)) + list(zip(a1, b1)):
            assert rel_err(u, v) < FP64_TIGHT
        x, dx = a1[0], a1[2]
    if M > L:                                                   # least-squares projection over the observed rows (moihgp.h:167-178)
        ym = rng.standard_normal(M); ym[rng.choice(M, size=max(1, (M - L) // 2), replace=False)] = np.nan
        a, b = gp.step(x, ym), ref.step(x, ym)
        assert rel_err(a[0], b[0]) < FP64_TIGHT and rel_err(a[1], b[1]) < FP64_TIGHT
    # the learners' window loop as one device call
    W = 7
    Y = 0.5 * rng.standard_normal((W, M))
    loss, grad, xT, dxT = gp.window_objective(Y, x, dx)
    xr, dxr, lref, gref = x, dx, 0.0, np.zeros(gp.num_param)
    for t in range(W):
        l1, g1 = ref.negLogLikelihood(xr, Y[t], dxr)
        xr, _, dxr = ref.step(xr, Y[t], dxr)
        lref += l1; gref += g1
    assert abs(loss - lref) < 1e-9 * max(1.0, abs(lref)) and rel_err(grad, gref) < 1e-8
    assert rel_err(xT, xr) < 1e-9 and rel_err(dxT, dxr) < 1e-8
    # whole streams through the same object: project -> stacked filter -> unproject == the tick loop
    T = 50
    Ys = rng.standard_normal((T, M))
    Ty = env["streams"].project_stream(gp, torch.from_numpy(Ys).cuda())
    bank = env["streams"].LatentBank.from_handle(gp)
    yl, _, _ = bank.filter(Ty, T=T)
    Yhat = env["streams"].unproject_stream(gp, yl, T)
    torch.cuda.synchronize()
    xr = np.zeros((L, d)); out = np.empty((T, M))
    for t in range(T):
        xr, out[t] = ref.step(xr, Ys[t])
    assert rel_err(Yhat.cpu().numpy(), out) < 1e-9


@pytest.mark.parametrize("kern,dtype", [("Matern52", torch.float64), ("Matern52x2", torch.float64), ("Matern52x2", torch.float32), ("Matern32x2", torch.float64)])
@pytest.mark.parametrize("nanf", [0.0005, 0.02])
def test_configs1_shape_with_gaps(env, kern, dtype, nanf):
    """BASELINE configs[1] shape (256 x 1e4) with missing ticks: every compute unit holds one latent, every segment of a latent is solved as a
    scan of its chunks' own maps inside the team kernel (recursion_x.hip chunk_maps_scan / replay_gaps) and handed on through the LDS flag chain.
    A 40-latent subset against the oracle, and the sweep in two slabs that carry the state."""
    L, T = 256, 10000
    stacked = "x" in kern
    rng = np.random.default_rng(3 + int(nanf * 1e4))
    prm = synth_params_stacked(L, int(kern[-1]), rng) if stacked else synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng, nan_frac=nanf)
    Ty[5, :] = np.nan; Ty[6, 2000:9000] = np.nan
    Tyd = to_dev(Ty, dtype)
    yhat, xT, nll = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    sub = np.concatenate([np.arange(8), np.sort(rng.choice(np.arange(8, L), size=32, replace=False))])
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=8)
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0, posinf=np.inf).max(axis=1) < 1e6
    assert tame.sum() >= 30
    assert rel_err_rows(yhat[sub][:, :T].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]) < tol
    assert rel_err(xT[sub].cpu().numpy()[tame], o["x"][tame]) < tol and rel_err(nll[sub].cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol
    assert nll[5].item() == 0.0
    cut = 4096 + 20 * 3 + 4                              # inside a segment and inside a chunk of either chunk length; a 16-byte boundary
    ya, xa, na = bank.filter(Tyd[:, :cut], T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:], T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    rt = 1e-9 if dtype == torch.float64 else 2e-4
    tm = torch.from_numpy(np.isin(np.arange(L), sub[tame])).cuda()
    whole = yhat[:, :T][tm]; parts = torch.cat([ya[:, :cut], yb[:, :T - cut]], 1)[tm]
    assert ((parts - whole).abs() / (whole.abs().amax(dim=1, keepdim=True) + 1e-30)).max().item() < rt
    assert rel_err((na + nb)[tm].cpu().numpy(), nll[tm].cpu().numpy()) < rt


@pytest.mark.parametrize("kern,dtype,L,T", [("Matern52x2", torch.float64, 256, 10000), ("Matern52x4", torch.float64, 4096, 10000),
                                            ("Matern52x2", torch.float32, 4096, 10000)])
def test_stacked_full_size_properties(env, kern, dtype, L, T):
    """BASELINE configs[1] (d = 6, fp64, 256 x 1e4) and configs[4] (d = 12, fp64, 4096 x 1e4) shapes: a 48-latent subset
    against the oracle, linearity, slab consistency."""
    J = int(kern[-1])
    rng = np.random.default_rng(11)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng)
    Tyd = to_dev(Ty, dtype)
    yhat, xT, nll = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    sub = np.sort(rng.choice(L, size=48, replace=False))
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), nthreads=4)
    e = (rel_err_rows(yhat[sub][:, :T].cpu().numpy(), o["yhat"]), rel_err(xT[sub].cpu().numpy(), o["x"]), rel_err(nll[sub].cpu().numpy(), o["nll_per_latent"]))
    print(f"stacked full-size {kern} {dtype} L={L}: subset vs oracle yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e}")
    assert max(e) < (FP64_TOL if dtype == torch.float64 else FP32_TOL)
    Y2 = to_dev(synth(L, T, rng), dtype)
    f2, _, _ = bank.filter(Y2, T=T, want_nll=False)
    f12, _, _ = bank.filter(2.0 * Tyd - 0.5 * Y2, T=T, want_nll=False)
    torch.cuda.synchronize()
    lin = (f12 - (2.0 * yhat - 0.5 * f2))[:, :T].abs().max().item() / f12[:, :T].abs().max().item()
    assert lin < (1e-10 if dtype == torch.float64 else 5e-5), lin
    cut = 4096 + 4 * 37
    ya, xa, na = bank.filter(Tyd[:, :cut], T=cut)
    yb, xb, nb = bank.filter(Tyd[:, cut:], T=T - cut, x=xa.clone())
    torch.cuda.synchronize()
    tol = 1e-8 if dtype == torch.float64 else FP32_TOL
    d1 = (torch.cat([ya[:, :cut], yb[:, :T - cut]], 1) - yhat[:, :T]).abs().max().item() / yhat[:, :T].abs().max().item()
    d2 = ((na + nb) - nll).abs().max().item() / nll.abs().max().item()
    assert max(d1, d2) < tol, (d1, d2)


@pytest.mark.parametrize("kern", STACKED)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T", [1025, 2049, 5000, 10000, 10240, 12000, 14000, 16384])
def test_stacked_team_kernels_vs_oracle(env, kern, dtype, T):
    """Few latents, streams of 2 .. 8 segments: one workgroup per latent, one wavefront per segment (recursion_x.hip, the team kernels:
    eight wavefronts and chunks of 16 .. 32 ticks to match where the replay allows it, 32-tick chunks otherwise or on request).  Each form
    against the oracle's tick loop and against the one-wavefront sweep, with what the segments hand to each other exercised: a latent that
    decays too slowly for the zero-start chaining, gaps in one segment only, sparse gaps everywhere, a series never observed, a start state."""
    J = int(kern[-1])
    rng = np.random.default_rng(31 * J + T)
    L = 7
    prm = synth_params_stacked(L, J, rng)
    prm[0, 1::2][:J] = 90.0; prm[0, -1] = 1e-3          # slow latent: lengthscales 90, noise 1e-3
    prm[5, 1::2][:J] = 25.0; prm[5, -1] = 0.02          # in between
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng)
    Ty[1, 1030:1040] = np.nan                           # one segment of either form
    Ty[2, rng.random(T) < 0.01] = np.nan
    Ty[3, :] = np.nan
    Ty[4, [0, 1023, 1024, T - 1]] = np.nan              # segment boundaries, first and last tick
    Tyd = to_dev(Ty, dtype)
    x0 = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(dtype).cuda()
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0.double().cpu().numpy(), nthreads=4)
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6     # (the slow latents may be unstable under the literal DARE)
    assert tame.sum() >= 5
    bank.set_option("filter_team", 0); bank.set_option("filter_split", 1)
    y0, xT0, n0 = bank.filter(Tyd, T=T, x=x0.clone())
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    for mode in (1, 2, -1):
        bank.set_option("filter_team", mode); bank.set_option("filter_split", 0)
        yh, xT, nll = bank.filter(Tyd, T=T, x=x0.clone())
        _, xb, nb = bank.filter(Tyd, T=T, x=x0.clone(), want_yhat=False)
        yc, xc, _ = bank.filter(Tyd, T=T, x=x0.clone(), want_nll=False)
        torch.cuda.synchronize()
        yg, yo = yh[:, :T].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]
        okn = np.isfinite(yo)
        assert np.array_equal(np.isfinite(yg), okn), mode
        assert np.abs((yg - yo)[okn]).max() / np.abs(yo[okn]).max() < tol * 10, mode
        assert rel_err(xT.cpu().numpy()[tame], o["x"][tame]) < tol * 10 and rel_err(nll.cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol * 10, mode
        assert nll[3].item() == 0.0
        # against the one-wavefront sweep, every latent (the unstable ones too, while finite), and the other output combinations
        rt = 1e-10 if dtype == torch.float64 else 2e-4
        ok = torch.isfinite(y0[:, :T])
        assert torch.equal(torch.isfinite(yh[:, :T]), ok), mode
        scale = torch.where(ok, y0[:, :T], torch.zeros_like(y0[:, :T])).abs().amax(dim=1, keepdim=True) + 1e-30
        assert (torch.where(ok, yh[:, :T] - y0[:, :T], torch.zeros_like(y0[:, :T])).abs() / scale).max().item() < rt, mode
        fin = torch.isfinite(n0)
        assert rel_err(nll[fin].cpu().numpy(), n0[fin].cpu().numpy()) < rt and rel_err(nb[fin].cpu().numpy(), n0[fin].cpu().numpy()) < rt, mode
        for xx in (xT, xb, xc):
            assert rel_err(torch.nan_to_num(xx).cpu().numpy(), torch.nan_to_num(xT0).cpu().numpy()) < rt, mode
        assert (torch.where(ok, yc[:, :T] - yh[:, :T], torch.zeros_like(y0[:, :T])).abs() / scale).max().item() < rt, mode


@pytest.mark.parametrize("kern", ["Matern52", "Matern32"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("T", [1025, 4097, 10000, 16384])
def test_reference_models_on_the_team_kernel_vs_oracle(env, kern, dtype, T):
    """The reference's own models (d = 2, 3) at few latents: the stacked filter's team kernel with one component (tables rebuilt from the CB
    blocks, stationary_x.hip xc_from_cb_kernel) against the oracle's tick loop and against recursion.hip's own time split: clean streams, a
    slow latent, gaps in one segment / everywhere / at the segment boundaries, a series never observed, unstable latents (literal DARE)."""
    rng = np.random.default_rng(91 + T + len(kern))
    L = 9
    prm = synth_params(L, rng)
    prm[0] = [1.0, 90.0, 1e-3]                            # slow: long lengthscale, tiny noise
    prm[7] = [99.2440457, 4.06889466, 2.55306111e-03]     # unstable under the literal DARE at Matern-3/2 (rho = 1.47)
    prm[8] = [0.927049235, 1.63239037, 4.34082530e-04]
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng)
    Ty[1, 1030:1040] = np.nan
    Ty[2, rng.random(T) < 0.01] = np.nan
    Ty[3, :] = np.nan
    Ty[4, [0, 1023, 1024, T - 1]] = np.nan
    Tyd = to_dev(Ty, dtype)
    x0 = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(dtype).cuda()
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0.double().cpu().numpy(), nthreads=4)
    lim = 1e100 if dtype == torch.float64 else 1e12
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0, posinf=np.inf).max(axis=1) < lim
    assert tame.sum() >= 5
    bank.set_option("filter_team", 0)
    y0, xT0, n0 = bank.filter(Tyd, T=T, x=x0.clone())
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    for mode in (1, -1):
        bank.set_option("filter_team", mode)
        yh, xT, nll = bank.filter(Tyd, T=T, x=x0.clone())
        _, xb, nb = bank.filter(Tyd, T=T, x=x0.clone(), want_yhat=False)
        yc, xc, _ = bank.filter(Tyd, T=T, x=x0.clone(), want_nll=False)
        torch.cuda.synchronize()
        yg, yo = yh[:, :T].cpu().numpy().astype(np.float64)[tame], o["yhat"][tame]
        okn = np.isfinite(yo)
        assert np.array_equal(np.isfinite(yg), okn), mode
        scale = np.nanmax(np.abs(np.where(okn, yo, 0.0)), axis=1, keepdims=True) + 1e-300
        assert (np.abs(np.where(okn, yg - yo, 0.0)) / scale).max() < tol * 10, mode
        assert rel_err(xT.cpu().numpy()[tame], o["x"][tame]) < tol * 10 and rel_err(nll.cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol * 10, mode
        assert nll[3].item() == 0.0
        # against recursion.hip's own time split, on the latents that stay inside the format (where an overflowing one turns inf / NaN is each path's own)
        rt = 1e-10 if dtype == torch.float64 else 2e-4
        tm = torch.from_numpy(tame).cuda()
        ok = torch.isfinite(y0[:, :T]) & tm[:, None]
        assert torch.equal(torch.isfinite(yh[:, :T]) & tm[:, None], ok), mode
        sc = torch.where(ok, y0[:, :T], torch.zeros_like(y0[:, :T])).abs().amax(dim=1, keepdim=True) + 1e-30
        assert (torch.where(ok, yh[:, :T] - y0[:, :T], torch.zeros_like(y0[:, :T])).abs() / sc).max().item() < rt, mode
        fin = torch.isfinite(n0) & tm
        assert rel_err(nll[fin].cpu().numpy(), n0[fin].cpu().numpy()) < rt and rel_err(nb[fin].cpu().numpy(), n0[fin].cpu().numpy()) < rt, mode
        assert (torch.where(ok, yc[:, :T] - yh[:, :T], torch.zeros_like(y0[:, :T])).abs() / sc).max().item() < rt, mode


@pytest.mark.parametrize("kern", ["Matern52", "Matern32"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,nanf", [(3, 17, 0.0), (5, 2049, 0.02), (1030, 2100, 0.0), (1100, 4500, 0.001), (1025, 1024, 0.3), (40, 9000, 0.0)])
def test_reference_models_through_the_stacked_kernels_vs_oracle(env, kern, dtype, L, T, nanf):
    """Option filter_plain_x = 1: Matern-3/2 and -5/2 through every kernel of the stacked filter with one component (tables rebuilt from the CB
    blocks: xc_from_cb_kernel) -- the many-latent sweep and its second pass for gaps, the time split, the team kernels -- against the oracle."""
    rng = np.random.default_rng(7 * L + T)
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    bank.set_option("filter_plain_x", 1)
    Ty = synth(L, T, rng, nan_frac=nanf)
    x0 = 0.3 * rng.standard_normal((L, bank.d))
    sub = np.arange(L) if L <= 64 else np.sort(rng.choice(L, size=48, replace=False))
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm[sub]), np.ascontiguousarray(Ty[sub]), x0=x0[sub], nthreads=4)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    tol = (FP64_TIGHT if dtype == torch.float64 else FP32_TOL) * 10
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0, posinf=np.inf).max(axis=1) < (1e100 if dtype == torch.float64 else 1e12)
    assert tame.sum() >= len(sub) // 2
    yg = yhat[:, :T].cpu().numpy().astype(np.float64)[sub][tame]
    assert rel_err_rows(yg, o["yhat"][tame]) < tol
    assert rel_err(xT.cpu().numpy()[sub][tame], o["x"][tame]) < tol and rel_err(nll.cpu().numpy()[sub][tame], o["nll_per_latent"][tame]) < tol


@pytest.mark.parametrize("kern,dtype", [("Matern52x2", torch.float64), ("Matern52x4", torch.float64), ("Matern32x3", torch.float32)])
def test_stacked_time_split_matches_unsplit(env, kern, dtype, monkeypatch):
    """Few latents: the stream is cut into time slices that start from a zero state after a warm-up (recursion_x.hip).  Same
    results as the unsplit sweep to rounding, including latents that decay too slowly for the warm-up argument (long lengthscale
    and tiny noise: those are run whole) and streams with missing ticks."""
    J = int(kern[-1])
    rng = np.random.default_rng(21 + J)
    L, T = 12, 9000
    prm = synth_params_stacked(L, J, rng)
    prm[0, 1::2][:J] = 90.0; prm[0, -1] = 1e-3          # slow latent: lengthscales 90, noise 1e-3
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    Ty = synth(L, T, rng)
    Ty[3, rng.random(T) < 0.02] = np.nan
    Tyd = to_dev(Ty, dtype)
    x0 = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(dtype).cuda()
    bank.set_option("filter_split", 1)
    y1, x1, n1 = bank.filter(Tyd, T=T, x=x0.clone())
    torch.cuda.synchronize()
    for ns in ("0", "3", "5"):
        bank.set_option("filter_split", int(ns))
        y2, x2, n2 = bank.filter(Tyd, T=T, x=x0.clone())
        torch.cuda.synchronize()
        tol = 1e-12 if dtype == torch.float64 else 1e-5
        ok = torch.isfinite(y1[:, :T])
        assert torch.equal(torch.isfinite(y2[:, :T]), ok)
        d = ((y2[:, :T] - y1[:, :T])[ok]).abs().max().item() / y1[:, :T][ok].abs().max().item()
        assert d < tol, (ns, d)
        assert rel_err(x2.cpu().numpy(), x1.cpu().numpy()) < tol and rel_err(n2.cpu().numpy(), n1.cpu().numpy()) < tol
        # the other output combinations (their own kernel instantiations): state only, NLL only, means only
        _, x3, _ = bank.filter(Tyd, T=T, x=x0.clone(), want_yhat=False, want_nll=False)
        _, x4, n4 = bank.filter(Tyd, T=T, x=x0.clone(), want_yhat=False)
        y5, x5, _ = bank.filter(Tyd, T=T, x=x0.clone(), want_nll=False)
        torch.cuda.synchronize()
        for xx in (x3, x4, x5):
            assert rel_err(xx.cpu().numpy(), x1.cpu().numpy()) < tol
        assert rel_err(n4.cpu().numpy(), n1.cpu().numpy()) < tol
        assert ((y5[:, :T] - y1[:, :T])[ok]).abs().max().item() / y1[:, :T][ok].abs().max().item() < tol
    o = env["cref"].filter_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0.double().cpu().numpy(), nthreads=4)
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6     # (the slow latent may be unstable under the literal DARE)
    yg, yo = y2[:, :T].cpu().numpy()[tame], o["yhat"][tame]
    okn = np.isfinite(yo)
    assert np.abs((yg - yo)[okn]).max() / np.abs(yo[okn]).max() < tol
    assert rel_err(n2.cpu().numpy()[tame], o["nll_per_latent"][tame]) < tol


# ------------------------------------------------------------------------------------------ seeded fuzz over shapes and gaps
def _fuzz_cases(n, seed):
    rng = np.random.default_rng(seed)
    kerns = ["Matern32", "Matern52", "Matern52x2", "Matern32x3", "Matern52x4"]
    out = []
    for i in range(n):
        T = int(rng.choice([0, 1, 2, 15, 16, 17, 31, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4100, int(rng.integers(1, 6000))]))
        out.append((kerns[i % len(kerns)], int(rng.integers(1, 48)), T, float(rng.choice([0.0, 0.0, 0.01, 0.3, 1.0])),
                    "f64" if rng.random() < 0.5 else "f32", int(rng.integers(0, 2 ** 31))))
    return out


@pytest.mark.parametrize("kern,L,T,nanf,dt_,seed", _fuzz_cases(200, 20260101))
def test_filter_fuzz_vs_oracle(env, kern, L, T, nanf, dt_, seed):
    """Random latent counts, lengths around every segment / chunk boundary, missing-data rates from none to all, random
    start states, both precisions, reference and stacked models: filtered means, final state and NLL against the oracle."""
    rng = np.random.default_rng(seed)
    dtype = torch.float64 if dt_ == "f64" else torch.float32
    stacked = "x" in kern
    prm = synth_params_stacked(L, int(kern[-1]), rng) if stacked else synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern if stacked else KMAP[kern])
    igps = env["cref"].ihgp_array(kern, 0.1, prm)
    x0 = 0.3 * rng.standard_normal((L, bank.d))
    if T == 0:
        _, xT, nll = bank.filter(torch.zeros((L, 4), dtype=dtype, device="cuda"), T=0, x=torch.from_numpy(x0).to(dtype).cuda())
        torch.cuda.synchronize()
        assert rel_err(xT.cpu().numpy(), x0) < 1e-6 and float(nll.abs().sum()) == 0.0
        return
    Ty = synth(L, T, rng, nan_frac=nanf if nanf < 1.0 else 0.0)
    if nanf >= 1.0:
        Ty[:] = np.nan
    o = env["cref"].filter_stream(igps, Ty, x0=x0, nthreads=4)
    yhat, xT, nll = bank.filter(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda())
    torch.cuda.synchronize()
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    yo = o["yhat"]
    tame = np.nan_to_num(np.abs(yo), nan=0.0, posinf=np.inf).max(axis=1) < (1e100 if dtype == torch.float64 else 1e20)   # literal-DARE unstable latents aside
    if not tame.any():
        return
    yg = yhat[:, :T].cpu().numpy()
    scale = max(np.abs(yo[tame]).max(), 1e-300)
    assert np.abs(yg[tame] - yo[tame]).max() / scale < tol * 10, (kern, L, T, nanf, dt_)
    # ... and row by row among the latents that stay calm: one unstable latent at 1e16 sets a global scale behind which a wrong ordinary latent hides
    # (round 4: an imputed latent with an error of 8e11 passed the line above; only its NLL gave it away)
    calm = np.nan_to_num(np.abs(yo), nan=0.0, posinf=np.inf).max(axis=1) < 1e3
    if calm.any():
        assert rel_err_rows(yg[calm].astype(np.float64), yo[calm]) < tol * 10, (kern, L, T, nanf, dt_)
    xscale = max(np.abs(o["x"][tame]).max(), 1e-6 * np.abs(x0).max())         # (an all-missing stream decays the state to ~0)
    assert np.abs(xT.cpu().numpy()[tame] - o["x"][tame]).max() / xscale < tol * 10
    # (the kernel sums v^2 per chunk in the stream's precision: a trajectory beyond ~1e18 squares out of fp32's range, where the
    # fp64 reference still holds a finite 1e38-sized NLL -- seen for literal-DARE unstable latents that a 2048-tick stream
    # carries to 5e19, and for one at 9.8e16 whose reference NLL is 1.8e39 (fuzz campaign, seed 203635316); such latents are compared
    # on their means and state only)
    ntame = tame & (np.nan_to_num(np.abs(yo), nan=0.0, posinf=np.inf).max(axis=1) < (1e100 if dtype == torch.float64 else 1e16))
    if ntame.any():
        nscale = max(np.abs(o["nll_per_latent"][ntame]).max(), 1e-300)
        assert np.abs(nll.cpu().numpy()[ntame] - o["nll_per_latent"][ntame]).max() / nscale < tol * 10


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("T,gaps", [(2600, [0]), (2600, [1300]), (2600, [2599]), (2600, [511, 512, 1023, 1024]), (3072, [100, 2000, 3071]),
                                    (4100, list(range(1030, 1100))), (1500, [7, 1400]), (5000, "dense")])
def test_gradstream_gaps_in_chosen_segments(env, dtype, kern, T, gaps):
    """Long streams (several 512- / 1024-tick segments) with missing ticks at chosen places: the second pass of the gradient sweep
    walks only the segments that hold a gap tick by tick (ihgp.h:37-48) and scans the others, so the carried (x, dx), the split
    gradient sums and the means written from either path must join: first tick, last tick, both sides of a segment boundary, a run
    of gaps, the ragged tail, a gap in every segment.  Latent 0 stays clean (first pass only), latent 1 has every tick missing."""
    L = 5
    rng = np.random.default_rng(T * 3 + (1 if kern == "Matern52" else 0) + (len(gaps) if gaps != "dense" else 99))
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=KMAP[kern])
    d = bank.d
    Ty = synth(L, T, rng)
    if gaps == "dense":
        Ty[2:, ::97] = np.nan
    else:
        Ty[2:, gaps] = np.nan
    Ty[1, :] = np.nan
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, 3, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    for want in (True, False):
        r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=want)
        torch.cuda.synchronize()
        if want:
            assert rel_err_rows(r["yhat"][:, :T].cpu().numpy(), o["yhat"]) < tol
        assert rel_err(r["x"].cpu().numpy(), o["x"]) < tol and rel_err(r["dx"].cpu().numpy(), o["dx"]) < tol * 10
        assert rel_err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol
        assert rel_err(r["grad"].cpu().numpy(), o["grad"]) < tol * 10
    assert float(r["nll"][1]) == 0.0 and float(r["grad"][1].abs().max()) == 0.0      # nothing observed: no loss, no gradient


def _grad_fuzz_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = int(rng.choice([1, 2, 7, 8, 9, 16, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1500, int(rng.integers(1, 2500))]))
        out.append((["Matern32", "Matern52"][i % 2], int(rng.integers(1, 40)), T, float(rng.choice([0.0, 0.0, 0.02, 0.4])),
                    "f64" if rng.random() < 0.5 else "f32", int(rng.integers(0, 2 ** 31))))
    return out


@pytest.mark.parametrize("kern,L,T,nanf,dt_,seed", _grad_fuzz_cases(80, 77))
def test_gradstream_fuzz_vs_oracle(env, kern, L, T, nanf, dt_, seed):
    """The sensitivity / gradient sweep (A2 + A5) over random shapes around its chunk boundaries, with and without gaps."""
    rng = np.random.default_rng(seed)
    dtype = torch.float64 if dt_ == "f64" else torch.float32
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=KMAP[kern])
    d = bank.d
    Ty = synth(L, T, rng, nanf)
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, 3, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=True)
    torch.cuda.synchronize()
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6           # literal-DARE unstable latents aside
    if not tame.any():
        return
    def err(a, b, floor=0.0):
        return float(np.abs(a[tame] - b[tame]).max() / max(np.abs(b[tame]).max(), floor, 1e-300))
    assert err(r["yhat"][:, :T].cpu().numpy(), o["yhat"]) < tol
    assert err(r["x"].cpu().numpy(), o["x"]) < tol and err(r["dx"].cpu().numpy(), o["dx"], 1e-6) < tol * 10
    assert err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol
    assert err(r["grad"].cpu().numpy(), o["grad"], 1e-6) < tol * 10


def _abi_fuzz_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(1, 40))
        M = L + int(rng.choice([0, 0, 1, 3, int(rng.integers(0, 120))]))
        out.append((["Matern32", "Matern52"][i % 2], M, L, i % 3 != 0, int(rng.integers(0, 2 ** 31))))
    return out


@pytest.mark.parametrize("kern,M,L,fused,seed", _abi_fuzz_cases(45, 5))
def test_reference_abi_fuzz_vs_oracle(env, kern, M, L, fused, seed, monkeypatch):
    """The 26-symbol reference ABI over random model sizes on both of its device paths (single-workgroup fused kernels for small
    models, the multi-kernel path otherwise or when MOIHGP_TICK_FUSED=0): every step overload, both likelihood overloads, a
    missing-output tick, states fed forward like the reference's callers do."""
    if not fused:
        monkeypatch.setenv("MOIHGP_TICK_FUSED", "0")
    rng = np.random.default_rng(seed)
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    ref = env["cref"].GP(0.1, M, L, kern)
    ref.set_literal_ugrad(0)
    d, P = gp.igp_dim, 3
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [rng.uniform(0.01, 0.1)], synth_params(L, rng).ravel()])
    gp.update(params); ref.update(params)
    assert rel_err(gp.params, ref.params) < FP64_TIGHT
    x, dx = 0.5 * rng.standard_normal((L, d)), 0.1 * rng.standard_normal((L, P, d))
    for t in range(4):
        y = rng.standard_normal(M)
        l1, g1 = gp.negLogLikelihood(x, y, dx); l2, g2 = ref.negLogLikelihood(x, y, dx)
        assert abs(l1 - l2) < FP64_TIGHT * max(1.0, abs(l2)) and rel_err(g1, g2) < 1e-8
        assert abs(gp.negLogLikelihood(x, y) - ref.negLogLikelihood(x, y)) < FP64_TIGHT * max(1.0, abs(l2))
        a = gp.step(x, y, dx); b = ref.step(x, y, dx)                      # overload 1
        for u, v in zip(a, b):
            assert rel_err(u, v) < FP64_TIGHT
        a3 = gp.step(x, y); b3 = ref.step(x, y)                            # overload 3
        assert rel_err(a3[0], b3[0]) < FP64_TIGHT and rel_err(a3[1], b3[1]) < FP64_TIGHT
        if t == 1:
            a4 = gp.step(x); b4 = ref.step(x)                              # overload 4 (prediction only)
            assert rel_err(a4[0], b4[0]) < FP64_TIGHT and rel_err(a4[1], b4[1]) < FP64_TIGHT
        if t == 2 and M > L:
            ym = y.copy(); ym[rng.choice(M, size=max(1, (M - L) // 2), replace=False)] = np.nan
            am = gp.step(x, ym); bm = ref.step(x, ym)                      # least-squares projection over the observed rows
            assert rel_err(am[0], bm[0]) < 1e-7 and rel_err(am[1], bm[1]) < 1e-7
        x, dx = a[0], a[2]


@pytest.mark.parametrize("kern", STACKED)
def test_stacked_sensitivities_vs_oracle(env, kern):
    """IHGP::update's derivative part (ihgp.h:136-200) for stacked models: dA, dAKHA, dK, dS, HdA per hyper-parameter and the
    DLyap iteration counts against the C oracle (bitwise for Matern-3/2 stacks; the Matern-5/2 ones differ by the block-wise
    matrix exponential)."""
    J = int(kern[-1])
    rng = np.random.default_rng(40 + J)
    L = 5
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    for l in range(L):
        m = bank.latent(l)
        c = env["cref"].ihgp_update(kern, 0.1, prm[l])
        for k in ("dA", "dAKHA", "dK", "dS", "HdA"):
            assert rel_err(m[k], c.mat(k)) < 1e-11, (k, rel_err(m[k], c.mat(k)))
        assert m["iters"][0] == c.dare_iters and list(m["iters"][1:]) == list(c.dlyap_iters)[:2 * J + 1]


@pytest.mark.parametrize("kern", STACKED)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,nanf", [(3, 1, 0.0), (5, 64, 0.0), (4, 65, 0.0), (7, 130, 0.05), (2, 700, 0.0)])
def test_stacked_gradstream_vs_oracle(env, kern, dtype, L, T, nanf):
    J = int(kern[-1])
    rng = np.random.default_rng(9 * L + T + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    d, P = bank.d, bank.P
    Ty = synth(L, T, rng, nanf)
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, P, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=True)
    torch.cuda.synchronize()
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6
    if not tame.any():
        return
    def err(a, b, floor=0.0):
        return float(np.abs(a[tame] - b[tame]).max() / max(np.abs(b[tame]).max(), floor, 1e-300))
    assert err(r["yhat"][:, :T].cpu().numpy(), o["yhat"]) < tol
    assert err(r["x"].cpu().numpy(), o["x"]) < tol and err(r["dx"].cpu().numpy(), o["dx"], 1e-6) < tol * 10
    assert err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol * 10
    assert err(r["grad"].cpu().numpy(), o["grad"], 1e-6) < tol * 10


@pytest.mark.parametrize("kern", STACKED)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,gap", [(3, 512, None), (2, 543, None), (5, 2048, None), (3, 2081, None), (2, 4133, None), (3, 6500, None),
                                     (4, 2500, 1700), (3, 1024, 0), (3, 4500, [0, 31, 32, 2047, 2048, 4499]), (3, 5000, "dense")])
def test_stacked_gradstream_long_streams_vs_oracle(env, kern, dtype, L, T, gap):
    """Streams of >= 512 ticks take the time-parallel sweep of the stacked models (grad_scan_x.hip: innovation-form sensitivity
    recursion, chunk-local sensitivities scanned with the filter's own powers): whole 32-tick chunks there, the last T mod 32 ticks
    in the tick-by-tick kernel, which must continue seamlessly; a segment with a missing tick (gap: NaNs in latents 1..) is walked
    tick by tick inside the sweep (all P + 1 vectors in registers) between segments solved in parallel.  Exactly one segment, one chunk past a segment, several segments, ragged ends."""
    J = int(kern[-1])
    rng = np.random.default_rng(11 * L + T + J)
    prm = synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern)
    d, P = bank.d, bank.P
    Ty = synth(L, T, rng)
    if isinstance(gap, str):
        Ty[1:, ::37] = np.nan                               # a gap in every segment (and most chunks)
        Ty[2, :] = np.nan                                   # nothing observed at all
    elif gap is not None:
        Ty[1:, gap] = np.nan
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, P, d))
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, prm), Ty, x0=x0, dx0=dx0)
    tol = 1e-9 if dtype == torch.float64 else FP32_TOL
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6
    if not tame.any():
        return
    def err(a, b, floor=0.0):
        return float(np.abs(a[tame] - b[tame]).max() / max(np.abs(b[tame]).max(), floor, 1e-300))
    for want in (True, False):
        r = bank.grad(to_dev(Ty, dtype), T=T, x=torch.from_numpy(x0).to(dtype).cuda(), dx=torch.from_numpy(dx0).to(dtype).cuda(), want_yhat=want)
        torch.cuda.synchronize()
        if want:
            assert err(np.nan_to_num(r["yhat"][:, :T].cpu().numpy()), np.nan_to_num(o["yhat"])) < tol
        assert err(r["x"].cpu().numpy(), o["x"]) < tol and err(r["dx"].cpu().numpy(), o["dx"], 1e-6) < tol * 10
        assert err(r["nll"].cpu().numpy(), o["nll_per_latent"]) < tol * 10
        assert err(r["grad"].cpu().numpy(), o["grad"], 1e-6) < tol * 10


@pytest.mark.parametrize("kern", ["Matern32x2", "Matern52x2", "Matern52x4"])
def test_stacked_gradient_tables_follow_every_update(env, kern):
    """The time-parallel gradient sweep of the stacked models reads per-latent tables that depend on the hyper-parameters
    (gp_table_kernel).  They are rebuilt by every update -- not by the first long sweep after it: update(p2), a SHORT sweep
    (below the 512-tick threshold: tick-by-tick kernel, touches no table), then a LONG sweep must use p2's tables; and a long
    sweep issued on a side stream right behind an update must find them complete.  Compared with a fresh handle built at p2
    and with the oracle."""
    J = int(kern[-1])
    rng = np.random.default_rng(77 + J)
    L, Tl, Ts = 5, 4096, 100
    p1, p2 = synth_params_stacked(L, J, rng), synth_params_stacked(L, J, rng)
    bank = env["streams"].LatentBank(0.1, p1, kernel=kern)
    d, P = bank.d, bank.P
    Ty = synth(L, Tl, rng)
    dev = to_dev(Ty, torch.float64)
    def sweep(b, T, stream=None):
        x = torch.zeros((L, d), dtype=torch.float64, device="cuda"); dx = torch.zeros((L, P, d), dtype=torch.float64, device="cuda")
        if stream is None:
            r = b.grad(dev, T=T, x=x, dx=dx, want_yhat=False)
        else:
            with torch.cuda.stream(stream):
                r = b.grad(dev, T=T, x=x, dx=dx, want_yhat=False)
        torch.cuda.synchronize()
        return r
    sweep(bank, Tl)                                  # tables of p1 now exist
    bank.update(p2)
    sweep(bank, Ts)                                  # short sweep: no table involved
    r = sweep(bank, Tl)                              # must see p2's tables
    fresh = env["streams"].LatentBank(0.1, p2, kernel=kern)
    f = sweep(fresh, Tl)
    o = env["cref"].grad_stream(env["cref"].ihgp_array(kern, 0.1, p2), Ty)
    tame = np.abs(o["yhat"]).max(axis=1) < 1e6
    assert tame.any()
    for key, ok in (("grad", "grad"), ("nll", "nll_per_latent"), ("x", "x")):
        a, b, c = r[key].cpu().numpy()[tame], f[key].cpu().numpy()[tame], o[ok][tame]
        assert np.array_equal(a, b), key
        assert np.abs(a - c).max() <= 1e-8 * max(np.abs(c).max(), 1e-6), key
    # straight behind an update, on a side stream
    side = torch.cuda.Stream()
    bank.update(p1); bank.update(p2)
    r2 = sweep(bank, Tl, side)
    assert np.array_equal(r2["grad"].cpu().numpy()[tame], f["grad"].cpu().numpy()[tame])


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T,nanf", [(1030, 1024, 0.0), (1500, 5000, 0.0), (1100, 4097, 0.0), (1200, 777, 0.0), (1300, 3000, 0.01), (5, 2100, 0.0), (1024, 1, 0.0)])
def test_segment_major_streams_equal_series_major(env, kern, dtype, L, T, nanf):
    """moihgp_filter_stream_tiled sweeps the same ticks with the same arithmetic as the series-major entry -- only the addresses differ
    ([ceil(T / SEG)][L][SEG] instead of [L][ld]) -- so filtered means, end states and per-latent NLLs are equal BIT FOR BIT: whole and ragged
    last tiles, a single tick, missing ticks (generic path), unstable latents (sequential kernel), a separate start state, the NLL total;
    and the series-major result is the one the rest of this file checks against the oracle.  moihgp_stream_retile round-trips."""
    S = env["streams"]
    rng = np.random.default_rng(3 * L + T)
    prm = synth_params(L, rng)
    bank = S.LatentBank(0.1, prm, kernel=KMAP[kern])
    Ty = synth(L, T, rng, nanf)
    dev = to_dev(Ty, dtype)
    x0 = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(dtype).cuda()
    ya, xa, na = bank.filter(dev, T=T, x=torch.zeros_like(x0), x_start=x0)
    tot_a = torch.zeros(1, dtype=torch.float64, device="cuda"); tot_b = torch.zeros_like(tot_a)
    bank.filter(dev, T=T, x=torch.zeros_like(x0), x_start=x0, nll_total=tot_a)
    tiled = S.tile_stream(dev, T)
    assert tuple(tiled.shape) == ((T + S.seg_ticks(dtype) - 1) // S.seg_ticks(dtype), L, S.seg_ticks(dtype))
    back = S.untile_stream(tiled, T)
    torch.cuda.synchronize()
    a, b = dev[:, :T].cpu().numpy(), back[:, :T].cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True)
    yb_t, xb, nb = bank.filter_tiled(tiled, T, x=torch.zeros_like(x0), x_start=x0, nll_total=tot_b)
    yb = S.untile_stream(yb_t, T)
    torch.cuda.synchronize()
    if L > 1024 or (L > 512 and kern == "Matern32"):
        # both layouts run the one-wavefront-per-latent kernel: the same operations in the same order (Matern-5/2 at up to 1024 latents may take
        # the eight-wavefront team kernel series-major)
        assert np.array_equal(ya[:, :T].cpu().numpy(), yb[:, :T].cpu().numpy(), equal_nan=True)
        assert np.array_equal(xa.cpu().numpy(), xb.cpu().numpy(), equal_nan=True) and np.array_equal(na.cpu().numpy(), nb.cpu().numpy(), equal_nan=True)
        assert np.array_equal(tot_a.cpu().numpy(), tot_b.cpu().numpy(), equal_nan=True)
    else:
        # few latents: the series-major entry splits a latent's stream over the wavefronts of a workgroup (another summation order)
        tol = 1e-11 if dtype == torch.float64 else 2e-4
        tame = np.nan_to_num(np.abs(ya[:, :T].cpu().numpy())).max(axis=1) < 1e6
        assert rel_err(yb[:, :T].cpu().numpy()[tame], ya[:, :T].cpu().numpy()[tame]) < tol
        assert rel_err(xb.cpu().numpy()[tame], xa.cpu().numpy()[tame]) < tol and rel_err(nb.cpu().numpy()[tame], na.cpu().numpy()[tame]) < tol
    # NLL-only and means-only modes
    _, xc, nc = bank.filter_tiled(tiled, T, x=torch.zeros_like(x0), x_start=x0, want_yhat=False)
    yd_t, xd, _ = bank.filter_tiled(tiled, T, x=torch.zeros_like(x0), x_start=x0, want_nll=False)
    torch.cuda.synchronize()
    assert np.array_equal(nc.cpu().numpy(), nb.cpu().numpy(), equal_nan=True) and np.array_equal(xc.cpu().numpy(), xb.cpu().numpy(), equal_nan=True)
    assert np.array_equal(S.untile_stream(yd_t, T)[:, :T].cpu().numpy(), yb[:, :T].cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("kern", ["Matern52", "Matern52x2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_filter_separate_start_state(env, kern, dtype):
    """moihgp_filter_stream_io: the sweep starts from x_start (left untouched) and writes the end state to x -- same results as
    the in-place form, for many latents, few latents (time split) and repeated sweeps."""
    stacked = "x" in kern
    for L, T in ((1100, 1500), (7, 5000)):
        rng = np.random.default_rng(L)
        prm = synth_params_stacked(L, 2, rng) if stacked else synth_params(L, rng)
        bank = env["streams"].LatentBank(0.1, prm, kernel=kern if stacked else KMAP[kern])
        Tyd = to_dev(synth(L, T, rng), dtype)
        x0 = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(dtype).cuda()
        y1, x1, n1 = bank.filter(Tyd, T=T, x=x0.clone())
        keep = x0.clone()
        xo = torch.full_like(x0, 7.0)
        for _ in range(2):
            y2, x2, n2 = bank.filter(Tyd, T=T, x=xo, x_start=x0)
        torch.cuda.synchronize()
        assert torch.equal(x0, keep) and x2.data_ptr() == xo.data_ptr()
        assert torch.equal(x2, x1) and torch.equal(n2, n1) and torch.equal(y2[:, :T], y1[:, :T])


def test_handles_release_their_device_memory(env):
    """gp32_del / moihgp_del free everything the handle allocated (device buffers, pinned staging, stream): creating and dropping
    a few hundred objects of every kind leaves the free device memory where it was."""
    import gc
    def churn(n):
        for i in range(n):
            gp = env["MOIHGP"](0.1, 12, 5, kernel="Matern52ss")
            gp.step(np.zeros((5, 3)), np.ones(12))
            bank = env["streams"].LatentBank(0.1, [[1, 1, 1, 2, 0.1]] * 8, kernel="Matern52x2")
            Ty = torch.zeros((8, 64), dtype=torch.float64, device="cuda")
            bank.filter(Ty, T=64); bank.grad(Ty, T=64)
            del gp, bank, Ty
        gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
    churn(20)
    free0, _ = torch.cuda.mem_get_info()
    churn(200)
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 32 * 1024 * 1024, (free0, free1)


@pytest.mark.parametrize("kern,L,T", [("Matern52", 4096, 3000), ("Matern52", 1500, 700), ("Matern52", 37, 5000), ("Matern32", 1025, 100), ("Matern52x2", 1100, 2100), ("Matern52x2", 9, 4100)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_nll_total_from_the_sweep(env, kern, L, T, dtype):
    """moihgp_filter_stream_io's nll_total: the sum of the per-latent NLLs left on the device by a one-wavefront kernel queued
    behind the sweep (every path: many / few latents, reference and stacked models), repeated launches."""
    stacked = "x" in kern
    rng = np.random.default_rng(L + T)
    prm = synth_params_stacked(L, 2, rng) if stacked else synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern if stacked else KMAP[kern])
    Tyd = to_dev(synth(L, T, rng), dtype)
    tot = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    for rep in range(3):
        _, _, nll = bank.filter(Tyd, T=T, nll_total=tot)
        torch.cuda.synchronize()
        ref = nll.sum().item()
        assert abs(tot.item() - ref) <= 1e-12 * abs(ref), (rep, tot.item(), ref)
        tot.fill_(-1.0)


PROFILE_ROUTES = [       # the smallest shapes that still take each route of moihgp_filter_stream_io / _tiled
    ("dma", "Matern52", torch.float32, 1030, 1100, {}),                  # many latents: the LDS-DMA kernel
    ("dma-segment-major", "Matern52", torch.float32, 1030, 1100, {}),
    ("team", "Matern52", torch.float64, 3, 5000, {}),                    # few latents: team kernel / time split
    ("split2", "Matern52", torch.float64, 3, 5000, {"filter_split": 2}),
    ("stacked", "Matern52x2", torch.float32, 1030, 2100, {}),            # first pass plus second
    ("stacked-imputed", "Matern52x2", torch.float32, 1030, 2100, {"filter_impute": 1}),   # 1 % NaN: three passes, the pair rides on the first
    ("stacked-team", "Matern52x2", torch.float64, 3, 2100, {}),
    ("stacked-split2", "Matern52x2", torch.float64, 3, 2100, {"filter_split": 2}),
]


@pytest.mark.parametrize("route,kern,dtype,L,T,opts", PROFILE_ROUTES, ids=[r[0] for r in PROFILE_ROUTES])
def test_profile_event_pairs_on_every_route(env, route, kern, dtype, L, T, opts):
    """moihgp_profile_enable / _read: every sweep carries one event pair around its sweep kernel, whichever route the call takes (bench.py takes
    every kernel time from them).  Two sweeps give two durations, finite and positive, and -- an event pair brackets part of what the host
    waited for -- together they are shorter than the wall-clock time of the two calls between two synchronisations."""
    import time
    stacked = "x" in kern
    rng = np.random.default_rng(L + T)
    prm = synth_params_stacked(L, 2, rng) if stacked else synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel=kern if stacked else KMAP[kern])
    for name, value in opts.items():
        bank.set_option(name, value)
    Tyd = to_dev(synth(L, T, rng, nan_frac=0.01 if route == "stacked-imputed" else 0.0), dtype)
    tiled = route == "dma-segment-major"
    if tiled:
        Tyd = env["streams"].tile_stream(Tyd, T)
    sweep = (lambda: bank.filter_tiled(Tyd, T)) if tiled else (lambda: bank.filter(Tyd, T=T))
    sweep()                                                     # (first-use allocations and tables stay out of the timed pair)
    torch.cuda.synchronize()
    bank.profile_enable(2)
    t0 = time.perf_counter()
    for _ in range(2):
        yhat, _, nll = sweep()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms = bank.profile_read()
    print(f"{route}: event pairs {ms} ms, wall {wall_ms:.3f} ms")
    assert yhat is not None and nll is not None
    assert len(ms) == 2, ms
    assert all(np.isfinite(v) and v > 0 for v in ms), ms
    assert sum(ms) < wall_ms, (ms, wall_ms)


# ------------------------------------------------------------------------------------------ ordering: sweeps in flight vs update()
@pytest.mark.parametrize("kernel,J", [("Matern52ss", 0), ("Matern52x4", 4)])
def test_update_waits_for_sweeps_in_flight(env, kernel, J):
    """A sweep is asynchronous on the caller's stream and reads the per-latent tables; update() rewrites them on the handle's own
    stream.  An update issued right behind queued sweeps must not change their results (include/moihgp.h, ordering contract)."""
    rng = np.random.default_rng(5)
    L, T = 2048, 6000
    P = 2 * J + 1 if J else 3
    def draw():
        cols = [rng.uniform(0.5, 2, L) for _ in range(P - 1)] + [rng.uniform(0.05, 0.2, L)]
        return np.column_stack(cols)
    p_old, p_new = draw(), draw()
    Ty = to_dev(synth(L, T, rng), torch.float64)
    bank = env["streams"].LatentBank(0.1, p_old, kernel=kernel)
    y_ref, x_ref, nll_ref = bank.filter(Ty, T)
    torch.cuda.synchronize()
    y_ref, nll_ref = y_ref.clone(), nll_ref.clone()
    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        for _ in range(6):                                     # a pipeline of sweeps, none of them waited for ...
            outs.append(bank.filter(Ty, T, stream=side))
    bank.update(p_new)                                         # ... and the tables are rewritten right behind them
    y_new, _, nll_new = bank.filter(Ty, T)                     # enqueued after update() returned: sees the new tables
    torch.cuda.synchronize()
    for yh, _, nll in outs:
        assert torch.equal(yh[:, :T], y_ref[:, :T]) and torch.equal(nll, nll_ref)
    fresh = env["streams"].LatentBank(0.1, p_new, kernel=kernel)
    y_f, _, nll_f = fresh.filter(Ty, T)
    torch.cuda.synchronize()
    assert torch.equal(y_new[:, :T], y_f[:, :T]) and torch.equal(nll_new, nll_f)
    assert not torch.equal(nll_new, nll_ref)


# ------------------------------------------------------------------------------------------ additive ABI: output stride, return codes
def test_filtered_means_into_a_buffer_shaped_unlike_the_stream(env):
    """moihgp_filter_stream_v2: yhat has its own row stride.  A column slice of a wide slab as input, a compact array as output (the
    shape that wrote out of bounds through the single-ld entries in round 1), and the other way round."""
    rng = np.random.default_rng(12)
    L, Tw, T0, T = 37, 3000, 1000, 1536
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern52ss")
    wide = to_dev(synth(L, Tw, rng), torch.float32)
    src = wide[:, T0:T0 + T]                                   # row stride 3000, 16-byte aligned start
    guard = torch.full((L * T + 4096,), 777.0, dtype=torch.float32, device="cuda")
    compact = guard[:L * T].view(L, T)                         # row stride T: the tail of `guard` must stay untouched
    y1, x1, n1 = bank.filter(src, T=T, yhat=compact)
    ref_y, ref_x, ref_n = bank.filter(src.contiguous(), T=T)
    torch.cuda.synchronize()
    assert torch.equal(y1, ref_y[:, :T]) and torch.equal(n1, ref_n) and torch.equal(x1, ref_x)
    assert bool((guard[L * T:] == 777.0).all())
    out_wide = torch.full((L, Tw), 555.0, dtype=torch.float32, device="cuda")
    y2, _, _ = bank.filter(src.contiguous(), T=T, yhat=out_wide[:, 500:500 + T])
    torch.cuda.synchronize()
    assert torch.equal(y2, ref_y[:, :T]) and bool((out_wide[:, :500] == 555.0).all()) and bool((out_wide[:, 500 + T:] == 555.0).all())
    # stacked kernels take the same entry
    Ls = 9
    prm_s = np.column_stack([rng.uniform(0.5, 2, Ls), rng.uniform(0.5, 2, Ls), rng.uniform(0.5, 2, Ls), rng.uniform(0.5, 2, Ls), rng.uniform(0.05, 0.2, Ls)])
    bs = env["streams"].LatentBank(0.1, prm_s, kernel="Matern52x2")
    wide_s = to_dev(synth(Ls, Tw, rng), torch.float64)
    src_s = wide_s[:, 1000:1000 + T]
    comp_s = torch.empty((Ls, T), dtype=torch.float64, device="cuda")
    ya, _, na = bs.filter(src_s, T=T, yhat=comp_s)
    yb, _, nb = bs.filter(src_s.contiguous(), T=T)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb[:, :T]) and torch.equal(na, nb)


def test_additive_entries_report_instead_of_aborting(env):
    """Part 2 of include/moihgp.h returns codes: 1 invalid argument, 2 HIP failure, 3 unsupported input; constructors return NULL.
    moihgp_last_error() holds the text.  (The reference entries have no channel and abort, wrapper.cpp:31-326.)"""
    import ctypes as C
    from multioutputihgp_amd._lib import c_double_p, last_error
    lib = env["lib"]
    bank = env["streams"].LatentBank(0.1, [[1, 1, 0.1]] * 8, kernel="Matern32")
    Ty = torch.zeros((8, 64), dtype=torch.float32, device="cuda"); x = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    yh = torch.zeros((8, 64), dtype=torch.float32, device="cuda")
    args = lambda ld_out: (bank._h, 1, C.c_void_p(Ty.data_ptr()), 64, 64, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(yh.data_ptr()), ld_out, None, None, None)
    assert lib.moihgp_filter_stream_v2(*args(62)) == 1 and "ld_out" in last_error(lib)          # not a multiple of 16 bytes
    assert lib.moihgp_filter_stream_v2(*args(32)) == 1 and "ld_out" in last_error(lib)          # shorter than T
    assert lib.moihgp_filter_stream_v2(*args(64)) == 0
    gp = env["MOIHGP"](0.1, 4, 2, kernel="Matern32")
    z = np.zeros(64)
    assert lib.moihgp_window_eval(gp.handle, z.ctypes.data_as(c_double_p), z.ctypes.data_as(c_double_p), z.ctypes.data_as(c_double_p),
                                  z.ctypes.data_as(c_double_p), None, None) == 1                 # no window set
    Yn = np.full((3, 4), np.nan)
    assert lib.moihgp_window_set(gp.handle, Yn.ctypes.data_as(c_double_p), 3) == 3
    assert lib.moihgp_pin_host_buffer(gp.handle, C.c_void_p(8), 1 << 20) == 2                    # HIP refuses: reported, not fatal
    # a device allocation that cannot succeed (2^27 latents: 375 GB of constant blocks): NULL + message, the process lives
    h = lib.moihgp_new_latents(1, C.c_double(0.1), C.c_size_t(1 << 27), None)
    assert not h and "HIP error" in last_error(lib)
    torch.cuda.synchronize()
    yb, _, _ = bank.filter(Ty, T=64)                                                             # and the library still works
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yb).all())


# ------------------------------------------------------------------------------------------ N1: partially observed ticks on the batched path
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kern,M,L,T", [("Matern32", 8, 4, 60), ("Matern52", 96, 64, 300), ("Matern52", 700, 300, 128)])
def test_project_stream_with_missing_outputs(env, dtype, kern, M, L, T):
    """moihgp.h:167-178: a tick with missing outputs (NaN) is projected by least squares over the observed rows.  The stream
    projection does it per affected tick behind its GEMM; checked against the oracle's per-tick projection and, end to end, against
    the per-tick ABI (project -> sweep -> unproject == a loop of gp.step(x, y) with the same NaNs)."""
    rng = np.random.default_rng(M + L + T)
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    ref = env["cref"].GP(0.1, M, L, kern)
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.04], synth_params(L, rng).ravel()])
    gp.update(params); ref.update(params)
    Y = rng.standard_normal((T, M))
    hit = rng.choice(T, size=T // 4, replace=False)
    for t in hit:                                              # 1 .. min(M - L, 40) missing outputs per affected tick
        k = int(rng.integers(1, max(2, min(M - L, 40)) + 1)) if M - L >= 2 else 1
        Y[t, rng.choice(M, size=min(k, M - L), replace=False)] = np.nan
    Yd = torch.from_numpy(Y).to(dtype).cuda()
    Ty = env["streams"].project_stream(gp, Yd)
    torch.cuda.synchronize()
    want = np.stack([ref.project(Y[t]) for t in range(T)], axis=1)            # [L, T]
    got = Ty[:, :T].double().cpu().numpy()
    assert np.isfinite(got).all()
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    assert rel_err(got, want) < tol
    assert rel_err(got[:, hit], want[:, hit]) < tol
    if dtype == torch.float64:
        bank = env["streams"].LatentBank.from_handle(gp)
        yl, xT, _ = bank.filter(Ty, T=T)
        Yhat = env["streams"].unproject_stream(gp, yl, T)
        torch.cuda.synchronize()
        x = np.zeros((L, gp.igp_dim)); out = np.empty((T, M))
        for t in range(min(T, 80)):
            x, out[t] = gp.step(x, Y[t])
        assert rel_err(Yhat[:min(T, 80)].cpu().numpy(), out[:min(T, 80)]) < 1e-9


def test_project_stream_missing_outputs_beyond_the_least_squares_path(env):
    """More than 64 missing outputs, or fewer observed outputs than latents: the column stays NaN (the tick is then a missing tick for the
    recursion); a mixing without orthonormal columns (moihgp_set_mixing with an arbitrary matrix) switches the path off."""
    import ctypes as C
    from multioutputihgp_amd._lib import c_double_p
    rng = np.random.default_rng(3)
    M, L, T = 200, 100, 10
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    Y = rng.standard_normal((T, M))
    Y[2, :70] = np.nan                                         # 70 missing > 64
    Y[5, :101] = np.nan                                        # 99 observed < L
    Y[7, 3] = np.nan
    Ty = env["streams"].project_stream(gp, torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    bad = torch.isnan(Ty[:, :T]).all(dim=0).cpu().numpy()
    assert list(np.nonzero(bad)[0]) == [2, 5] and bool(torch.isfinite(Ty[:, 7]).all())
    U = np.ascontiguousarray(np.eye(M, L) + 0.3 * rng.standard_normal((M, L))); S = np.ones(L)
    assert env["lib"].moihgp_set_mixing(gp.handle, U.ctypes.data_as(c_double_p), S.ctypes.data_as(c_double_p), C.c_double(0.01)) == 0
    Ty2 = env["streams"].project_stream(gp, torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    assert bool(torch.isnan(Ty2[:, 7]).all())                  # not orthonormal: NaN propagates as documented
    Q, _ = np.linalg.qr(U); Q = np.ascontiguousarray(Q)
    assert env["lib"].moihgp_set_mixing(gp.handle, Q.ctypes.data_as(c_double_p), S.ctypes.data_as(c_double_p), C.c_double(0.01)) == 0
    Ty3 = env["streams"].project_stream(gp, torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    y7 = Y[7].copy(); obs = ~np.isnan(y7)
    a = np.linalg.solve(Q[obs].T @ Q[obs], Q[obs].T @ y7[obs])
    assert rel_err(Ty3[:, 7].cpu().numpy(), a) < 1e-10


# ------------------------------------------------------------------------------------------ round 3: options, stream release, device vectors
def test_options_and_stream_release(env):
    """moihgp_set_option: per-handle hooks (nothing reads the environment per launch); the kernel tiling probes are not in the shipped library.
    moihgp_release_stream: a caller may destroy a stream that carried batched work once it has handed it back."""
    import ctypes as C
    lib = env["lib"]
    rng = np.random.default_rng(5)
    L, T = 8, 3000
    prm = synth_params(L, rng)
    bank = env["streams"].LatentBank(0.1, prm, kernel="Matern52ss")
    assert lib.moihgp_set_option(bank._h, b"filter_split", 3) == 0 and lib.moihgp_set_option(bank._h, b"filter_split", 0) == 0
    assert lib.moihgp_set_option(bank._h, b"no_such_option", 1) == 1
    assert lib.moihgp_set_option(bank._h, b"filter_variant", 0) == 0
    assert lib.moihgp_set_option(bank._h, b"filter_variant", 9) == 1          # the staging-only probe (no arithmetic) exists in tuning builds only
    assert lib.moihgp_set_option(bank._h, b"filter_split", 1000) == 1
    Ty = synth(L, T, rng)
    o = env["cref"].filter_stream(env["cref"].ihgp_array("Matern52", 0.1, prm), Ty)
    side = torch.cuda.Stream()
    Tyd = to_dev(Ty, torch.float64)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        yhat, xT, nll = bank.filter(Tyd, T=T, stream=side)
    assert lib.moihgp_release_stream(bank._h, C.c_void_p(side.cuda_stream)) == 0
    bank.update(prm * 1.1)                                                     # ordered behind the sweep on the released stream; must not touch it again
    side.synchronize()
    assert rel_err_rows(yhat[:, :T].cpu().numpy(), o["yhat"]) < FP64_TIGHT
    del side
    prm2 = prm * 1.1
    o2 = env["cref"].filter_stream(env["cref"].ihgp_array("Matern52", 0.1, prm2), Ty)
    y2, _, _ = bank.filter(Tyd, T=T)
    torch.cuda.synchronize()
    assert rel_err_rows(y2[:, :T].cpu().numpy(), o2["yhat"]) < FP64_TIGHT


def test_device_vector_blocks_are_kept_for_reuse(env):
    """moihgp_dvec_alloc / _free (csrc/vecops.hip): a freed block of 1 MB or more is handed out again for the next allocation of its size
    (the optimiser frees and allocates its correction pairs at every solve), smaller ones go back to the driver, moihgp_dvec_trim empties
    the cache; a reused block is ordinary device memory."""
    import ctypes as C
    lib = env["lib"]
    lib.moihgp_dvec_alloc.restype = C.c_void_p; lib.moihgp_dvec_alloc.argtypes = [C.c_size_t]
    lib.moihgp_dvec_free.restype = None; lib.moihgp_dvec_free.argtypes = [C.c_void_p]
    lib.moihgp_dvec_trim()
    n = 1 << 18                                           # 2 MB
    p1 = lib.moihgp_dvec_alloc(n); p2 = lib.moihgp_dvec_alloc(n)
    assert p1 and p2 and p1 != p2
    lib.moihgp_dvec_free(p1)
    p3 = lib.moihgp_dvec_alloc(n)
    assert p3 == p1                                       # the kept block
    p4 = lib.moihgp_dvec_alloc(n)
    assert p4 and p4 not in (p1, p2)
    t = torch.arange(n, dtype=torch.float64, device="cuda")
    ctx = lib.moihgp_dvec_ctx_new()
    back = torch.empty_like(t)
    torch.cuda.synchronize()                              # (t was filled on torch's stream; the copies below run on the context's own)
    assert lib.moihgp_dvec_copy(C.c_void_p(ctx), C.c_void_p(p3), C.c_void_p(t.data_ptr()), C.c_size_t(n)) == 0
    assert lib.moihgp_dvec_copy(C.c_void_p(ctx), C.c_void_p(back.data_ptr()), C.c_void_p(p3), C.c_size_t(n)) == 0
    assert lib.moihgp_dvec_sync(ctx) == 0 and torch.equal(back, t)
    lib.moihgp_dvec_ctx_del(ctx)
    for p in (p2, p3, p4): lib.moihgp_dvec_free(p)
    lib.moihgp_dvec_trim()
    q = lib.moihgp_dvec_alloc(n)                          # after the trim: a fresh block from the driver (may or may not be the same address)
    assert q
    lib.moihgp_dvec_free(q)
    s1 = lib.moihgp_dvec_alloc(16); lib.moihgp_dvec_free(s1)      # small: not kept, nothing to check but that it works
    lib.moihgp_dvec_trim()


def test_device_vector_kernels_vs_numpy(env):
    """csrc/vecops.hip (moihgp_dvec_*): the vector kernels of the device-resident optimiser against numpy, sizes that span one and many
    reduction workgroups, with and without the free-variable mask."""
    import ctypes as C
    lib = env["lib"]
    dp = C.POINTER(C.c_double)
    lib.moihgp_dvec_ctx_new.restype = C.c_void_p
    lib.moihgp_dvec_ctx_del.argtypes = [C.c_void_p]
    ctx = lib.moihgp_dvec_ctx_new()
    assert ctx
    rng = np.random.default_rng(2)
    for n in (1, 257, 70001, 1 << 20):
        a, b, g = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        lb, ub = -0.5 * np.ones(n), 0.7 * np.ones(n)
        lb[::7] = ub[::7] = 0.1                                                # fixed variables
        x = np.clip(rng.standard_normal(n), lb, ub)
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        ta, tb, tg, tx, tl, tu = (torch.from_numpy(v).cuda() for v in (a, b, g, x, lb, ub))
        tm = torch.from_numpy(mask).cuda()
        P = lambda t: C.c_void_p(t.data_ptr())
        r = C.c_double()
        assert lib.moihgp_dvec_dot(C.c_void_p(ctx), C.c_size_t(n), P(ta), P(tb), None, C.byref(r)) == 0
        assert abs(r.value - a @ b) <= 1e-12 * max(1.0, np.abs(a * b).sum())
        assert lib.moihgp_dvec_dot(C.c_void_p(ctx), C.c_size_t(n), P(ta), P(tb), P(tm), C.byref(r)) == 0
        assert abs(r.value - (a * b)[mask > 0].sum()) <= 1e-12 * max(1.0, np.abs(a * b).sum())
        r1 = C.c_double(); lib.moihgp_dvec_dot(C.c_void_p(ctx), C.c_size_t(n), P(ta), P(tb), P(tm), C.byref(r1))
        assert r1.value == r.value                                              # deterministic
        free = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.moihgp_dvec_active_set(C.c_void_p(ctx), C.c_size_t(n), P(tx), P(tg), P(tl), P(tu), P(free)) == 0
        lib.moihgp_dvec_sync(C.c_void_p(ctx))
        want_free = ~(((x <= lb) & (g > 0)) | ((x >= ub) & (g < 0)) | (lb == ub))
        assert np.array_equal(free.cpu().numpy().astype(bool), want_free)
        xt = torch.empty(n, dtype=torch.float64, device="cuda")
        dec = C.c_double()
        assert lib.moihgp_dvec_proj_step(C.c_void_p(ctx), C.c_size_t(n), P(tx), P(ta), C.c_double(0.3), P(tl), P(tu), P(tg), P(xt), C.byref(dec)) == 0
        want_xt = np.clip(x + 0.3 * a, lb, ub)
        assert np.abs(xt.cpu().numpy() - want_xt).max() < 1e-14
        assert abs(dec.value - g @ (want_xt - x)) <= 1e-12 * max(1.0, np.abs(g * (want_xt - x)).sum())
        assert lib.moihgp_dvec_proj_grad_norm(C.c_void_p(ctx), C.c_size_t(n), P(tx), P(tg), P(tl), P(tu), C.byref(r)) == 0
        assert abs(r.value - np.abs(np.clip(x - g, lb, ub) - x).max()) < 1e-15
        y = tb.clone()
        torch.cuda.synchronize()                                                # (the clone runs on torch's stream, the vector kernels on the context's own)
        assert lib.moihgp_dvec_axpy(C.c_void_p(ctx), C.c_size_t(n), C.c_double(-1.5), P(ta), P(y), P(tm)) == 0
        lib.moihgp_dvec_sync(C.c_void_p(ctx))
        assert np.allclose(y.cpu().numpy(), np.where(mask > 0, b - 1.5 * a, b), rtol=0, atol=1e-14)      # (fused multiply-add on the device)
        assert lib.moihgp_dvec_scale(C.c_void_p(ctx), C.c_size_t(n), C.c_double(2.0), P(ta), P(y), P(tm)) == 0
        lib.moihgp_dvec_sync(C.c_void_p(ctx))
        assert np.array_equal(y.cpu().numpy(), np.where(mask > 0, 2.0 * a, 0.0))
    lib.moihgp_dvec_ctx_del(C.c_void_p(ctx))
