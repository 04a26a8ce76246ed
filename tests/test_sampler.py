"""Seeded steady-state posterior sampling (include/moihgp.h moihgp_sample_stream): the numpy definition the GPU is held to -- the Philox4x32-10
generator against Random123's known answers, the innovations realization of the smoother's autocovariance against the dense GP posterior
covariance (CPU) -- then the library's generator, tables and sweeps against it (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rel_err
from parity_support import synth
from stream_reference import acov_hat, deviations_np, noise_np, philox4x32_10, realization, smooth_outputs_np, tables
from stream_support import (KMAP, POOL, assert_declared, assert_exported, bank_and_tables, cxx_fmt, cxx_rows, cxx_run, cxx_test_binary,
                            end_to_end_inputs, env, to_dev)  # noqa: F401  (env: the module's fixture)

SAMPLE_SYMBOLS = ("moihgp_sample_stream", "moihgp_sample_noise", "moihgp_get_sampler")
GROUP = 8          # samples per wavefront of sample_sweep_kernel (sampler.hip kSampleGroup)
SEED = (0x9E3779B9 << 32) | 0x1234567          # a non-zero high word


# ------------------------------------------------------------------------------------------------ cross-check of the numpy definition
def dense_posterior_cov(tb, T):
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    c = np.zeros(T); M = np.eye(A.shape[0])
    for k in range(T):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    i = np.arange(T)
    Cm = c[np.abs(i[:, None] - i[None, :])]
    return Cm - Cm @ np.linalg.solve(Cm + R * np.eye(T), Cm)


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_sampler():
    assert_declared(SAMPLE_SYMBOLS)


def test_library_exports_the_sampler(hip_built):
    assert_exported(hip_built, SAMPLE_SYMBOLS)


def test_numpy_philox_gives_the_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    u = lambda *w: np.array(w, dtype=np.uint32)
    ones = 0xFFFFFFFF
    for ctr, key, ref in ((u(0, 0, 0, 0), u(0, 0), u(0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                          (u(ones, ones, ones, ones), u(ones, ones), u(0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                          (u(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), u(0xa4093822, 0x299f31d0), u(0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert np.array_equal(philox4x32_10(ctr, key), ref)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_realization_reproduces_the_posterior_autocovariance(kern):
    for p in POOL:
        tb = tables(kern, 0.1, p)
        R = realization(tb["G"], tb["Ps"])
        assert R["status"] == 0 and R["err"] <= 1e-12, (p, R["err"])
        W = tb["PF"] - tb["G"] @ tb["P"] @ tb["G"].T
        if kern == "Matern52":      # why the state-form backward sampler is not used: its noise covariance is indefinite
            assert np.linalg.eigvalsh((W + W.T) / 2)[0] < 0, p
    tb = tables(kern, 0.1, [1.3, 0.7, 0.05])
    R = realization(tb["G"], tb["Ps"])
    post = dense_posterior_cov(tb, 600)
    rh = acov_hat(tb["G"], R["Sigma"], R["sigma2"], R["B"], 40)
    assert np.max(np.abs(rh - post[300, 300:340])) <= 1e-12


def test_numpy_realization_over_the_learners_box():
    """The draw of test_smoother_gain_is_contractive_over_the_learners_box (same seed and skip rule): the 1e-9 acceptance holds on at least 95 %
    of the draws scipy's DARE solves."""
    rng = np.random.default_rng(3)
    used = ok = 0
    for i in range(400):
        kern = ("Matern32", "Matern52")[i % 2]
        dt = (1e-3, 1e-2, 0.1, 1.0)[(i // 2) % 4]
        tb = tables(kern, dt, 10.0 ** rng.uniform(-4, 2, 3))
        if tb is None:
            continue
        used += 1
        ok += realization(tb["G"], tb["Ps"])["status"] == 0
    assert used >= 300 and ok >= 0.95 * used, (used, ok)


def test_cxx_sample_smoothed_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "sampler_test"))


# ------------------------------------------------------------------------------------------------ GPU: the generator
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 1027])
def test_noise_matches_numpy(env, T):
    """|n| <= 5.9 (u1 >= 2^-25); the fp32 rounding of the angle (<= 2 pi 2^-24 relative half an ulp -> 3.7e-7 rad) gives 5.9 * 3.7e-7 = 2.2e-6, and
    logf, sqrtf, cosf, sinf at an ulp or two each are of the same order: 1e-5 absolute."""
    torch, streams = env["torch"], env["streams"]
    noise, start = streams.sample_noise(SEED, 3, 3, T, latent0=7, sample0=2)
    torch.cuda.synchronize()
    rn, rs = noise_np(SEED, 7, 3, 2, 3, T)
    en, es = np.max(np.abs(noise.cpu().numpy() - rn)), np.max(np.abs(start.cpu().numpy() - rs))
    print(f"noise: max abs difference {en:.3e} (ticks), {es:.3e} (start)")
    assert noise.shape == (3, 3, T) and en <= 1e-5 and es <= 1e-5


@pytest.mark.gpu
def test_noise_moments_and_streams(env):
    torch, streams = env["torch"], env["streams"]
    L = S = 4; T = 4099
    a, sa = streams.sample_noise(SEED, L, S, T)
    b, sb = streams.sample_noise(SEED, L, S, T)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(sa, sb)                      # identical arguments, identical bits
    n = a.double().cpu().numpy()
    N = n.size
    assert abs(n.mean()) <= 5 / np.sqrt(N) and abs(n.var() - 1) <= 5 * np.sqrt(2 / N), (n.mean(), n.var())
    planes = [n[s, l] for s in range(S) for l in range(L)]
    planes.append(streams.sample_noise(SEED + 1, 1, 1, T)[0][0, 0].double().cpu().numpy())            # another seed (low word)
    planes.append(streams.sample_noise(SEED + (1 << 32), 1, 1, T)[0][0, 0].double().cpu().numpy())    # ... (high word)
    for i in range(len(planes)):
        for j in range(i):
            assert np.max(np.abs(planes[i] - planes[j])) > 1.0 and abs(np.corrcoef(planes[i], planes[j])[0, 1]) <= 5 / np.sqrt(T), (i, j)
    # latent0 / sample0 are offsets into the same counters
    c, _ = streams.sample_noise(SEED, 2, 2, T, latent0=2, sample0=1)
    assert np.array_equal(c.cpu().numpy(), a[1:3, 2:4].cpu().numpy())


# ------------------------------------------------------------------------------------------------ GPU: the tables
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_sampler_tables_match_numpy(env, kern):
    bank, tbs, _ = bank_and_tables(env["streams"], kern, 8)
    for l in range(8):
        got, ref = bank.sampler(l), realization(tbs[l]["G"], tbs[l]["Ps"])
        assert got["status"] == 0 and got["acov_err"] <= 1e-9, (l, got)
        assert rel_err(got["B"], ref["B"]) <= 1e-8 and abs(got["sigma2"] - ref["sigma2"]) <= 1e-8 * ref["sigma2"], (l, got, ref)
        assert np.max(np.abs(got["Lc"] @ got["Lc"].T - got["Sigma"])) <= 1e-9 * np.max(np.abs(got["Sigma"])), l
    r0 = np.random.default_rng(0)
    prm = np.column_stack([r0.uniform(0.5, 2, 64), r0.uniform(0.5, 2, 64), r0.uniform(0.05, 0.2, 64)])      # bench.py's box
    bank = env["streams"].LatentBank(0.1, prm, kernel=KMAP[kern])
    assert all(bank.sampler(l)["status"] == 0 for l in range(64))


# ------------------------------------------------------------------------------------------------ GPU: the sweeps
def device_tables(bank, L):
    sm = [bank.smoother(l) for l in range(L)]
    sp = [bank.sampler(l) for l in range(L)]
    return (np.stack([t["G"] for t in sm]), np.stack([t["B"] for t in sp]), np.sqrt(np.array([t["sigma2"] for t in sp])),
            np.stack([t["Lc"] for t in sp]))


def reference_samples(streams, bank, L, S, T, ys, seed=SEED, sample0=0, latent0=0):
    """ysmooth (as returned) plus the numpy recursion on the device's own noise and tables."""
    noise, start = streams.sample_noise(seed, L, S, T, latent0=latent0, sample0=sample0)
    o = deviations_np(*device_tables(bank, L), noise.double().cpu().numpy(), start.double().cpu().numpy())
    return ys.double().cpu().numpy()[None] + o


def worst_row(got, ref):
    return float(np.max(np.max(np.abs(got - ref), axis=-1) / np.maximum(np.max(np.abs(ref), axis=-1), 1e-300)))


def stream_with_gaps(L, T, rng):
    Ty = synth(L, T, rng)
    for t in (15, 16, 1023, 1024):           # a chunk edge and a segment edge
        if t < T - 1:
            Ty[:, t] = np.nan
    return Ty


TOL = {"f64": 1e-9, "f32": 1e-5}     # of the row's max; fp32: two roundings (ysmooth as stored, the sample) at 6e-8 each, two decades of margin


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 1023, 1024, 1025, 2049 + 5])
def test_sample_parity(env, kern, dtype, T):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    for L in (1, 3, 65):
        rng = np.random.default_rng(L * 100003 + T)
        bank, _, _ = bank_and_tables(streams, kern, L)
        Ty = stream_with_gaps(L, T, rng)
        dev = to_dev(torch, Ty, tdt, T)
        x0 = torch.from_numpy(0.1 * rng.standard_normal((L, bank.d))).to(tdt).cuda()
        ys0, xe0, _ = bank.smooth(dev, x=torch.empty_like(x0), x_start=x0)
        for S in (1, 3, 2 * GROUP + 1):
            ld = (T + 3) // 4 * 4
            buf = torch.full((S, L + 2, ld + 8), float("nan"), dtype=tdt, device="cuda")       # rows ld + 8 apart, planes L + 2 rows
            ysb = torch.full((L, ld + 4), float("nan"), dtype=tdt, device="cuda")              # ysmooth's rows ld + 4 apart
            smp, ys, x, status = bank.sample(dev, S, seed=SEED, x=torch.empty_like(x0), x_start=x0, out=buf[:, :L, :T], ysmooth=ysb[:, :T])
            torch.cuda.synchronize()
            assert int(status.abs().sum()) == 0
            assert torch.equal(ys, ys0) and torch.equal(x, xe0)                                # bit-equal to LatentBank.smooth
            assert bool(torch.isnan(buf[:, L:]).all()) and bool(torch.isnan(buf[:, :, T:]).all())   # nothing written outside the rows
            err = worst_row(smp.double().cpu().numpy(), reference_samples(streams, bank, L, S, T, ys))
            assert err <= TOL[dtype], (L, S, err)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sample_scan_and_serial_paths_agree(env, kern, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    L, T, S = 9, 2500, 3
    bank, _, _ = bank_and_tables(streams, kern, L)
    dev = to_dev(torch, stream_with_gaps(L, T, np.random.default_rng(21)), tdt, T)
    bank.set_option("sample_path", 0)
    a = bank.sample(dev, S, seed=SEED)[0].clone()
    bank.set_option("sample_path", 1)
    b, ys, _, _ = bank.sample(dev, S, seed=SEED)
    torch.cuda.synchronize()
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    assert worst_row(a, b) <= TOL[dtype]
    assert worst_row(b, reference_samples(streams, bank, L, S, T, ys)) <= TOL[dtype]


@pytest.mark.gpu
def test_sample_growth_bound_fallback(env):
    """The latent of test_growth_bound_fallback (Matern-5/2, lengthscale 0.01 at dt 0.01): powers of G above the scan's growth bound, so the automatic
    path walks it serially -- bit for bit the all-serial path -- while the other latents take the scan."""
    torch, streams = env["torch"], env["streams"]
    pool = [(1.0, 0.01, 0.01), (1.0, 1.0, 0.1), (0.7, 0.5, 0.05), (1.0, 0.03, 1e-4)]
    L, T, S = 8, 3000, 3
    bank, tbs, _ = bank_and_tables(streams, "Matern52", L, dt=0.01, pool=pool)
    G = tbs[0]["G"]
    assert max(np.abs(np.linalg.matrix_power(G, k)).sum(1).max() for k in range(1, 33)) > 1e4      # the fallback is reached
    dev = to_dev(torch, synth(L, T, np.random.default_rng(22)), torch.float64, T)
    sa, ys, _, st = bank.sample(dev, S, seed=SEED)
    sa = sa.clone()
    bank.set_option("sample_path", 1)
    ss = bank.sample(dev, S, seed=SEED)[0]
    bank.set_option("sample_path", 0)
    sc = bank.sample(dev, S, seed=SEED)[0]
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    sa, ss, sc = sa.cpu().numpy(), ss.cpu().numpy(), sc.cpu().numpy()
    slow = [l for l in range(L) if l % 4 in (0, 3)]                    # (the fourth pool entry exceeds the bound too)
    fast = [l for l in range(L) if l % 4 in (1, 2)]
    assert np.array_equal(sa[:, slow], ss[:, slow])                    # the fallback latents: the serial walk itself
    assert np.array_equal(sa[:, fast], sc[:, fast])                    # the others: the scan
    assert not np.array_equal(sa[:, slow], sc[:, slow])
    assert worst_row(sa, reference_samples(streams, bank, L, S, T, ys)) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("path", [0, 1])
def test_sample_ranges_reproduce_one_call(env, dtype, path):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    L, T = 8, 1500
    bank, _, prm = bank_and_tables(streams, "Matern52", L)
    bank.set_option("sample_path", path)
    Ty = synth(L, T, np.random.default_rng(23))
    dev = to_dev(torch, Ty, tdt, T)
    whole = bank.sample(dev, 4, seed=SEED)[0].clone()
    first = bank.sample(dev, 2, seed=SEED, sample0=0)[0].clone()
    second = bank.sample(dev, 2, seed=SEED, sample0=2)[0]
    assert torch.equal(whole[:2], first) and torch.equal(whole[2:], second)
    part = streams.LatentBank(0.1, prm[4:], kernel="Matern52ss")
    part.set_option("sample_path", path)
    rows = part.sample(to_dev(torch, Ty[4:], tdt, T), 4, seed=SEED, latent0=4)[0]
    assert torch.equal(whole[:, 4:], rows)
    assert not torch.equal(whole, bank.sample(dev, 4, seed=SEED + 1)[0])


# ------------------------------------------------------------------------------------------------ GPU: the lazy tables
@pytest.mark.gpu
@pytest.mark.parametrize("first", ["sample", "read"])
def test_sample_after_update_uses_the_new_parameters(env, first):
    """The realization's tables follow a parameter update, whether a sweep or a host read built them before it."""
    torch, streams = env["torch"], env["streams"]
    L, T, S = 7, 1000, 3
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    dev = to_dev(torch, synth(L, T, np.random.default_rng(29)), torch.float64, T)
    if first == "sample":
        bank.sample(dev, S, seed=SEED)
    else:
        bank.sampler(0)
    pool2 = [(p[0] * 1.5, p[1] * 0.7, p[2] * 2.0) for p in POOL]      # of test_smooth_after_update_uses_the_new_parameters
    bank.update(np.array([pool2[l % len(pool2)] for l in range(L)]))
    smp, ys, _, status = bank.sample(dev, S, seed=SEED)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    for l in range(L):
        tb = tables("Matern52", 0.1, pool2[l % len(pool2)])
        got, ref = bank.sampler(l), realization(tb["G"], tb["Ps"])
        assert got["status"] == 0 and got["acov_err"] <= 1e-9, (l, got)
        assert rel_err(got["B"], ref["B"]) <= 1e-8 and abs(got["sigma2"] - ref["sigma2"]) <= 1e-8 * ref["sigma2"], (l, got, ref)
    assert worst_row(smp.cpu().numpy(), reference_samples(streams, bank, L, S, T, ys)) <= TOL["f64"]


@pytest.mark.gpu
def test_tables_built_on_one_stream_serve_another(env):
    """The smoother's tables are built on s1 and read on s2, the realization's built on s2 and read on s1: every call gives what the same calls
    on one stream of another fresh bank give.  (One run cannot prove the ordering; it pins the contract and catches an event that is not
    recorded or not waited for.)"""
    torch, streams = env["torch"], env["streams"]
    L, T, S, hz = 8, 1500, 3, (1, 7)
    dev = to_dev(torch, synth(L, T, np.random.default_rng(30)), torch.float64, T)
    torch.cuda.synchronize()

    def calls(s1, s2):
        bank, _, _ = bank_and_tables(streams, "Matern52", L)
        with torch.cuda.stream(s1):
            out = list(bank.smooth(dev))
        with torch.cuda.stream(s2):
            out += list(bank.sample(dev, S, seed=SEED)) + list(bank.forecast(dev, hz, gains="kalman"))
        with torch.cuda.stream(s1):
            out += list(bank.sample(dev, S, seed=SEED))
        s1.synchronize(); s2.synchronize()
        return out

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    two, one = calls(s1, s2), calls(s1, s1)
    assert len(two) == len(one) == 14
    for i, (a, b) in enumerate(zip(two, one)):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------ GPU: status
@pytest.mark.gpu
@pytest.mark.parametrize("path", [-1, 0, 1])
def test_failed_latent_gives_nan_everywhere_and_status_1(env, path):
    torch, streams = env["torch"], env["streams"]
    L, T, S, bad = 7, 1500, 3, 3
    bank, _, prm = bank_and_tables(streams, "Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    bank.set_option("sample_path", path)
    smp, ys, x, status = bank.sample(to_dev(torch, synth(L, T, np.random.default_rng(24)), torch.float64, T), S, seed=SEED)
    torch.cuda.synchronize()
    st, got = status.cpu().numpy(), smp.cpu().numpy()
    keep = [l for l in range(L) if l != bad]
    assert st[bad] == 1 and not st[keep].any() and bank.sampler(bad)["status"] == 1
    assert np.all(np.isnan(got[:, bad])) and np.all(np.isnan(ys.cpu().numpy()[bad])) and np.all(np.isnan(x.cpu().numpy()[bad]))
    assert worst_row(got[:, keep], reference_samples(streams, bank, L, S, T, ys)[:, keep]) <= 1e-9


@pytest.mark.gpu
def test_bad_arguments_return_1_and_stacked_models_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    L, T, ld = 4, 64, 64
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    lib = bank._lib
    Ty = torch.zeros((L, ld), dtype=torch.float64, device="cuda")
    x = torch.zeros((L, bank.d), dtype=torch.float64, device="cuda")
    ys = torch.full((L, ld), 7.0, dtype=torch.float64, device="cuda")
    good = torch.full((2, L, ld), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(S=2, ysp=p(ys), ld_out=ld, smp=p(good), plane=L * ld):
        return lib.moihgp_sample_stream(bank._h, 0, p(Ty), T, ld, p(x), p(x), S, SEED, 0, 0, ysp, ld_out, smp, plane, None, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((good == 7.0).any()) and not bool((ys == 7.0).any())
    ys.fill_(7.0); good.fill_(7.0)
    for kw in (dict(S=0), dict(S=65536), dict(ysp=None), dict(smp=None), dict(ysp=p(Ty)), dict(smp=p(Ty)), dict(smp=p(ys)),      # counts, nulls, overlaps
               dict(smp=p(good, 8)), dict(ysp=p(ys, 8)), dict(ld_out=ld + 1), dict(ld_out=ld - 2), dict(plane=L * ld - 2), dict(plane=L * ld + 1)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((good == 7.0).all()) and bool((ys == 7.0).all())        # nothing was launched
    stacked = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (L, 1)), kernel="Matern32x2")
    xs = torch.zeros((L, stacked.d), dtype=torch.float64, device="cuda")
    assert lib.moihgp_sample_stream(stacked._h, 0, p(Ty), T, ld, p(xs), p(xs), 2, SEED, 0, 0, p(ys), ld, p(good), L * ld, None, None) == 3
    assert lib.moihgp_get_sampler(stacked._h, 0, None, None, None, None, None, None) == 3
    with pytest.raises(MoihgpError):
        stacked.sample(Ty, 2)
    with pytest.raises(ValueError):
        bank.sample(Ty, 0)


@pytest.mark.gpu
def test_sample_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(25)
    M, L, T = 8, 3, 100
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.sample_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda(), 2)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("missing", [False, True])
def test_sample_outputs_end_to_end(env, kern, missing):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    M, L, T, S = 6, 3, 300, 3
    params, Y = end_to_end_inputs(np.random.default_rng(26), M, L, T, missing)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yd = torch.from_numpy(Y).cuda()
    Ys, Ymean, var = streams.sample_outputs(gp, Yd, S, seed=SEED)
    Ysm, var_s = streams.smooth_outputs(gp, Yd)
    torch.cuda.synchronize()
    assert Ys.shape == (S, T, M) and torch.equal(Ymean, Ysm) and np.array_equal(var, var_s)
    ref_mean, ref_var = smooth_outputs_np(gp, Y, kern)
    assert rel_err(Ymean.T.cpu().numpy(), ref_mean) <= 1e-9 and rel_err(var, ref_var) <= 1e-10
    prm = gp.params
    U, Sc = prm[:M * L].reshape(M, L), prm[M * L:M * L + L]
    igp = prm[-3 * L:].reshape(L, 3)
    tbs = [tables(kern, 0.1, igp[l]) for l in range(L)]
    rz = [realization(t["G"], t["Ps"]) for t in tbs]
    noise, start = noise_np(SEED, 0, L, 0, S, T)
    o = deviations_np(np.stack([t["G"] for t in tbs]), np.stack([r["B"] for r in rz]), np.sqrt([r["sigma2"] for r in rz]),
                      np.stack([r["Lc"] for r in rz]), noise, start)
    W = U * np.sqrt(Sc)
    ref = ref_mean[None] + np.einsum("ml,slt->smt", W, o)
    # The deviations are linear in the normals, and the device's differ from numpy's by up to 1e-5 each (test_noise_matches_numpy): a deviation
    # moves by at most 1e-5 times the absolute sum of its impulse response, sigma (1 + sum_k |(G^k B)_0|) + max_k sum_j |(G^k Lc)_0j|; the means
    # and tables agree to 1e-9 of the outputs' scale.
    gain = np.zeros(L)
    for l, (t, r) in enumerate(zip(tbs, rz)):
        v, Z, acc, top = r["B"].copy(), r["Lc"].copy(), 1.0, 0.0
        for _ in range(T):
            acc += abs(v[0]); top = max(top, np.abs(Z[0]).sum())
            v = t["G"] @ v; Z = t["G"] @ Z
        gain[l] = np.sqrt(r["sigma2"]) * acc + top
    bound = 1e-5 * (np.abs(W) @ gain) + 1e-9 * np.max(np.abs(ref))
    diff = np.max(np.abs(Ys.permute(0, 2, 1).cpu().numpy() - ref), axis=(0, 2))
    print("sample_outputs: max abs difference per output", diff, "bound", bound)
    assert np.all(diff <= bound), (diff, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_sample_smoothed_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    M, L, T, S = 12, 4, 300, 2
    params, Y = end_to_end_inputs(np.random.default_rng(27), M, L, T, True)
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T} {S} {SEED}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
    out = cxx_run(cxx_test_binary(hip_built, "sampler_test"), inp)
    got = cxx_rows(out).reshape(S, T, M)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Ys, _, _ = streams.sample_outputs(gp, torch.from_numpy(Y).cuda(), S, seed=SEED)
    torch.cuda.synchronize()
    assert rel_err(got, Ys.cpu().numpy()) <= 1e-12


@pytest.mark.gpu
def test_sample_variance_is_var_smoothed(env):
    """One statistical net: 16 samples x 3072 interior ticks per latent are ~3000 effective draws (the posterior's correlation length is a few
    ticks), a 2.6 % standard error of the variance; 15 % is more than five of them."""
    torch, streams = env["torch"], env["streams"]
    L, T, S = 8, 4096, 16
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    dev = to_dev(torch, synth(L, T, np.random.default_rng(28)).astype(np.float32).astype(np.float64), torch.float32, T)
    smp, ys, _, status = bank.sample(dev, S, seed=SEED)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    dev_ = (smp - ys[None]).double().cpu().numpy()[:, :, 512:3584]
    var = (dev_ ** 2).mean(axis=(0, 2))
    _, vs = bank.latent_variances()
    print("sample variance / var_smoothed:", var / vs)
    assert np.max(np.abs(var / vs - 1)) <= 0.15, var / vs
