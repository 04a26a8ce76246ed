"""Seeded forecast paths (include/moihgp.h moihgp_forecast_paths): the numpy definition the GPU is held to -- its two forms against each other, its
covariance across horizons against the dense GP predictive covariance, a Monte-Carlo run of it (CPU) -- then the library's generator, kernel,
chaining contract, statistics, argument checks and end-to-end pipeline against it (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rel_err
from paths_reference import (dense_predictive_cov, path_cov_np, paths_filter_form_np, paths_noise_np, paths_np, table_arrays, tail_mean_np)
from stream_reference import forecast_var_np, forward_np, noise_np, project_np, tables
from stream_support import (KMAP, POOL, assert_declared, assert_exported, bank_and_tables, cxx_fmt, cxx_rows, cxx_run, cxx_test_binary,
                            end_to_end_inputs, env)  # noqa: F401  (env: the module's fixture)

PATH_SYMBOLS = ("moihgp_forecast_paths", "moihgp_forecast_paths_noise")
B = 32             # ticks per tile of paths_kernel (paths.hip kPathBlock)
SEED = (0x9E3779B9 << 32) | 0x1234567          # the sampler tests' seed: a non-zero high word
TOL = {"f64": 1e-9, "f32": 1e-5}               # of the row's max, the sampler's: fp32 is one rounding at the store (6e-8), two decades of margin
MC = dict(S=4096, L=8, n=24)                   # the Monte-Carlo shape, on the CPU and on the device


def worst_row(got, ref):
    return float(np.max(np.max(np.abs(got - ref), axis=-1) / np.maximum(np.max(np.abs(ref), axis=-1), 1e-300)))


def pool_tables(kern, L):
    tbs = {p: tables(kern, 0.1, p) for p in POOL}
    return [tbs[POOL[l % len(POOL)]] for l in range(L)]


def mc_worst(paths, mean, covs):
    """Worst entry of the sample covariance about the known mean, in units of sqrt((C_ii C_jj + C_ij^2) / S), and worst mean in units of
    sqrt(C_jj / S): paths [S, L, n], mean [L, n], covs [L, n, n]."""
    S = paths.shape[0]
    dev = paths - mean[None]
    wc = wm = 0.0
    for l in range(paths.shape[1]):
        Cl, d = covs[l], np.diag(covs[l])
        emp = dev[:, l].T @ dev[:, l] / S
        wc = max(wc, float(np.max(np.abs(emp - Cl) / np.sqrt((np.outer(d, d) + Cl ** 2) / S))))
        wm = max(wm, float(np.max(np.abs(dev[:, l].mean(axis=0)) / np.sqrt(d / S))))
    return wc, wm


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_the_paths():
    assert_declared(PATH_SYMBOLS)


def test_library_exports_the_paths(hip_built):
    assert_exported(hip_built, PATH_SYMBOLS)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_definition_two_forms_agree(kern):
    rng = np.random.default_rng(41)
    S, L, n = 5, 8, 40
    A, K, Sv = table_arrays(pool_tables(kern, L))
    start, noise = 0.3 * rng.standard_normal((L, A.shape[1])), rng.standard_normal((S, L, n))
    a, ua = paths_np(A, K, Sv, start, noise)
    b, ub = paths_filter_form_np(A, K, Sv, start, noise)
    assert np.max(np.abs(a - b)) <= 1e-14 and np.max(np.abs(ua - ub)) <= 1e-14
    # a walk continued from its states is the walk itself
    c1, u1 = paths_np(A, K, Sv, start, noise[:, :, :13])
    c2, u2 = paths_np(A, K, Sv, u1, noise[:, :, 13:])
    assert np.array_equal(np.concatenate([c1, c2], axis=2), a) and np.array_equal(u2, ua)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_path_covariance_is_the_dense_predictive_covariance(kern):
    n = 40
    worst = 0.0
    for p in [(1.3, 0.7, 0.05)] + POOL:
        tb = tables(kern, 0.1, p)
        Cp = path_cov_np(tb, n)
        err = float(np.max(np.abs(Cp - dense_predictive_cov(tb, 600, n))))
        diag = np.array([forecast_var_np(tb, j + 1) + tb["R"] for j in range(n)])
        worst = max(worst, err)
        assert err <= 1e-12, (p, err)
        assert np.max(np.abs(np.diag(Cp) - diag)) <= 1e-12, p
    print(f"path covariance against the dense predictive covariance: {worst:.2e}")
    if kern == "Matern52":      # why the state-form recursion is not used: its noise covariance is indefinite
        assert np.linalg.eigvalsh(tables(kern, 0.1, (1.0, 0.5, 0.1))["Q"])[0] < -0.01


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_numpy_monte_carlo_reproduces_mean_and_covariance(kern):
    S, L, n = MC["S"], MC["L"], MC["n"]
    tbs = pool_tables(kern, L)
    A, K, Sv = table_arrays(tbs)
    x = 0.3 * np.random.default_rng(42).standard_normal((L, A.shape[1]))
    paths, _ = paths_np(A, K, Sv, x, paths_noise_np(SEED, 0, L, 0, S, 0, n))
    wc, wm = mc_worst(paths, np.stack([tail_mean_np(tbs[l], x[l], n) for l in range(L)]), np.stack([path_cov_np(t, n) for t in tbs]))
    print(f"Monte-Carlo of the definition: worst covariance entry {wc:.2f}, worst mean {wm:.2f} standard errors")
    assert wc <= 5.0 and wm <= 5.0, (wc, wm)


def test_cxx_sample_paths_ahead_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "paths_test"))


# ------------------------------------------------------------------------------------------------ GPU: the generator
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_paths_noise_matches_numpy(env, n):
    """The sampler's derived bound (test_noise_matches_numpy): 1e-5 absolute."""
    torch, streams = env["torch"], env["streams"]
    whole = streams.forecast_paths_noise(SEED, 3, 3, 4096 + n, latent0=7, sample0=2)
    for step0 in (0, 1, 6, 4096):
        a = streams.forecast_paths_noise(SEED, 3, 3, n, step0=step0, latent0=7, sample0=2)
        b = streams.forecast_paths_noise(SEED, 3, 3, n, step0=step0, latent0=7, sample0=2)
        torch.cuda.synchronize()
        err = np.max(np.abs(a.cpu().numpy() - paths_noise_np(SEED, 7, 3, 2, 3, step0, n)))
        print(f"paths noise n={n} step0={step0}: max abs difference {err:.3e}")
        assert a.shape == (3, 3, n) and err <= 1e-5, (step0, err)
        assert torch.equal(a, b)                                          # identical arguments, identical bits
        assert torch.equal(a, whole[:, :, step0:step0 + n])               # step0 is an offset into the same counters
    tag0 = streams.sample_noise(SEED, 3, 3, n, latent0=7, sample0=2, want_start=False)[0]
    a = streams.forecast_paths_noise(SEED, 3, 3, n, latent0=7, sample0=2)
    torch.cuda.synchronize()
    assert not torch.equal(a, tag0) and float((a - tag0).abs().max()) > 1e-3      # another tag, other normals
    assert np.max(np.abs(tag0.cpu().numpy() - noise_np(SEED, 7, 3, 2, 3, n)[0])) <= 1e-5


# ------------------------------------------------------------------------------------------------ GPU: the kernel
_DEVICE_TABLES = {}


def device_tables(streams, kern, L, bank=None):
    """(A, K, Sv) [L, ...] from the device's own tables.  The banks of bank_and_tables cycle through POOL, so their tables are read once per model
    from a bank of len(POOL) latents; any other bank is read latent by latent."""
    if bank is None:
        if kern not in _DEVICE_TABLES:
            b8 = bank_and_tables(streams, kern, len(POOL))[0]
            _DEVICE_TABLES[kern] = device_tables(streams, kern, len(POOL), b8)
        return tuple(np.stack([t[l % len(POOL)] for l in range(L)]) for t in _DEVICE_TABLES[kern])
    lat = [bank.latent(l) for l in range(L)]
    sm = [bank.smoother(l) for l in range(L)]
    return (np.stack([t["A"] for t in lat]), np.stack([t["K"] for t in sm]), np.array([t["P"][0, 0] / t["K"][0] for t in sm]))


def reference_paths(streams, tabs, start, L, S, n, seed=SEED, step0=0, sample0=0, latent0=0):
    """paths_np on the device's own noise and tables."""
    noise = streams.forecast_paths_noise(seed, L, S, n, step0=step0, latent0=latent0, sample0=sample0)
    return paths_np(*tabs, start, noise.double().cpu().numpy())


def test_device_sv_is_p00_plus_r_in_numpy():
    """Sv = P_00 + R = P_00 / K_0: what device_tables and path_covariance take from the smoother's tables."""
    for kern in ("Matern32", "Matern52"):
        for p in POOL:
            tb = tables(kern, 0.1, p)
            assert abs(tb["P"][0, 0] / tb["K"][0] - tb["S"]) <= 1e-13 * tb["S"]


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, B - 1, B, B + 1, 2 * B + 5, 1024 + 5])
def test_paths_parity(env, kern, dtype, n):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    for L, S in ((1, 1), (3, 5), (65, 1), (7, 19), (64, 2)):
        rng = np.random.default_rng(L * 100003 + S * 1009 + n)
        bank, _, _ = bank_and_tables(streams, kern, L)
        x = torch.from_numpy(0.3 * rng.standard_normal((L, bank.d))).to(tdt).cuda()
        ld = (n + 3) // 4 * 4
        buf = torch.full((S, L + 2, ld + 8), float("nan"), dtype=tdt, device="cuda")          # rows ld + 8 apart, planes L + 2 rows
        paths, states, status = bank.forecast_paths(x, n, S, seed=SEED, out=buf[:, :L, :n])
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and paths.data_ptr() == buf.data_ptr()
        assert bool(torch.isnan(buf[:, L:]).all()) and bool(torch.isnan(buf[:, :, n:]).all())  # nothing written outside the rows
        ref, ref_states = reference_paths(streams, device_tables(streams, kern, L), x.double().cpu().numpy(), L, S, n)
        err = worst_row(paths.double().cpu().numpy(), ref)
        serr = worst_row(states.cpu().numpy(), ref_states)
        assert states.dtype == torch.float64 and err <= TOL[dtype] and serr <= 1e-9, (L, S, err, serr)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_paths_chain_and_ranges_reproduce_one_call(env, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    L, S, n = 8, 3, 70
    bank, _, prm = bank_and_tables(streams, "Matern52", L)
    x = torch.from_numpy(0.3 * np.random.default_rng(43).standard_normal((L, bank.d))).to(tdt).cuda()
    whole, wstates, _ = bank.forecast_paths(x, n, S, seed=SEED)
    for n1 in (1, 4, 33, 69):
        a, sa, _ = bank.forecast_paths(x, n1, S, seed=SEED)
        out = torch.empty((S, L, 72), dtype=tdt, device="cuda")[:, :, :n - n1]
        b, sb, _ = bank.forecast_paths(None, n - n1, S, seed=SEED, step0=n1, states=sa, out=out)
        assert b.dtype == tdt and torch.equal(torch.cat([a, b], dim=2), whole) and torch.equal(sb, wstates), n1
    # ranges of samples, and a bank of the last four latents
    first = bank.forecast_paths(x, n, 2, seed=SEED, sample0=0)
    last = bank.forecast_paths(x, n, 1, seed=SEED, sample0=2)
    assert torch.equal(whole[:2], first[0]) and torch.equal(whole[2:], last[0])
    assert torch.equal(wstates[:2], first[1]) and torch.equal(wstates[2:], last[1])
    part = streams.LatentBank(0.1, prm[4:], kernel="Matern52ss")
    rows, rstates, _ = part.forecast_paths(x[4:].contiguous(), n, S, seed=SEED, latent0=4)
    assert torch.equal(whole[:, 4:], rows) and torch.equal(wstates[:, 4:], rstates)
    assert not torch.equal(whole, bank.forecast_paths(x, n, S, seed=SEED + 1)[0])
    # n = 0 writes nothing and returns the start
    slab = torch.full((S, L, 4), 7.0, dtype=tdt, device="cuda")
    none, s0, st = bank.forecast_paths(x, 0, S, seed=SEED, out=slab[:, :, :0])
    torch.cuda.synchronize()
    assert none.shape == (S, L, 0) and bool((slab == 7.0).all()) and not st.cpu().numpy().any()
    assert torch.equal(s0, x.double()[None].expand(S, L, bank.d))
    s1 = bank.forecast_paths(None, 0, S, seed=SEED, states=wstates)[1]
    assert torch.equal(s1, wstates)


# ------------------------------------------------------------------------------------------------ GPU: statistics
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_device_monte_carlo_reproduces_mean_and_covariance(env, kern):
    """The CPU test's shape and bounds on the library's own draws, means and covariances."""
    torch, streams = env["torch"], env["streams"]
    S, L, n = MC["S"], MC["L"], MC["n"]
    bank, tbs, prm = bank_and_tables(streams, kern, L)
    x = torch.from_numpy(0.3 * np.random.default_rng(42).standard_normal((L, bank.d))).cuda()
    paths, _, status = bank.forecast_paths(x, n, S, seed=SEED, want_states=False)
    mean = bank.forecast_tail(x, n)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    covs = np.stack([bank.path_covariance(l, n)[0] for l in range(L)])
    wc, wm = mc_worst(paths.cpu().numpy(), mean.cpu().numpy(), covs)
    print(f"Monte-Carlo on the device: worst covariance entry {wc:.2f}, worst mean {wm:.2f} standard errors")
    assert wc <= 5.0 and wm <= 5.0, (wc, wm)
    hz = [1, 2, 3, 5, 8, 13, 21, 24]
    var = bank.forecast_variances(hz)
    for l in range(L):
        C_l, taps = bank.path_covariance(l, n)
        diag = np.array([C_l[h - 1, h - 1] for h in hz])
        assert np.max(np.abs(diag / (var[:, l] + prm[l, 2]) - 1)) <= 1e-10, l
        # (test_smoother holds the device's K and P to 1e-10 of numpy's; C is a product of 2 n of their entries' powers: a decade more)
        assert taps[0] == 1.0 and rel_err(C_l, path_cov_np(tbs[l], n)) <= 1e-9, l


# ------------------------------------------------------------------------------------------------ GPU: status and arguments
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_latent_gives_nan_rows_and_status_1(env, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    L, S, n, bad = 7, 11, 2 * B + 5, 3
    bank, _, prm = bank_and_tables(streams, "Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    x = torch.from_numpy(0.3 * np.random.default_rng(44).standard_normal((L, bank.d))).to(tdt).cuda()
    paths, states, status = bank.forecast_paths(x, n, S, seed=SEED)
    torch.cuda.synchronize()
    st, got, gs = status.cpu().numpy(), paths.double().cpu().numpy(), states.cpu().numpy()
    keep = [l for l in range(L) if l != bad]
    assert st[bad] == 1 and not st[keep].any()
    assert np.all(np.isnan(got[:, bad])) and np.all(np.isnan(gs[:, bad]))
    assert np.all(np.isnan(bank.path_covariance(bad, 4)[0])) and np.all(np.isnan(bank.path_covariance(bad, 4)[1]))
    tabs = tuple(t[keep] for t in device_tables(streams, "Matern52", L))
    noise = streams.forecast_paths_noise(SEED, L, S, n).double().cpu().numpy()[:, keep]
    ref, ref_states = paths_np(*tabs, x.double().cpu().numpy()[keep], noise)
    assert worst_row(got[:, keep], ref) <= TOL[dtype] and worst_row(gs[:, keep], ref_states) <= 1e-9


@pytest.mark.gpu
def test_bad_arguments_return_1_and_stacked_models_3(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    L, S, n, ld = 4, 2, 64, 64
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    lib, d = bank._lib, bank.d
    x = torch.zeros((L, d), dtype=torch.float64, device="cuda")
    # one slab: the planes, then room for states that overlap them
    slab = torch.full((S * L * ld + 64,), 7.0, dtype=torch.float64, device="cuda")
    sin = torch.zeros((S, L, d), dtype=torch.float64, device="cuda")
    sout = torch.full((S, L, d), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(h=bank._h, xp=p(x), si=None, so=p(sout), n=n, step0=0, S=S, out=p(slab), ld_out=ld, plane=L * ld):
        return lib.moihgp_forecast_paths(h, 0, xp, si, so, n, step0, S, SEED, 0, 0, out, ld_out, plane, None, None)

    assert call() == 0 and call(xp=None, si=p(sin)) == 0
    torch.cuda.synchronize()
    assert not bool((slab[:S * L * ld] == 7.0).any()) and not bool((sout == 7.0).any()) and bool((slab[S * L * ld:] == 7.0).all())
    slab.fill_(7.0); sout.fill_(7.0)
    xin = slab[8:8 + L * d]                                          # a start state inside the planes
    for kw in (dict(si=p(sin)), dict(xp=None),                                            # both, neither
               dict(S=0), dict(S=65536), dict(n=(1 << 20) + 1, ld_out=(1 << 20) + 2, plane=L * ((1 << 20) + 2)),
               dict(step0=(1 << 32) - n + 1), dict(step0=1 << 40), dict(out=None),
               dict(out=p(slab, 8)), dict(ld_out=ld + 1), dict(ld_out=ld - 2), dict(plane=L * ld - 2), dict(plane=L * ld + 1),
               dict(xp=p(xin)), dict(xp=None, si=p(slab, 16)), dict(so=p(slab, S * L * ld - 16))):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((slab == 7.0).all()) and bool((sout == 7.0).all())        # nothing was launched
    assert call(step0=(1 << 32) - n) == 0                                  # the last step that exists
    stacked = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (L, 1)), kernel="Matern32x2")
    xs = torch.zeros((L, stacked.d), dtype=torch.float64, device="cuda")
    assert call(h=stacked._h, xp=p(xs), so=None) == 3
    with pytest.raises(MoihgpError):
        stacked.forecast_paths(xs, 4, 2)
    for kw in (dict(nsamples=0), dict(nsamples=65536), dict(n=-1), dict(n=(1 << 20) + 1), dict(n=2.5), dict(step0=-1), dict(step0=(1 << 32) - 3)):
        with pytest.raises(ValueError):
            bank.forecast_paths(x, **{**dict(n=4, nsamples=2), **kw})
    with pytest.raises(ValueError):
        bank.forecast_paths(x, 4, 2, states=sin)
    with pytest.raises(ValueError):
        bank.forecast_paths(None, 4, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ GPU: the lazy tables
@pytest.mark.gpu
def test_paths_after_update_use_the_new_parameters(env):
    torch, streams = env["torch"], env["streams"]
    L, S, n = 7, 3, 2 * B + 5
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    x = torch.from_numpy(0.3 * np.random.default_rng(45).standard_normal((L, bank.d))).cuda()
    before = bank.forecast_paths(x, n, S, seed=SEED)[0].clone()
    pool2 = [(p[0] * 1.5, p[1] * 0.7, p[2] * 2.0) for p in POOL]      # of test_sample_after_update_uses_the_new_parameters
    bank.update(np.array([pool2[l % len(pool2)] for l in range(L)]))
    paths, states, status = bank.forecast_paths(x, n, S, seed=SEED)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and not torch.equal(paths, before)
    tabs = device_tables(streams, "Matern52", L, bank)
    for l in range(L):
        tb = tables("Matern52", 0.1, pool2[l % len(pool2)])
        assert rel_err(tabs[0][l], tb["A"]) <= 1e-9 and rel_err(tabs[1][l], tb["K"]) <= 1e-8 and abs(tabs[2][l] - tb["S"]) <= 1e-8 * tb["S"], l
    ref, ref_states = reference_paths(streams, tabs, x.cpu().numpy(), L, S, n)
    assert worst_row(paths.cpu().numpy(), ref) <= TOL["f64"] and worst_row(states.cpu().numpy(), ref_states) <= 1e-9


@pytest.mark.gpu
def test_tables_built_on_one_stream_serve_the_paths_on_another(env):
    """The smoother's tables are built on s1 by the first call and read on s2 right behind it: every call gives what the same calls on one
    stream of another fresh bank give.  (One run cannot prove the ordering; it pins the contract and catches an event that is not recorded or
    not waited for.)"""
    torch, streams = env["torch"], env["streams"]
    L, S, n = 8, 3, 2 * B + 5
    x = torch.from_numpy(0.3 * np.random.default_rng(46).standard_normal((L, 3))).cuda()
    torch.cuda.synchronize()

    def calls(s1, s2):
        bank, _, _ = bank_and_tables(streams, "Matern52", L)
        with torch.cuda.stream(s1):
            out = list(bank.forecast_paths(x, n, S, seed=SEED))
        with torch.cuda.stream(s2):
            out += list(bank.forecast_paths(x, n, S, seed=SEED, sample0=S))
        s1.synchronize(); s2.synchronize()
        return out

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    two, one = calls(s1, s2), calls(s1, s1)
    assert len(two) == len(one) == 6
    for i, (a, b) in enumerate(zip(two, one)):
        assert torch.equal(a, b), i
    ref, _ = reference_paths(streams, device_tables(streams, "Matern52", L), x.cpu().numpy(), L, S, n, sample0=S)
    assert worst_row(two[3].cpu().numpy(), ref) <= TOL["f64"]


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("missing", [False, True])
def test_forecast_path_outputs_end_to_end(env, kern, missing):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    M, L, T, n, S = 8, 3, 300, 20, 4
    params, Y = end_to_end_inputs(np.random.default_rng(47), M, L, T, missing)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yd = torch.from_numpy(Y).cuda()
    Ypaths, Ymean = streams.forecast_path_outputs(gp, Yd, n, S, seed=SEED)
    torch.cuda.synchronize()
    assert Ypaths.shape == (S, n, M) and Ymean.shape == (n, M)
    U, Sc, igp, Ty = project_np(gp, Y)
    tbs = [tables(kern, 0.1, igp[l]) for l in range(L)]
    xe = forward_np(tbs, Ty)[2]                                          # the end state with the Kalman gains
    W = U * np.sqrt(Sc)
    noise = streams.forecast_paths_noise(SEED, L, S, n).double().cpu().numpy()
    ref = np.einsum("ml,slj->sjm", W, paths_np(*table_arrays(tbs), xe, noise)[0])
    ref_mean = (W @ np.stack([tail_mean_np(tbs[l], xe[l], n) for l in range(L)])).T
    # The device's own normals go into the reference, so nothing of test_sample_outputs_end_to_end's noise term is left: the means and tables
    # agree to 1e-9 of the outputs' scale, its other term.
    bound = 1e-9 * np.max(np.abs(ref))
    diff = np.max(np.abs(Ypaths.cpu().numpy() - ref), axis=(0, 1))
    print("forecast_path_outputs: max abs difference per output", diff, "bound", bound)
    assert np.all(diff <= bound), (diff, bound)
    assert rel_err(Ymean.cpu().numpy(), ref_mean) <= 1e-9
    # the mean is the un-projected forecast_tail of the same end state
    bank = streams.LatentBank.from_handle(gp)
    x = bank.forecast_scores(streams.project_stream(gp, Yd), [1], T=T)["x"]
    assert torch.equal(Ymean, streams.unproject_stream(gp, bank.forecast_tail(x, n), n))


@pytest.mark.gpu
def test_forecast_path_outputs_raises_on_a_failed_latent(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(48)
    M, L, T = 8, 3, 100
    gp = MOIHGP(0.1, M, L, kernel="Matern52ss")
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    igp[1, 0] = np.nan
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], igp.ravel()]))
    with pytest.raises(MoihgpError, match="did not converge"):
        streams.forecast_path_outputs(gp, torch.from_numpy(rng.standard_normal((T, M))).cuda(), 5, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_cxx_sample_paths_ahead_matches_python(env, hip_built, kern):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP
    M, L, T, n, S = 12, 4, 300, 37, 2
    params, Y = end_to_end_inputs(np.random.default_rng(49), M, L, T, True)
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T} {n} {S} {SEED}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) + "\n"
    out = cxx_run(cxx_test_binary(hip_built, "paths_test"), inp)
    got = cxx_rows(out).reshape(S, n, M)
    gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Ypaths, _ = streams.forecast_path_outputs(gp, torch.from_numpy(Y).cuda(), n, S, seed=SEED)
    torch.cuda.synchronize()
    assert rel_err(got, Ypaths.cpu().numpy()) <= 1e-12
