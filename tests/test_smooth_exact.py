"""Exact-edge smoothing (include/moihgp.h moihgp_smooth_stream_exact): the numpy definition (edges_reference.exact_np) held against the dense GP
posterior on the CPU, then the library against the definition on the GPU.

Tolerances.  CPU, definition against the dense posterior: 1e-10 for means (relative to the row's max |mean|, floor 1e-3) and 2e-8 for variances
(relative to the largest variance).  GPU: means and end states at the project's FP64_TIGHT / FP32_TOL relative to the row's max |mean|, against
exact_np on scipy's tables.  fp64 variances: per pool draw, ten times the disagreement between exact_np in np.float64 and the same lines in
np.longdouble (var_rounding below, the worst over T_DEVICE; stream_support describes the precedent at VAR_EDGE).  That figure is a rounding error
of the edge formulas GIVEN the tables, a few 1e-16 on most draws, far below the 1e-10 to which the device's and scipy's DARE solutions agree: so
the variances are compared with exact_np evaluated on the device's own tables (LatentBank.smoother / .latent, as test_smoother's growth-bound test
does), which isolates the edge kernel; the tables themselves are held to scipy's in test_smoother.  fp32 variances: FP32_TOL.

Measured on an MI355X (test_exact_parity, worst over its cases): fp64 means 1.8e-13, end states 4.8e-12, variances 0.29 of their bound; fp32 means
and end states 6.2e-7."""
import ctypes as C
import os

import numpy as np
import pytest

from edges_reference import EDGE_CAP, dense_posterior_np, edge_lengths_np, edge_terms, exact_np
from stream_reference import model, project_np, smooth_np, tables
from stream_support import (FP32_TOL, FP64_TIGHT, KMAP, POOL, assert_declared, assert_exported, bank_and_tables, cxx_fmt, cxx_rows, cxx_run,
                            cxx_test_binary, end_to_end_inputs, env, gaps_ends_run_copy, padding_untouched, sentinel_out, tdt_of, to_dev,
                            to_dev_poison, tol_of)  # noqa: F401  (env: the module's fixture)

EXACT_SYMBOLS = ("moihgp_smooth_stream_exact", "moihgp_edge_lengths")
KERNS = ("Matern32", "Matern52")
T_DENSE = (1, 2, 17, 63, 300, 1000)
T_DEVICE = (1, 2, 17, 63, 64, 300, 1025, 4096)     # one tick, inside one chunk, chunk and segment edges, overlapping and separate edges, the scratch limit
SLOW = (1.0, 50.0, 1.0)                            # Matern-5/2: rho(G) = 0.9934, head about 6800 ticks
MEAN_TOL, VAR_TOL = 1e-10, 2e-8


def stream_of(L, T, rng):
    t = np.arange(T)[None, :]
    return np.sin(0.05 * t + 1.0 + np.arange(L)[:, None]) + 0.3 * rng.standard_normal((L, T))


def row_err(got, ref, floor=1e-3):
    """Worst row of max |got - ref| over the row's max |ref| (at least `floor`)."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), floor)))


def var_err(got, ref):
    """Worst row of max |got - ref| over the row's largest variance."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    return float(np.max(np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)))


_ROUNDING = {}


def var_rounding(tb, Ts=T_DEVICE):
    """The disagreement between the fp64 and the 80-bit evaluation of the variance formulas on the tables tb: the worst over Ts of
    max_t |var64 - var80| / max_t var80."""
    key = (tb["G"].tobytes(), tb["P"].tobytes(), tuple(Ts))
    if key not in _ROUNDING:
        worst = 0.0
        for T in Ts:
            v64, v80 = edge_terms(tb, T, np.float64)["var"], edge_terms(tb, T, np.longdouble)["var"]
            worst = max(worst, float(np.max(np.abs(v64 - v80)) / np.max(v80)))
        _ROUNDING[key] = worst
    return _ROUNDING[key]


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_loader_declare_exact_smoothing():
    assert_declared(EXACT_SYMBOLS)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moihgp.h")).read()
    assert "no exactness is claimed" in text


def test_library_exports_exact_smoothing(hip_built):
    assert_exported(hip_built, EXACT_SYMBOLS)


def test_cxx_predict_smoothed_exact_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "smooth_exact_test"))


@pytest.mark.parametrize("kern", KERNS)
def test_definition_is_the_gp_posterior_and_the_steady_smoother_is_not(kern):
    """exact_np against the dense posterior C (C + R I)^-1 y over the whole POOL: means, variances and the 12-tick forecast from the end state.
    Measured with this seed, worst over both kernels: means 2.1e-12, variances 1.7e-9 (the draw with R = 1e-6; 1.9e-12 on the others), forecasts
    8.4e-13.  On POOL[0] the steady smoother's mean at tick 0 is off by 15 % of the row's scale or more at every T (measured 15 - 55 %)."""
    rng = np.random.default_rng(17)
    worst = np.zeros(3)
    for prm in POOL:
        tb = tables(kern, 0.1, prm)
        for T in T_DENSE:
            y = np.sin(0.05 * np.arange(T) + 1.0) + 0.3 * rng.standard_normal(T)
            mean, var, ahead = dense_posterior_np(tb, y, 12)
            e = exact_np([tb], y[None, :])
            assert e["status"][0] == 0
            scale = max(float(np.max(np.abs(mean))), 1e-3)
            em = float(np.max(np.abs(e["ys"][0] - mean))) / scale
            ev = float(np.max(np.abs(e["var"][0] - var)) / np.max(var))
            x, fc = e["x"][0], []
            for _ in range(12):
                x = tb["A"] @ x
                fc.append(x[0])
            ef = float(np.max(np.abs(np.array(fc) - ahead))) / scale
            e0 = abs(smooth_np([tb], y[None, :])[0][0, 0] - mean[0]) / scale
            print(f"{kern} {prm} T={T}: mean {em:.1e} var {ev:.1e} forecast {ef:.1e}; steady smoother at tick 0 {e0:.2f}")
            worst = np.maximum(worst, [em, ev, ef])
            assert em <= MEAN_TOL and ev <= VAR_TOL and ef <= MEAN_TOL, (prm, T, em, ev, ef)
            if prm == POOL[0]:
                assert e0 > 0.05, (T, e0)
    print(f"{kern}: worst mean {worst[0]:.1e} var {worst[1]:.1e} forecast {worst[2]:.1e}")


@pytest.mark.parametrize("kern", KERNS)
def test_ticks_outside_the_edges_are_untouched(kern):
    """T >= head + tail: between the edges the definition keeps the steady sweeps' bits and the steady variance, and what it leaves out there is
    below 1e-12 of the row's scale (a hundredth of the definition's own tolerance): the formulas at every tick give the same row."""
    rng = np.random.default_rng(18)
    T = 1000
    for prm in POOL:
        tb = tables(kern, 0.1, prm)
        head, tail = edge_lengths_np(tb)
        assert 0 < tail <= head and head + tail <= T, (prm, head, tail)
        y = stream_of(1, T, rng)
        e, f = exact_np([tb], y), exact_np([tb], y, full=True)
        assert (e["head"][0], e["tail"][0]) == (head, tail)
        steady = smooth_np([tb], y)[0]
        assert np.array_equal(e["ys"][0, head:T - tail], steady[0, head:T - tail])
        assert np.array_equal(e["x"], e["x_steady"])
        assert np.all(e["var"][0, head:T - tail] == tb["var_s"])
        assert not np.array_equal(e["ys"][0, :head], steady[0, :head])
        assert e["var"][0, 0] > tb["var_s"] and e["var"][0, T - 1] > tb["var_s"]
        assert row_err(e["ys"], f["ys"]) <= 1e-12 and var_err(e["var"], f["var"]) <= 1e-12 and row_err(e["x"], f["x"]) <= 1e-12


@pytest.mark.parametrize("kern", KERNS)
def test_numpy_variance_rounding_error(kern):
    """The figures the device's fp64 variances are held to (ten times these): exact_np's variances in fp64 against the same lines in 80-bit
    arithmetic, per pool draw, worst over T_DEVICE.  Measured: 2.0e-16 - 7.8e-16 (Matern-3/2), 1.9e-16 - 4.7e-14 (Matern-5/2, the largest on
    (0.7, 1.2, 0.01)); the low-noise draws are among the smallest: the 1.7e-9 against the dense posterior is the dense solve's."""
    assert np.finfo(np.longdouble).eps < 1e-18
    for prm in POOL:
        r = var_rounding(tables(kern, 0.1, prm))
        print(f"{kern} {prm}: fp64 against 80-bit variances {r:.1e}")
        assert 0.0 < r <= VAR_TOL / 10


# ------------------------------------------------------------------------------------------------ GPU
def device_tables(bank, kern, prm, n):
    """The numpy table dicts of the first n latents from the device's own tables (Pinf and R from the model's definition)."""
    out = []
    for l in range(n):
        s, A = bank.smoother(l), bank.latent(l)["A"]
        Pinf = model(kern, 0.1, prm[l])[3]
        out.append(dict(A=A, K=s["K"], G=s["G"], P=s["P"], PF=s["P"] - np.outer(s["K"], s["P"][0]), Ps=s["Ps"], Pinf=Pinf, R=float(prm[l][2]),
                        var_s=s["Ps"][0, 0]))
    return out


def run_exact(torch, bank, Ty, tdt, T, **kw):
    ys, var, x, status = bank.smooth_exact(to_dev(torch, Ty, tdt, T), **kw)
    torch.cuda.synchronize()
    return ys.double().cpu().numpy(), None if var is None else var.double().cpu().numpy(), x.double().cpu().numpy(), status.cpu().numpy()


def assert_matches_definition(kern, dtype, Ty, tbs, dtbs, got, what=""):
    """ysmooth and x against exact_np on scipy's tables, var against exact_np on the device's own (fp64: ten times the formulas' rounding error)."""
    ys, var, x, status = got
    ref = exact_np(tbs, Ty)
    assert not status.any(), (what, status)
    em, ex = row_err(ys, ref["ys"]), row_err(x, ref["x"])
    assert em <= tol_of(dtype) and ex <= tol_of(dtype), (what, em, ex)
    dref = exact_np(dtbs, Ty)["var"]
    worst = 0.0
    for l in range(Ty.shape[0]):
        ev = var_err(var[l], dref[l])
        tol = 10 * var_rounding(dtbs[l]) if dtype == "f64" else FP32_TOL
        worst = max(worst, ev / tol)
        assert ev <= tol, (what, l, ev, tol)
    print(f"{kern} {dtype} L={Ty.shape[0]} T={Ty.shape[1]} {what}: mean {em:.1e} x {ex:.1e} var / its bound {worst:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNS)
@pytest.mark.parametrize("L", [1, 7, 67])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_parity(env, kern, L, dtype):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    bank, tbs, prm = bank_and_tables(streams, kern, L)
    n = min(L, len(POOL))
    dev = device_tables(bank, kern, prm, n)
    dtbs = [dev[l % n] for l in range(L)]
    for T in T_DEVICE:
        rng = np.random.default_rng(L * 100003 + T)
        Ty = stream_of(L, T, rng)
        if dtype == "f32":
            Ty = Ty.astype(np.float32).astype(np.float64)
        assert_matches_definition(kern, dtype, Ty, tbs, dtbs, run_exact(torch, bank, Ty, tdt, T))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_interior_keeps_the_bits_of_smooth(env, dtype):
    """T = 1025 >= head + tail on the whole pool: between the edges ysmooth holds smooth()'s bits and var the rounded var_smoothed, x is smooth()'s;
    and smooth() gives the same bits before and after a smooth_exact() on the same bank."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    L, T = 8, 1025
    for kern in KERNS:
        bank, tbs, _ = bank_and_tables(streams, kern, L)
        Ty = to_dev(torch, stream_of(L, T, np.random.default_rng(21)), tdt, T)
        y0, x0, _ = bank.smooth(Ty)
        y0, x0 = y0.clone(), x0.clone()
        ys, var, x, status = bank.smooth_exact(Ty)
        y1, x1, _ = bank.smooth(Ty)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(x0, x1)
        assert not status.cpu().numpy().any()
        head, tail = bank.edge_lengths()
        assert np.all(head + tail <= T)
        vs = torch.from_numpy(bank.latent_variances()[1]).to(tdt).cuda()
        for l in range(L):
            a, b = int(head[l]), T - int(tail[l])
            assert torch.equal(ys[l, a:b], y0[l, a:b]), (kern, l)
            assert not torch.equal(ys[l, :a], y0[l, :a]), (kern, l)
            assert bool((var[l, a:b] == vs[l]).all()), (kern, l)
            assert bool((var[l, 0] > vs[l]) & (var[l, T - 1] > vs[l])), (kern, l)
        assert torch.equal(x, x0)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNS)
def test_scan_and_serial_paths_agree(env, kern):
    torch, streams = env["torch"], env["streams"]
    L = 8
    bank, tbs, prm = bank_and_tables(streams, kern, L)
    dtbs = device_tables(bank, kern, prm, L)
    for T in (63, 300, 1025):
        Ty = stream_of(L, T, np.random.default_rng(22 + T))
        res = []
        for path in (0, 1):
            bank.set_option("smoother_path", path)
            res.append(run_exact(torch, bank, Ty, torch.float64, T))
            assert_matches_definition(kern, "f64", Ty, tbs, dtbs, res[-1], f"path {path}")
        assert row_err(res[0][0], res[1][0]) <= FP64_TIGHT and row_err(res[0][2], res[1][2]) <= FP64_TIGHT
    bank.set_option("smoother_path", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNS)
def test_edge_lengths_match_numpy(env, kern):
    torch, streams = env["torch"], env["streams"]
    pool = POOL + ([SLOW] if kern == "Matern52" else [])
    bank, tbs, _ = bank_and_tables(streams, kern, len(pool), pool=pool)
    head, tail = bank.edge_lengths()
    ref = np.array([edge_lengths_np(tb) for tb in tbs])
    print(kern, "head", head, "tail", tail, "numpy", ref.T)
    assert head.dtype.kind == "i" and head.shape == (len(pool),) and tail.shape == (len(pool),)
    assert np.all(np.abs(head - ref[:, 0]) <= 1) and np.all(np.abs(tail - ref[:, 1]) <= 1)
    assert np.all(head < EDGE_CAP)
    if kern == "Matern52":
        assert 6000 < head[-1] < 8000


@pytest.mark.gpu
def test_overlapping_edges_beyond_the_scratch_limit_give_status_3(env):
    """Matern-5/2 (1, 50, 1) beside ordinary pool latents: at T = 4100 its edges overlap and the stream is longer than 4096 ticks -- status 3, the row,
    the end state and the variance are the steady ones; at T = 4096 the scratch rows carry it and it agrees with the definition.  The pool
    latents beside it are exact at both lengths."""
    torch, streams = env["torch"], env["streams"]
    pool = [POOL[0], SLOW, POOL[1], POOL[2]]
    L, slow = len(pool), 1
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L, pool=pool)
    dtbs = device_tables(bank, "Matern52", prm, L)
    head, tail = bank.edge_lengths()
    assert head[slow] + tail[slow] > 4100 and np.all((head + tail)[[0, 2, 3]] < 4096)
    for T in (4100, 4096):
        Ty = stream_of(L, T, np.random.default_rng(23))
        dev = to_dev(torch, Ty, torch.float64, T)
        y0, x0, _ = bank.smooth(dev)
        y0, x0 = y0.clone(), x0.clone()
        ys, var, x, status = bank.smooth_exact(dev)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        got = (ys.cpu().numpy(), var.cpu().numpy(), x.cpu().numpy(), np.zeros(L, dtype=np.int32))
        if T == 4100:
            assert list(st) == [0, 3, 0, 0]
            assert torch.equal(ys[slow], y0[slow]) and torch.equal(x[slow], x0[slow])
            assert bool((var[slow] == bank.latent_variances()[1][slow]).all())
            ref = exact_np(tbs, Ty)
            assert list(ref["status"]) == [0, 3, 0, 0]
            keep = [0, 2, 3]
            assert_matches_definition("Matern52", "f64", Ty[keep], [tbs[l] for l in keep], [dtbs[l] for l in keep], tuple(g[keep] for g in got), "T 4100")
        else:
            assert not st.any()
            assert not torch.equal(ys[slow], y0[slow]) and not torch.equal(x[slow], x0[slow])
            assert_matches_definition("Matern52", "f64", Ty, tbs, dtbs, got, "T 4096")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("T", [17, 300, 1025])
def test_nothing_outside_the_rows(env, dtype, T):
    """Poisoned stream padding, sentinel-filled ysmooth and var slabs of another row stride than the stream's: the padding and the row past the last
    latent stay as they were; without var no variance is written and ysmooth is the same; NaN ticks (tick 0 and T - 1 among them) give finite rows."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    L = 7
    for kern in KERNS:
        bank, tbs, _ = bank_and_tables(streams, kern, L)
        rng = np.random.default_rng(24 + T)
        Ty = gaps_ends_run_copy(stream_of(L, T, rng), rng)
        assert np.isnan(Ty[:, 0]).all() and np.isnan(Ty[:, T - 1]).all()
        dev = to_dev_poison(torch, Ty, tdt, T)
        yslab, yview = sentinel_out(torch, 1, L, T, tdt)
        vslab, vview = sentinel_out(torch, 1, L, T, tdt, pad_row=12)
        with pytest.raises(ValueError):
            bank.smooth_exact(dev, ysmooth=yview[0], var=vview[0])          # one row stride serves both
        vslab, vview = sentinel_out(torch, 1, L, T, tdt)
        assert yview.stride(1) != dev.stride(0)
        ys, var, x, status = bank.smooth_exact(dev, ysmooth=yview[0], var=vview[0])
        torch.cuda.synchronize()
        assert padding_untouched(torch, yslab, yview) and padding_untouched(torch, vslab, vview)
        assert not status.cpu().numpy().any()
        assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(var).all()) and bool(torch.isfinite(x).all())
        assert bool((var > 0).all())
        ref = exact_np(tbs, Ty)
        assert row_err(ys.double().cpu().numpy(), ref["ys"]) <= tol_of(dtype)
        assert var_err(var.double().cpu().numpy(), ref["var"]) <= (1e-7 if dtype == "f64" else FP32_TOL)      # (scipy's tables: test_exact_parity is the sharp one)
        y2, v2, x2, _ = bank.smooth_exact(dev, want_var=False)
        torch.cuda.synchronize()
        assert v2 is None and torch.equal(y2, ys) and torch.equal(x2, x)


@pytest.mark.gpu
def test_smooth_outputs_exact_end_to_end(env, hip_built):
    """project -> exact_np -> un-project in numpy against smooth_outputs_exact and against MOIHGPRegression::predictSmoothedExact."""
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MOIHGP, MoihgpError
    rng = np.random.default_rng(25)
    M, L, T = 12, 5, 200
    ticks = (0, -1, 7, T - 3)
    params, Y = end_to_end_inputs(rng, M, L, T, False)
    exe = cxx_test_binary(hip_built, "smooth_exact_test")
    for kern in KERNS:
        gp = MOIHGP(0.1, M, L, kernel=KMAP[kern])
        gp.update(params)
        U, S, igp, Ty = project_np(gp, Y)
        ref = exact_np([tables(kern, 0.1, igp[l]) for l in range(L)], Ty)
        Yref = ((U * np.sqrt(S)) @ ref["ys"]).T
        Vref = np.array([(U ** 2) @ (S * ref["var"][:, t]) for t in ticks])
        Ys, varY = streams.smooth_outputs_exact(gp, torch.from_numpy(Y).cuda(), var_ticks=ticks)
        torch.cuda.synchronize()
        assert Ys.shape == (T, M) and varY.shape == (len(ticks), M) and varY.dtype == np.float64
        scale = float(np.max(np.abs(Yref)))
        assert np.max(np.abs(Ys.cpu().numpy() - Yref)) <= FP64_TIGHT * scale
        assert np.max(np.abs(varY - Vref) / Vref) <= 1e-8
        assert np.all(varY[0] > 1.2 * varY[2])                                # tick 0 is known worse than tick 7
        inp = (f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T}\n{cxx_fmt(params)}\n" + "\n".join(cxx_fmt(y) for y in Y) +
               f"\n{len(ticks)}\n" + " ".join(str(t) for t in ticks) + "\n")
        got = cxx_rows(cxx_run(exe, inp))
        assert got.shape == (T + len(ticks), M)
        assert np.max(np.abs(got[:T] - Yref)) <= FP64_TIGHT * scale
        assert np.max(np.abs(got[T:] - Vref) / Vref) <= 1e-8
        assert np.max(np.abs(got[:T] - Ys.cpu().numpy())) <= 1e-12 * scale
    bad = params.copy()
    bad[-3 * L + 3] = np.nan                                                 # latent 1's magnitude
    gp.update(bad)
    with pytest.raises(MoihgpError, match="non-zero status"):
        streams.smooth_outputs_exact(gp, torch.from_numpy(Y).cuda())


@pytest.mark.gpu
def test_failed_latent_gives_nan_rows_and_status_1(env):
    torch, streams = env["torch"], env["streams"]
    L, T, bad = 7, 300, 3
    bank, tbs, prm = bank_and_tables(streams, "Matern52", L)
    prm[bad, 0] = np.nan
    bank.update(prm)
    Ty = stream_of(L, T, np.random.default_rng(26))
    ys, var, x, st = run_exact(torch, bank, Ty, torch.float64, T)
    assert st[bad] == 1 and np.all(np.isnan(ys[bad])) and np.all(np.isnan(var[bad])) and np.all(np.isnan(x[bad]))
    keep = [l for l in range(L) if l != bad]
    assert not st[keep].any()
    ref = exact_np([tbs[l] for l in keep], Ty[keep])
    assert row_err(ys[keep], ref["ys"]) <= FP64_TIGHT and row_err(x[keep], ref["x"]) <= FP64_TIGHT
    assert var_err(var[keep], ref["var"]) <= 1e-7


@pytest.mark.gpu
def test_bad_calls_return_the_first_error(env):
    torch, streams = env["torch"], env["streams"]
    from multioutputihgp_amd import MoihgpError
    from multioutputihgp_amd._lib import last_error
    L, T, ld = 4, 64, 64
    bank, _, _ = bank_and_tables(streams, "Matern52", L)
    lib = bank._lib
    buf = torch.zeros((3 * L + 1, ld), dtype=torch.float64, device="cuda")
    x = torch.zeros((L, bank.d), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    Ty, ys, var = buf[:L], buf[L:2 * L], buf[2 * L:3 * L]

    def call(h, Ty=Ty, ys=ys, var=var, ld_in=ld, ld_out=ld, x=x, T=T):
        return lib.moihgp_smooth_stream_exact(h, 0, p(Ty), T, ld_in, p(x) if x is not None else None, p(ys), p(var) if var is not None else None,
                                              ld_out, None, None)

    assert call(bank._h) == 0 and call(bank._h, var=None) == 0
    assert call(bank._h, var=buf[L + 1:2 * L + 1]) == 1 and "var must not overlap ysmooth" in last_error(lib)
    assert call(bank._h, var=Ty) == 1 and "var must not overlap the input stream" in last_error(lib)
    assert call(bank._h, ys=Ty) == 1 and "ysmooth must not overlap the input stream" in last_error(lib)
    assert call(bank._h, ld_out=ld + 1) == 1 and "ld_out" in last_error(lib)
    assert call(bank._h, ld_in=ld + 1) == 1 and "ld (" in last_error(lib)
    assert call(bank._h, ys=buf[L:2 * L, 1:]) == 1 and "16-byte aligned" in last_error(lib)
    assert call(bank._h, ys=Ty, ld_out=ld + 1) == 1 and "ld_out" in last_error(lib)      # the strides come before the overlaps
    assert call(bank._h, x=None) == 1 and "null" in last_error(lib)
    assert call(None) == 1
    assert lib.moihgp_edge_lengths(None, None, None) == 1
    assert lib.moihgp_edge_lengths(bank._h, None, None) == 0
    torch.cuda.synchronize()
    stacked = streams.LatentBank(0.1, np.tile([1.0, 1.0, 1.0, 2.0, 0.1], (L, 1)), kernel="Matern32x2")
    xs = torch.zeros((L, stacked.d), dtype=torch.float64, device="cuda")
    assert call(stacked._h, x=xs) == 3
    assert call(stacked._h, x=xs, var=Ty) == 1                                           # ... and the argument checks before the model's
    assert lib.moihgp_edge_lengths(stacked._h, None, None) == 3
    with pytest.raises(MoihgpError) as e:
        stacked.smooth_exact(Ty)
    assert e.value.rc == 3
    with pytest.raises(MoihgpError):
        stacked.edge_lengths()
