"""The stream sweeps (smooth, forecast, lagged, forecast_tail and the two variance tables) on latents that decay slowly.

The other stream tests draw every latent from stream_support.POOL (lengthscales 0.5 .. 2.0 at dt = 0.1): anything further than a few hundred ticks
away has decayed to nothing there, so a forecast plane at h = 300, a lag of 1023 or the far blocks of a tail of 4096 are compared against numbers
far below any tolerance.  Three slow rows (magnitude, lengthscale, noise variance), mixed into a bank with POOL rows so that no slow row is alone
in a launch, keep those parts of the kernels above it:

    SLOW = [(1.0, 50.0, 0.1), (0.8, 200.0, 0.1), (1.2, 100.0, 0.02)]

What they carry, measured with the numpy definitions on the very streams, horizons and lags the GPU tests use (the CPU tests below assert these
figures against thresholds; the least over every case, Matern-3/2 / Matern-5/2 where two are given):
  growth figures (inf-norm of the powers 1 .. 32 and of the 1024th): G <= 94, Kalman A - K H A <= 28, the handle's AKHA (Matern-3/2) <= 34,
      all under the fp32 bound of 1e2: every slow row takes the scan kernels in both precisions
  forecast planes of (0.8, 200, 0.1), maximum over the latent's h = 0 scale, Kalman gains: h = 300 1.9 / 1.6, h = 1023 and 1024 2.8 / 2.4,
      h = 4096 0.69 / 1.0; the handle's gains (Matern-3/2): 0.56, 0.048, 0.016 (threshold 1e-3)
  lagged planes of (0.8, 200, 0.1), over the row maximum: lag 300 differs from the smoothed mean by 0.048 / 0.11, lag 1023 by 8.8e-5 / 2.9e-3
      (threshold 1e-5), lags 1023 and 1024 from each other by 9.5e-6 / 3.1e-4 (threshold 1e-6)
  variances: the forecast deficit (Pinf_00 - var) / Pinf_00 is 0.58 .. 0.98 at h = 300 and >= 0.022 at h = 1024 on the three slow rows; the
      lagged excess over var_smoothed at lag 300 is 1.6e-2 / 3.1e-2 of it on (0.8, 200, 0.1) (thresholds 1e-3)
  tail of 4096 of (0.8, 200, 0.1): the least maximum of a 1024-block is 0.10 / 0.81 of the row maximum, the value at j = 4095 0.065 / 0.57
  a sequential float32 walk of the forecast recursion in numpy against the fp64 one, every qualifying plane against its own maximum: at most
      8.3e-6 / 1.1e-5 (Kalman gains), 2.2e-5 (handle), under the 3e-4 that leaves half a decade to the fp32 tolerance

A forecast plane of a latent "qualifies" where its maximum is at least 1e-3 of that latent's h = 0 scale; it is then also held against its own
maximum.  Tolerances are the project's (1e-9 fp64, 1e-3 fp32) throughout."""
import functools

import numpy as np
import pytest

from conftest import rel_err_rows
from parity_support import synth
from stream_reference import forecast_np, forecast_var_np, forward_np, gain_tables, lagged_np, lagged_var_np, smooth_np, tables
from stream_support import (HMAX, LAGS8, LMAX, POOL, bank_and_tables, env, gaps_edges_blocks_inplace, make_bank, padding_untouched, plane_err,
                            round32, sentinel_out, tdt_of, to_dev, tol_of)  # noqa: F401  (env: the module's fixture)

SLOW = [(1.0, 50.0, 0.1), (0.8, 200.0, 0.1), (1.2, 100.0, 0.02)]
FAR_PRM = SLOW[1]
# the bank: the slow rows first, the slowest on an even row (gaps_edges_blocks_inplace blanks ticks 1024 .. 2047 of the odd rows, which would leave it nothing to
# tell lag 1023 from the smoother by), then four POOL rows, the R = 1e-6 one among them
BANK = [SLOW[0], SLOW[2], SLOW[1], POOL[3], POOL[0], POOL[1], POOL[4]]
L = len(BANK)
SLOW_ROWS = [BANK.index(p) for p in SLOW]
FAR = BANK.index(FAR_PRM)
NAN_ROW = 5                                              # entirely missing in the gap variant of the forecast streams
DT = 0.1
TS = (15, 16, 17, 1023, 1024, 1025, 2048, 2049)          # a stream that ends on a chunk (16 ticks) or a segment (1024), and one tick either side
FC_HORIZONS = [1, 0, 7, 300, 1023, 1024, 4096, HMAX]     # K = 8, the most one call takes
FC_MODES = [("Matern32", "kalman"), ("Matern32", "handle"), ("Matern52", "kalman")]    # (the slow rows are unstable under the Matern-5/2 handle gains)
LAGS2 = [300, 40]
LAG_TS = (2049, 2100)
STATE_ATS = (15, 16, 17, 1023, 1024, 1025)
TAIL_NS = (1, 63, 64, 65, 1023, 1024, 1025, 4096)
VAR_HORIZONS = [0, 1, 300, 1024, 4096, HMAX]
VAR_LAGS = [0, 1, 16, 300]
QUALIFY = 1e-3                                           # a plane / block / variance term is held against its own size from here up
HANDLE_TABLE_TOL = 1e-5                                  # the handle's literal tables on the slow rows: thirty times their measured own error
F32_INPUT_BOUND = 3e-4                                 # half a decade under FP32_TOL, as tests/test_parameter_box.py keeps


def _norm_inf(X):
    return float(np.max(np.sum(np.abs(X), axis=1)))


def growth_figure(X):
    """As chunk_powers / segment_growth of the tables kernels: the largest inf-norm of X^1 .. X^32 and of X^1024."""
    g, P = 0.0, np.eye(X.shape[0])
    for _ in range(32):
        P = X @ P
        g = max(g, _norm_inf(P))
    return max(g, _norm_inf(np.linalg.matrix_power(X, 1024)))


@functools.lru_cache(maxsize=None)
def bank_tables(kern, gains="smoother"):
    """One numpy table dict per row of BANK: the smoother's (tables) or a forecast mode's (gain_tables)."""
    if gains == "smoother":
        return tuple(tables(kern, DT, p) for p in BANK)
    return tuple(gain_tables(kern, DT, p, gains) for p in BANK)


def start_state(kern, rng, size):
    """A start state of the stationary prior's proportions: component i (the i-th derivative) of latent l is drawn at size * lambda_l^i, lambda =
    sqrt(2 nu) / lengthscale.  Components of equal size would be derivatives ~1/lambda^i too large for a slow latent, whose far horizons (which
    weigh them by ~(h dt)^i) would then exceed the h = 0 scale the planes are measured against by three decades on the short streams."""
    d = 2 if kern == "Matern32" else 3
    lam = np.array([np.sqrt(2 * d - 1) / p[1] for p in BANK])
    return round32(size * rng.standard_normal((L, d)) * lam[:, None] ** np.arange(d)[None, :])


def _stream(T, rng, variant):
    Ty = synth(L, T, rng)
    if variant != "dense":
        Ty = gaps_edges_blocks_inplace(Ty, rng)
    return Ty


# ------------------------------------------------------------------------------------------------ cases, built once and kept unchanged
@functools.lru_cache(maxsize=None)
def forecast_case(kern, gains, T, variant):
    """Stream, start state and numpy reference of one forecast case, shared by the dtypes (the data are fp32 numbers), by the CPU conditions and by
    the GPU tests.  own[k][l]: the maximum of plane k of latent l; qual: where it reaches QUALIFY of the latent's h = 0 scale."""
    rng = np.random.default_rng([FC_MODES.index((kern, gains)), T, ("dense", "gaps").index(variant), 41])
    tbs = list(bank_tables(kern, gains))
    Ty = _stream(T, rng, variant)
    if variant == "gaps":
        Ty[NAN_ROW] = np.nan
    Ty = round32(Ty)
    x0 = start_state(kern, rng, 0.1)
    ref, xe, scale = forecast_np(tbs, Ty, FC_HORIZONS, x0)
    own = np.max(np.abs(ref), axis=-1)
    return dict(Ty=Ty, x0=x0, ref=ref, xe=xe, scale=scale, own=own, qual=own >= QUALIFY * scale[None, :])


def forecast_f32_np(tbs, Ty, horizons, x0):
    """forecast_np's recursion walked tick by tick in float32 (tables rounded once from fp64, as the library's fp32 copy of them is)."""
    f = np.float32
    A = np.stack([t["A"] for t in tbs]).astype(f); K = np.stack([t["K"] for t in tbs]).astype(f); M = np.stack([t["M"] for t in tbs]).astype(f)
    c = np.array([[np.linalg.matrix_power(t["A"], int(h))[0] for t in tbs] for h in horizons]).astype(f)
    Ty32 = Ty.astype(f)
    x = x0.astype(f)
    fc = np.zeros((len(horizons),) + Ty.shape, dtype=f)
    for t in range(Ty.shape[1]):
        y = Ty32[:, t]
        miss = np.isnan(y)
        xo = np.einsum("lij,lj->li", M, x) + K * np.where(miss, f(0), y)[:, None]
        xm = np.einsum("lij,lj->li", A, x)
        x = np.where(miss[:, None], xm, xo)
        fc[:, :, t] = np.einsum("kld,ld->kl", c, x)
    assert fc.dtype == f and x.dtype == f
    return fc.astype(np.float64)


@functools.lru_cache(maxsize=None)
def smooth_case(kern, T, variant):
    rng = np.random.default_rng([("Matern32", "Matern52").index(kern), T, ("dense", "gaps").index(variant), 42])
    tbs = list(bank_tables(kern))
    Ty = round32(_stream(T, rng, variant))
    x0 = start_state(kern, rng, 0.1)
    ref, xe = smooth_np(tbs, Ty, x0)
    return dict(Ty=Ty, x0=x0, ref=ref, xe=xe)


@functools.lru_cache(maxsize=None)
def lagged_case(kern, T):
    rng = np.random.default_rng([("Matern32", "Matern52").index(kern), T, 43])
    tbs = list(bank_tables(kern))
    Ty = round32(_stream(T, rng, "gaps"))
    x0 = start_state(kern, rng, 0.1)
    ref, p, xe = lagged_np(tbs, Ty, LAGS8 + LAGS2, x0)
    return dict(Ty=Ty, x0=x0, p=p, xe=xe, ref={"8": ref[:8], "2": ref[8:]})


@functools.lru_cache(maxsize=None)
def tail_case(kern):
    """A start state with every derivative component set (start_state), and tail[l][j] = H A^(j+1) x_l for j < 4096."""
    rng = np.random.default_rng([("Matern32", "Matern52").index(kern), 44])
    A = np.stack([t["A"] for t in bank_tables(kern)])
    x0 = start_state(kern, rng, 1.0)
    n = max(TAIL_NS)
    ref = np.zeros((L, n)); v = x0.copy()
    for j in range(n):
        v = np.einsum("lij,lj->li", A, v)
        ref[:, j] = v[:, 0]
    return dict(x0=x0, ref=ref)


def _blocks(n):
    return [(b, min(b + 1024, n)) for b in range(0, n, 1024)]


def forecast_var_terms(tb, h):
    """(variance, deficit Pinf_00 - variance) at horizon h, the deficit formed directly (no cancellation against Pinf_00)."""
    c = np.linalg.matrix_power(tb["A"], int(h))[0]
    deficit = float(c @ (tb["Pinf"] - tb["PF"]) @ c)
    return forecast_var_np(tb, h), deficit


def lagged_var_terms(tb, l):
    """(variance, excess over var_smoothed) at lag l, the excess formed directly."""
    g = np.linalg.matrix_power(tb["G"], int(l))[0]
    return lagged_var_np(tb, l), float(g @ (tb["PF"] - tb["Ps"]) @ g)


# ------------------------------------------------------------------------------------------------ CPU: the conditions on the inputs
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_slow_rows_are_solved_and_take_the_scan_route(kern):
    """scipy's DARE passes tables()'s residual check on every slow row, and the growth figures of G, of the Kalman A - K H A and (Matern-3/2) of
    the handle's AKHA stay under the fp32 bound of the scan kernels (scan_growth_bound: 1e2 fp32, 1e4 fp64)."""
    for prm in SLOW:
        tb = tables(kern, DT, prm)
        assert tb is not None, prm
        figs = dict(G=growth_figure(tb["G"]), kalman=growth_figure(tb["A"] - np.outer(tb["K"], tb["A"][0])))
        if kern == "Matern32":
            figs["handle"] = growth_figure(gain_tables(kern, DT, prm, "handle")["M"])
        print(f"{kern} {prm}: growth {', '.join('%s %.3g' % kv for kv in figs.items())}")
        assert max(figs.values()) <= 1e2, (prm, figs)


def test_handle_gains_of_the_slow_rows_are_defined_to_rounding_only():
    """The reference's literal DARE (100 iterations at the most, from P = Q) has not converged on the slow Matern-3/2 rows, and its start
    Q = Pinf - A Pinf A^T cancels to ~(lambda dt)^3 of its terms: moving entries of A by one unit in the last place moves K by up to 3e-7 of itself
    (measured: 5e-9, 3e-8, 3e-7 for lengthscales 50, 100, 200).  That is above FP64_TIGHT, which is why the handle-gain sweeps are compared with
    numpy on the device's own tables, and it stays a decade and a half under HANDLE_TABLE_TOL, which those tables are held to."""
    from oracle.moihgp_numpy import IHGP, dare
    rng = np.random.default_rng(45)
    for prm in SLOW:
        g = IHGP(DT, "Matern32")
        g.update(np.asarray(prm, dtype=np.float64))
        assert not g.dare_converged and g.dare_iters == 100, prm

        def gain(A):
            Q = g.ss.Pinf - A @ g.ss.Pinf @ A.T
            P, _, _ = dare(A, g.ss.H.T, (Q + Q.T) / 2.0, g.ss.R)
            return (P @ g.ss.H.T / (g.ss.H @ P @ g.ss.H.T + g.ss.R)[0, 0])[:, 0]
        K0 = gain(g.A)
        assert np.array_equal(K0, g.K[:, 0])
        moved = max(float(np.max(np.abs(gain(np.nextafter(g.A, rng.choice([-np.inf, np.inf], g.A.shape))) - K0) / np.abs(K0))) for _ in range(8))
        print(f"Matern32 {prm}: K moves by {moved:.2g} of itself when entries of A move by one unit in the last place")
        assert moved <= HANDLE_TABLE_TOL / 10, (prm, moved)


@pytest.mark.parametrize("kern,gains", FC_MODES)
def test_forecast_streams_carry_signal_at_every_horizon(kern, gains):
    """Every horizon but HMAX qualifies on some latent of the bank, and every horizon <= 4096 on (0.8, 200, 0.1), in every forecast case."""
    low = {h: np.inf for h in FC_HORIZONS}
    for T in TS:
        for variant in ("dense", "gaps"):
            case = forecast_case(kern, gains, T, variant)
            for k, h in enumerate(FC_HORIZONS):
                if h == HMAX:
                    continue
                assert case["qual"][k].any(), (T, variant, h)
                assert case["qual"][k, FAR], (T, variant, h, case["own"][k, FAR] / case["scale"][FAR])
                low[h] = min(low[h], case["own"][k, FAR] / case["scale"][FAR])
            assert np.all(np.isfinite(case["ref"])) and np.all(np.isfinite(case["xe"]))
    print(f"{kern} {gains}: least plane maximum over the h = 0 scale on {FAR_PRM}: " + ", ".join(f"h={h} {v:.2g}" for h, v in low.items() if h != HMAX))


@pytest.mark.parametrize("kern,gains", FC_MODES)
def test_fp32_forecast_streams_leave_margin_under_the_fp32_tolerance(kern, gains):
    """A condition on the inputs, not on the library: the forecast recursion walked in float32 in numpy stays within F32_INPUT_BOUND of the fp64
    reference on every qualifying plane, each against its own maximum, so that FP32_TOL is a fair demand of the fp32 sweep."""
    worst = 0.0
    for T in TS:
        for variant in ("dense", "gaps"):
            case = forecast_case(kern, gains, T, variant)
            f32 = forecast_f32_np(list(bank_tables(kern, gains)), case["Ty"], FC_HORIZONS, case["x0"])
            err = np.where(case["qual"], np.max(np.abs(f32 - case["ref"]), axis=-1) / np.maximum(case["own"], 1e-300), 0.0)
            assert np.max(err) <= F32_INPUT_BOUND, (T, variant, np.unravel_index(np.argmax(err), err.shape), float(np.max(err)))
            worst = max(worst, float(np.max(err)))
    print(f"{kern} {gains}: float32 walk against fp64, worst qualifying plane over its own maximum {worst:.2g}")


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_lagged_streams_tell_the_long_lags_apart(kern):
    """On (0.8, 200, 0.1): the lag-300 and lag-1023 planes differ from the lag-LMAX plane (the smoothed mean) by >= 1e-5 of the row maximum, and
    lags 1023 and 1024 from each other by >= 1e-6 of it."""
    for T in LAG_TS:
        ref = lagged_case(kern, T)["ref"]
        pl = {l: ref["8"][LAGS8.index(l)][FAR] for l in (1023, 1024, LMAX)}
        pl[300] = ref["2"][LAGS2.index(300)][FAR]
        top = np.max(np.abs(pl[LMAX]))
        d300, d1023, dd = (np.max(np.abs(pl[300] - pl[LMAX])) / top, np.max(np.abs(pl[1023] - pl[LMAX])) / top,
                           np.max(np.abs(pl[1023] - pl[1024])) / top)
        print(f"{kern} T={T}: lag 300 vs smoothed {d300:.2g}, lag 1023 vs smoothed {d1023:.2g}, lag 1023 vs 1024 {dd:.2g} (of the row maximum)")
        assert d300 >= 1e-5 and d1023 >= 1e-5, (T, d300, d1023)
        assert dd >= 1e-6, (T, dd)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_variances_are_off_their_limits_at_the_long_horizons_and_lags(kern):
    """The forecast deficit (Pinf_00 - var) / Pinf_00 at h = 300 and 1024 on every slow row, and the lagged excess (var - var_smoothed) /
    var_smoothed at lag 300 on (0.8, 200, 0.1), are >= 1e-3: the terms c (Pinf - PF) c^T and g (PF - Ps) g^T are visible."""
    tbs = bank_tables(kern)
    for l in SLOW_ROWS:
        for h in (300, 1024):
            _, deficit = forecast_var_terms(tbs[l], h)
            print(f"{kern} {BANK[l]}: forecast deficit at h={h} {deficit / tbs[l]['Pinf'][0, 0]:.3g} of Pinf_00")
            assert deficit >= QUALIFY * tbs[l]["Pinf"][0, 0], (BANK[l], h)
    _, excess = lagged_var_terms(tbs[FAR], 300)
    print(f"{kern} {FAR_PRM}: lagged excess at lag 300 {excess / tbs[FAR]['var_s']:.3g} of var_smoothed")
    assert excess >= QUALIFY * tbs[FAR]["var_s"]


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_tail_reaches_every_block(kern):
    """On (0.8, 200, 0.1) each of the four 1024-blocks of a tail of 4096 has a maximum >= 1e-3 of the row maximum."""
    ref = tail_case(kern)["ref"][FAR]
    parts = [np.max(np.abs(ref[a:b])) / np.max(np.abs(ref)) for a, b in _blocks(4096)]
    print(f"{kern} {FAR_PRM}: tail block maxima over the row maximum {['%.2g' % p for p in parts]}, j = 4095: {abs(ref[4095]) / np.max(np.abs(ref)):.2g}")
    assert min(parts) >= QUALIFY, parts


# ------------------------------------------------------------------------------------------------ GPU
_HANDLE_CASES = {}


def _handle_case_on_device_tables(bank, tbs, case, kern, T, variant):
    """The handle's gains come from the reference's literal DARE, which stops after 100 iterations far from its fixed point on the slow rows and
    starts from Q = Pinf - A Pinf A^T, a difference ~1e-9 of its terms: numpy's K is defined to HANDLE_TABLE_TOL there and no better
    (test_handle_gains_of_the_slow_rows_are_defined_to_rounding_only), so forecast_np runs on the device's own A, K and AKHA, as
    test_forecast.test_growth_bound_fallback_kalman does for its reason.  The device's tables are held to numpy's at that figure, which keeps
    the CPU conditions (margins of decades) valid for the case."""
    key = (kern, T, variant)
    if key not in _HANDLE_CASES:
        dtb = []
        for l in range(L):
            lt = bank.latent(l)
            for name, mine in (("A", "A"), ("K", "K"), ("AKHA", "M")):
                assert np.max(np.abs(lt[name] - tbs[l][mine])) <= HANDLE_TABLE_TOL * np.max(np.abs(tbs[l][mine])), (BANK[l], name)
            dtb.append(dict(A=lt["A"], K=lt["K"], M=lt["AKHA"]))
        ref, xe, scale = forecast_np(dtb, case["Ty"], FC_HORIZONS, case["x0"])
        own = np.max(np.abs(ref), axis=-1)
        qual = own >= QUALIFY * scale[None, :]
        assert qual[:FC_HORIZONS.index(HMAX), FAR].all()
        _HANDLE_CASES[key] = dict(case, ref=ref, xe=xe, scale=scale, own=own, qual=qual)
    return _HANDLE_CASES[key]


def _run_forecast(env, kern, gains, T, dtype, variant, K=8, alias=False):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    case = forecast_case(kern, gains, T, variant)
    hs = FC_HORIZONS[:K]
    bank, tbs, _ = make_bank(streams, kern, L, gains, pool=BANK)
    if gains == "handle":
        case = _handle_case_on_device_tables(bank, tbs, case, kern, T, variant)
    ref, qual, own, scale = case["ref"][:K], case["qual"][:K], case["own"][:K], case["scale"]
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    slab, out = sentinel_out(torch, K, L, T, tdt)            # ld_out != ld_in, plane_stride > L * ld_out
    if alias:
        fc, x, status = bank.forecast(to_dev(torch, case["Ty"], tdt, T), hs, x=x_start, out=out, gains=gains)
        assert x.data_ptr() == x_start.data_ptr()
    else:
        fc, x, status = bank.forecast(to_dev(torch, case["Ty"], tdt, T), hs, x=torch.empty_like(x_start), x_start=x_start, out=out, gains=gains)
    torch.cuda.synchronize()
    got = fc.double().cpu().numpy()
    errs = [plane_err(got[k], ref[k], scale) for k in range(K)]
    with np.errstate(invalid="ignore"):
        eown = np.where(qual, np.max(np.abs(got - ref), axis=-1) / np.maximum(own, 1e-300), 0.0)
    ex = rel_err_rows(x.double().cpu().numpy(), case["xe"], floor=1e-3)
    print(f"forecast {kern} {gains} {dtype} T={T} {variant} K={K}: planes over h=0 scale {max(errs):.1e}, qualifying planes over their own maximum "
          f"{np.max(eown):.1e} (plane, latent) {np.unravel_index(np.argmax(eown), eown.shape)}, end state {ex:.1e}")
    assert not status.cpu().numpy().any(), status.cpu().numpy()
    assert max(errs) <= tol_of(dtype), errs
    assert np.max(eown) <= tol_of(dtype), eown
    assert ex <= tol_of(dtype), ex
    assert padding_untouched(torch, slab, out)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dense", "gaps"])
@pytest.mark.parametrize("kern,gains", FC_MODES)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forecast_parity(env, kern, gains, T, dtype, variant):
    """Dense streams (whole wavefronts on the branch without selects) and gapped ones (gaps_edges_blocks_inplace) with one row entirely missing, K = 8 horizons out to
    4096 and HMAX: every plane against the h = 0 scale, and every qualifying plane of a latent against its own maximum."""
    _run_forecast(env, kern, gains, T, dtype, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forecast_parity_x_aliases_x_start(env, dtype):
    _run_forecast(env, "Matern52", "kalman", 2049, dtype, "gaps", alias=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forecast_parity_seven_horizons(env, dtype):
    """K = 7: the second plane of the last group of two is idle."""
    _run_forecast(env, "Matern32", "kalman", 1025, dtype, "gaps", K=7)


def _run_smooth(env, kern, T, dtype, variant, alias=False):
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    case = smooth_case(kern, T, variant)
    bank, _, _ = bank_and_tables(streams, kern, L, pool=BANK)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    out = torch.full((L, (T + 3) // 4 * 4 + 8), float("nan"), dtype=tdt, device="cuda")       # ld_out != ld_in
    if alias:
        ys, x, status = bank.smooth(to_dev(torch, case["Ty"], tdt, T), x=x_start, ysmooth=out[:, :T])
        assert x.data_ptr() == x_start.data_ptr()
    else:
        ys, x, status = bank.smooth(to_dev(torch, case["Ty"], tdt, T), x=torch.empty_like(x_start), x_start=x_start, ysmooth=out[:, :T])
    torch.cuda.synchronize()
    ey = rel_err_rows(ys.double().cpu().numpy(), case["ref"])
    ex = rel_err_rows(x.double().cpu().numpy(), case["xe"], floor=1e-3)
    print(f"smooth {kern} {dtype} T={T} {variant}: rows {ey:.1e}, end state {ex:.1e}")
    assert not status.cpu().numpy().any(), status.cpu().numpy()
    assert ey <= tol_of(dtype), ey
    assert ex <= tol_of(dtype), ex
    assert bool(torch.isnan(out[:, T:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dense", "gaps"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_smooth_parity(env, kern, T, dtype, variant):
    _run_smooth(env, kern, T, dtype, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_smooth_parity_x_aliases_x_start(env, kern):
    _run_smooth(env, kern, 1025, "f64", "gaps", alias=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("T", LAG_TS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lagged_parity(env, kern, T, dtype):
    """LAGS8 and [300, 40] on gapped streams (gaps_edges_blocks_inplace) of 2049 and 2100 ticks.  At fp64 the planes of lags 1023 and 1024 differ from the smoothed mean
    and from each other by far more than the tolerance on (0.8, 200, 0.1); at fp32 the lag-300 plane does."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    case = lagged_case(kern, T)
    bank, _, _ = bank_and_tables(streams, kern, L, pool=BANK)
    dev = to_dev(torch, case["Ty"], tdt, T)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    for name, lags in (("8", LAGS8), ("2", LAGS2)):
        K = len(lags)
        slab, out = sentinel_out(torch, K, L, T, tdt)
        ldo = out.stride(1)
        yslab = torch.full((L * ldo + 16,), 12345.0, dtype=tdt, device="cuda")
        yp = torch.as_strided(yslab, (L, T), (ldo, 1), 0)
        lg, ypred, x, status = bank.lagged(dev, lags, x=torch.empty_like(x_start), x_start=x_start, out=out, ypred=yp)
        torch.cuda.synchronize()
        got = lg.double().cpu().numpy()
        errs = [rel_err_rows(got[k], case["ref"][name][k]) for k in range(K)]
        ep = rel_err_rows(ypred.double().cpu().numpy(), case["p"])
        ex = rel_err_rows(x.double().cpu().numpy(), case["xe"], floor=1e-3)
        print(f"lagged {kern} {dtype} T={T} lags={lags}: planes {['%.1e' % e for e in errs]}, ypred {ep:.1e}, end state {ex:.1e}")
        assert not status.cpu().numpy().any(), status.cpu().numpy()
        assert max(errs) <= tol_of(dtype), errs
        assert ep <= tol_of(dtype) and ex <= tol_of(dtype), (ep, ex)
        assert padding_untouched(torch, slab, out) and padding_untouched(torch, yslab, yp)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lagged_state_at_chunk_and_segment_edges(env, kern, dtype, path):
    """The filtered state after tick state_at - 1, with state_at on a chunk edge, a segment edge and one tick either side of each."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    T = 2100
    case = lagged_case(kern, T)
    tbs = list(bank_tables(kern))
    bank, _, _ = bank_and_tables(streams, kern, L, pool=BANK)
    bank.set_option("lagged_path", path)
    dev = to_dev(torch, case["Ty"], tdt, T)
    x_start = torch.from_numpy(case["x0"]).to(tdt).cuda()
    for s in STATE_ATS:
        lg, _, x, status = bank.lagged(dev, LAGS2, x_start=x_start, state_at=s)
        torch.cuda.synchronize()
        _, _, xref = forward_np(tbs, case["Ty"], case["x0"], state_at=s)
        ex = rel_err_rows(x.double().cpu().numpy(), xref, floor=1e-3)
        el = max(rel_err_rows(lg[k].double().cpu().numpy(), case["ref"]["2"][k]) for k in range(2))
        print(f"lagged state_at={s} {kern} {dtype} path={path}: state {ex:.1e}, planes {el:.1e}")
        assert not status.cpu().numpy().any()
        assert ex <= tol_of(dtype), (s, ex)
        assert el <= tol_of(dtype), (s, el)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tail(env, kern, dtype):
    """forecast_tail from a state with derivative components: per row as test_forecast.test_tail, and per 1024-block (one workgroup each) against
    the block's own maximum on the rows where the block reaches QUALIFY of the row maximum."""
    torch, streams = env["torch"], env["streams"]
    tdt = tdt_of(torch, dtype)
    case = tail_case(kern)
    bank, _, _ = make_bank(streams, kern, L, "kalman", pool=BANK)
    xd = torch.from_numpy(case["x0"]).to(tdt).cuda()
    for n in TAIL_NS:
        tail = bank.forecast_tail(xd, n)
        torch.cuda.synchronize()
        assert tuple(tail.shape) == (L, n)
        got, ref = tail.double().cpu().numpy(), case["ref"][:, :n]
        top = np.max(np.abs(ref), axis=1)
        erow = plane_err(got, ref, np.maximum(top, np.abs(case["x0"][:, 0])))
        eblk, nq = 0.0, 0
        for a, b in _blocks(n):
            bmax = np.max(np.abs(ref[:, a:b]), axis=1)
            q = bmax >= QUALIFY * top
            nq += int(q.sum())
            with np.errstate(invalid="ignore"):
                e = np.where(q, np.max(np.abs(got[:, a:b] - ref[:, a:b]), axis=1) / np.maximum(bmax, 1e-300), 0.0)
            eblk = max(eblk, float(np.max(e))) if not np.isnan(e).any() else np.nan
        print(f"tail {kern} {dtype} n={n}: rows {erow:.1e}, {nq} qualifying blocks over their own maximum {eblk:.1e}")
        assert erow <= tol_of(dtype), (n, erow)
        assert eblk <= tol_of(dtype), (n, eblk)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_forecast_variances(env, kern):
    """forecast_variances against numpy at 1e-10 relative, as test_forecast.test_variances_match_numpy, and the deficit Pinf_00 - var itself at
    1e-7 relative wherever it reaches QUALIFY of Pinf_00."""
    bank, tbs, _ = make_bank(env["streams"], kern, L, "kalman", pool=BANK)
    var = bank.forecast_variances(VAR_HORIZONS)
    _, _, status = bank.forecast(env["torch"].zeros((L, 8), dtype=env["torch"].float64, device="cuda"), [0])
    assert not status.cpu().numpy().any()
    assert var.shape == (len(VAR_HORIZONS), L)
    ev, ed, nq = 0.0, 0.0, 0
    for l in range(L):
        p00 = tbs[l]["Pinf"][0, 0]
        for k, h in enumerate(VAR_HORIZONS):
            ref, deficit = forecast_var_terms(tbs[l], h)
            ev = max(ev, abs(var[k, l] - ref) / ref)
            if deficit >= QUALIFY * p00:
                nq += 1
                ed = max(ed, abs((p00 - var[k, l]) - deficit) / deficit)
    print(f"forecast variances {kern}: worst relative error {ev:.1e}, of the deficit ({nq} qualifying) {ed:.1e}")
    for l in range(L):
        p00 = tbs[l]["Pinf"][0, 0]
        for k, h in enumerate(VAR_HORIZONS):
            ref, deficit = forecast_var_terms(tbs[l], h)
            assert abs(var[k, l] - ref) <= 1e-10 * ref, (BANK[l], h, var[k, l], ref)
            if deficit >= QUALIFY * p00:
                assert abs((p00 - var[k, l]) - deficit) <= 1e-7 * deficit, (BANK[l], h, p00 - var[k, l], deficit)
    for l in SLOW_ROWS:
        assert all(forecast_var_terms(tbs[l], h)[1] >= QUALIFY * tbs[l]["Pinf"][0, 0] for h in (300, 1024))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_lagged_variances(env, kern):
    """lagged_variances against numpy at 1e-10 relative, as test_lagged.test_variances_match_numpy, and the excess over var_smoothed itself at
    1e-7 relative wherever it reaches QUALIFY of var_smoothed."""
    bank, tbs, _ = bank_and_tables(env["streams"], kern, L, pool=BANK)
    var = bank.lagged_variances(VAR_LAGS)
    _, vs = bank.latent_variances()
    _, _, status = bank.smooth(env["torch"].zeros((L, 8), dtype=env["torch"].float64, device="cuda"))
    assert not status.cpu().numpy().any()
    assert var.shape == (len(VAR_LAGS), L)
    ev, ee, nq = 0.0, 0.0, 0
    for l in range(L):
        for k, lag in enumerate(VAR_LAGS):
            ref, excess = lagged_var_terms(tbs[l], lag)
            ev = max(ev, abs(var[k, l] - ref) / ref)
            if excess >= QUALIFY * tbs[l]["var_s"]:
                nq += 1
                ee = max(ee, abs((var[k, l] - vs[l]) - excess) / excess)
    print(f"lagged variances {kern}: worst relative error {ev:.1e}, of the excess over var_smoothed ({nq} qualifying) {ee:.1e}")
    for l in range(L):
        for k, lag in enumerate(VAR_LAGS):
            ref, excess = lagged_var_terms(tbs[l], lag)
            assert abs(var[k, l] - ref) <= 1e-10 * ref, (BANK[l], lag, var[k, l], ref)
            if excess >= QUALIFY * tbs[l]["var_s"]:
                assert abs((var[k, l] - vs[l]) - excess) <= 1e-7 * excess, (BANK[l], lag, var[k, l] - vs[l], excess)
    assert lagged_var_terms(tbs[FAR], 300)[1] >= QUALIFY * tbs[FAR]["var_s"]
