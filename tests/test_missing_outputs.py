"""Partially observed ticks at the limits of the least-squares projection (moihgp.h:167-178): the three pieces of device code in csrc/tick.hip that
solve  a* = argmin |U[obs] a - y[obs]|,  Ty* = S^-1/2 a*  -- the stream path (ls_project_kernel, a k x k Woodbury system per tick, both layouts),
the sharded pair (ls_shard_gram_kernel / ls_shard_apply_kernel around an all-reduce) and the per-tick path (normal_eq_kernel + spd_solve_kernel) --
held entry by entry to a truth computed on the CPU and to a bar that scales with the conditioning of the tick.

Truth: numpy.linalg.lstsq followed by three steps of iterative refinement whose residual U0^T (y0 - U0 a) is formed in numpy.longdouble.  (At
L = 2000 one lstsq takes a second and there are twenty ticks per stream: there the start vector and the correction of every step come from the
Woodbury form in fp64 instead.  The fixed point of the refinement is the same -- where the longdouble residual of the actual U vanishes -- and
test_refinement_converged_at_the_largest_shape bounds what is left of that residual.)  fp32 streams: the truth takes the fp32-rounded y, cast back
to fp64, as its exact input; U and S are the handle's own fp64 values (gp.params).

Scale: kappa = (sigma_max / sigma_min)^2 of U[obs], the condition number of the reference's normal equations and of the Woodbury matrix alike.
    fp64                 |got - Ty*| <= C_BAR 2^-52 kappa max_l |Ty*_l|                 entry by entry over the tick's column
    fp32, stream path    + 2^-24 |Ty*|                (the kernel works in fp64 and rounds once on the store)
    fp32, shard pair     + 2^-24 kappa |r|_2 / sqrt(S_l)   as well  (r = U^T (y, NaN -> 0) is rebuilt from the fp32 Ty and a = (U0^T U0)^-1 r: derived
                         from the rounding of the input, not measured)
C_BAR is not chosen: err / (2^-52 kappa max |a*|) of the two textbook routes evaluated in plain numpy fp64, measured over the cases of this file:
    ROUTE_NORMAL   =  3.2    the reference's solve(U0^T U0, U0^T y0); worst at (M, L, k) = (135, 65, 1) "rand"; every case with L <= 257 (the
                             per-tick kernels, which take this route, run at no larger L, and one such solve at L = 2000 takes seconds)
    ROUTE_WOODBURY = 24.7    the Woodbury form of tick.hip's header comment; worst at (70, 5, 65) "ends"; every case of the stream path's
                             shapes, k = M - L > 64 included although the kernels refuse it
and C_BAR = 4 x the larger = 98.8: the device sums with fma and a 64-lane butterfly in another order; the margin covers ordering, not a lost digit.
The Woodbury form is at its worst where k is many times L and kappa small (its error is that of r = U^T y0, which does not grow with kappa): on
the per-tick cases (M = L + 70, L = 4, k = 70), where no kernel takes that route, it reaches 64.8.  Those are left out of the rule: they could
only widen the bar.  test_route_constants_and_the_bar re-measures all three and holds C_BAR within a factor two of the rule on whatever BLAS
runs the suite.
Worst kappa of the case table: KAPPA_WORST = 4.8e6 at (325, 255, 70) "head" (test_cases_are_well_posed asserts the cap of 1e7 on every case; the
square systems, k = M - L, are the ones that come near it, and SEED was changed until every case stayed below).
Measured on an MI355X, worst err / bar: fp64 stream path 0.38 at (70, 5), k = 64 (0.03 and less from L = 65 on), shard pair 0.10, per tick 0.05;
fp32 stream path 0.87 .. 1.00 (one correct rounding reaches its bound), fp32 shard pair 0.24."""
import ctypes as C
import functools

import numpy as np
import pytest

EPS = 2.0 ** -52
U32 = 2.0 ** -24
KAPPA_CAP = 1e7
ROUTE_NORMAL, ROUTE_WOODBURY = 3.2, 24.7               # measured, see above
C_BAR = 4 * max(ROUTE_NORMAL, ROUTE_WOODBURY)
KAPPA_WORST = 4.8e6
SEED = 2
SHAPES = [(8, 4), (70, 5), (130, 65), (200, 100), (321, 257), (2100, 2000)]
BIG = (2100, 2000)                                     # > 48 KB of LDS (L > 1984): mixing from a numpy QR factor through moihgp_set_mixing
KS = (1, 2, 63, 64)
PATTERNS = ("head", "tail", "ends", "rand")
T_STREAM = 40
LIMIT_SHAPES = [(200, 100), (130, 65), (128, 65)]      # (128, 65): M - L = 63, the only way to k = 64 with M - k = L - 1
TICK_L = [4, 65, 255, 256, 257]                        # per-tick ABI, M = L + 70
TICK_K = (1, 64, 65, 70)
SHARD_CASES = [(130, 65, (1, 64)), (130, 65, (21, 44)), (200, 100, (1, 99)), (200, 100, (33, 67)), (200, 100, (20, 47, 33))]
LSTSQ_MAX_L = 512
SENT = 12345.0


def ks_of(M, L):
    """k in {1, 2, 63, 64} capped at M - L, and k = M - L itself (past 64 only the per-tick path solves it: the stream path must refuse)."""
    return sorted({min(k, M - L) for k in KS} | {M - L})


def case_table():
    cases = [(M, L, k, p) for M, L in SHAPES for k in ks_of(M, L) for p in PATTERNS]
    cases += [(128, 65, k, p) for k in (1, 2, 63) for p in PATTERNS]
    cases += [(L + 70, L, k, p) for L in TICK_L for k in TICK_K for p in PATTERNS]
    return cases


CASES = case_table()


def rows_of(M, k, pattern, rng):
    if pattern == "head":
        return np.arange(k)
    if pattern == "tail":
        return np.arange(M - k, M)
    if pattern == "ends":
        return np.concatenate([np.arange((k + 1) // 2), np.arange(M - k // 2, M)])
    return np.sort(rng.choice(M, size=k, replace=False))


def case_vector(M, L, k, pattern):
    """(missing rows ascending, y [M] with NaN at them): one observation vector per (shape, k, pattern), wherever in a stream it is put."""
    rng = np.random.default_rng([SEED, M, L, k, PATTERNS.index(pattern)])
    miss = rows_of(M, k, pattern, rng)
    y = rng.standard_normal(M)
    y[miss] = np.nan
    return miss, y


@functools.lru_cache(maxsize=None)
def raw_params(M, L):
    """What update() is handed: eye(M, L) + 0.2 randn (its polar factor becomes U), S, sigma, the per-latent triples."""
    rng = np.random.default_rng([SEED, M, L])
    A = np.eye(M, L) + 0.2 * rng.standard_normal((M, L))
    S = rng.uniform(0.5, 2.0, L)
    igp = np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])
    return A, S, 0.04, igp


class Mix:
    """An orthonormal U [M, L] with S [L], and U in longdouble when the refinement first asks for it."""

    def __init__(self, U, S, tag):
        self.U, self.S, self.tag = np.ascontiguousarray(U), np.ascontiguousarray(S), tag
        self._Ul = None
        self._truth = {}

    @property
    def Ul(self):
        if self._Ul is None:
            self._Ul = self.U.astype(np.longdouble)
        return self._Ul


@functools.lru_cache(maxsize=None)
def mixing_np(M, L):
    """The CPU twin of the handle's mixing: the polar factor by SVD (the QR factor at BIG)."""
    A, S, _, _ = raw_params(M, L)
    if (M, L) == BIG:
        return Mix(np.linalg.qr(A)[0], S, "np")
    W, _, Vt = np.linalg.svd(A, full_matrices=False)
    return Mix(W @ Vt, S, "np")


# ------------------------------------------------------------------------------------------------ truth and scale (numpy)
def kappa_of(U, miss):
    """(sigma_max / sigma_min)^2 of U[obs] through the k missing rows: U^T U = I, so the eigenvalues of U0^T U0 = I - Um^T Um are 1 - s_i^2
    for the singular values s_i of Um and 1 otherwise."""
    s = np.linalg.svd(U[miss], compute_uv=False)
    ev = np.ones(U.shape[1])
    ev[:len(s)] = (1.0 - s) * (1.0 + s)
    return float(ev.max() / ev.min())


def kappa_direct(U, miss):
    obs = np.ones(U.shape[0], dtype=bool); obs[miss] = False
    s = np.linalg.svd(U[obs], compute_uv=False)
    return float((s[0] / s[-1]) ** 2)


def residual_ld(mix, a, y, miss):
    """U0^T (y0 - U0 a) in longdouble, without copying the observed rows: the missing rows of the residual are zeroed."""
    z = np.where(np.isnan(y), 0.0, y).astype(np.longdouble) - mix.Ul @ a
    z[miss] = 0.0
    return mix.Ul.T @ z


def woodbury_np(U, y, miss):
    """The header comment of tick.hip in numpy: a = r + Um^T (I_k - Um Um^T)^-1 Um r, r = U^T (y, NaN -> 0)."""
    r = U.T @ np.where(np.isnan(y), 0.0, y)
    Um = U[miss]
    return r + Um.T @ np.linalg.solve(np.eye(len(miss)) - Um @ Um.T, Um @ r)


def normal_np(U, y, miss):
    """The reference's route (moihgp.h:167-177): solve(U0^T U0, U0^T y0)."""
    obs = np.ones(U.shape[0], dtype=bool); obs[miss] = False
    U0 = U[obs]
    return np.linalg.solve(U0.T @ U0, U0.T @ y[obs])


def truth_a(mix, y, miss, steps=3):
    """a* in longdouble: lstsq, then `steps` refinements with the longdouble residual."""
    U = mix.U
    M, L = U.shape
    if L <= LSTSQ_MAX_L:
        obs = np.ones(M, dtype=bool); obs[miss] = False
        U0 = U[obs]
        a = np.linalg.lstsq(U0, y[obs], rcond=None)[0]
        N = U0.T @ U0
        corr = lambda g: np.linalg.solve(N, g)
    else:
        Um = U[miss]
        W = np.eye(len(miss)) - Um @ Um.T
        corr = lambda g: g + Um.T @ np.linalg.solve(W, Um @ g)
        a = corr(U.T @ np.where(np.isnan(y), 0.0, y))
    a = a.astype(np.longdouble)
    for _ in range(steps):
        a = a + corr(residual_ld(mix, a, y, miss).astype(np.float64))
    return a


def truth_Ty(mix, y, miss, key=None):
    """(Ty* [L] fp64, kappa), kept per mixing under `key`."""
    if key is not None and key in mix._truth:
        return mix._truth[key]
    out = ((truth_a(mix, y, miss) / np.sqrt(mix.S.astype(np.longdouble))).astype(np.float64), kappa_of(mix.U, miss))
    if key is not None:
        mix._truth[key] = out
    return out


def bars(Ty, kap, dtype, extra=0.0):
    b = C_BAR * EPS * kap * np.max(np.abs(Ty)) + extra
    return b + U32 * np.abs(Ty) if dtype == "f32" else b + 0.0 * Ty


def rounded(y, dtype):
    return y.astype(np.float32).astype(np.float64) if dtype == "f32" else y


# ------------------------------------------------------------------------------------------------ CPU
def test_case_table_holds_what_it_should():
    assert ks_of(8, 4) == [1, 2, 4] and ks_of(321, 257) == [1, 2, 63, 64] and ks_of(2100, 2000) == [1, 2, 63, 64, 100]
    for M, L, k, p in CASES:
        miss, y = case_vector(M, L, k, p)
        assert len(miss) == k == len(set(miss.tolist())) and M - k >= L and np.isnan(y).sum() == k and (np.diff(miss) > 0).all()
    assert (rows_of(10, 5, "ends", None) == [0, 1, 2, 8, 9]).all()


def test_cases_are_well_posed():
    """Every case of the table, with the seeds of this file: kappa <= 1e7 (so that the bars mean something), the two ways to kappa agree, and the
    mixing is orthonormal to rounding."""
    worst = (0.0, None)
    for M, L, k, p in CASES:
        mix = mixing_np(M, L)
        miss, _ = case_vector(M, L, k, p)
        kap = kappa_of(mix.U, miss)
        if L <= LSTSQ_MAX_L:
            assert abs(kap - kappa_direct(mix.U, miss)) <= 1e-6 * kap, (M, L, k, p)
        worst = max(worst, (kap, (M, L, k, p)))
        assert kap <= KAPPA_CAP, (M, L, k, p, kap)
    print(f"worst kappa {worst[0]:.3e} at {worst[1]}")
    assert KAPPA_WORST / 2 <= worst[0] <= 2 * KAPPA_WORST
    for M, L in {(M, L) for M, L, _, _ in CASES}:
        U = mixing_np(M, L).U
        assert np.max(np.abs(U.T @ U - np.eye(L))) < 1e-13


def cholesky_ld(mix, y, miss):
    """solve(U0^T U0, U0^T y0) by Cholesky, every operation in longdouble."""
    M, L = mix.U.shape
    obs = np.ones(M, dtype=bool); obs[miss] = False
    U0, y0 = mix.Ul[obs], y[obs].astype(np.longdouble)
    N, b = U0.T @ U0, U0.T @ y0
    R = np.zeros((L, L), dtype=np.longdouble)              # N = R^T R
    for i in range(L):
        R[i, i] = np.sqrt(N[i, i] - R[:i, i] @ R[:i, i])
        for j in range(i + 1, L):
            R[i, j] = (N[i, j] - R[:i, i] @ R[:i, j]) / R[i, i]
    z = np.zeros(L, dtype=np.longdouble)
    for i in range(L):
        z[i] = (b[i] - R[:i, i] @ z[:i]) / R[i, i]
    a = np.zeros(L, dtype=np.longdouble)
    for i in range(L - 1, -1, -1):
        a[i] = (z[i] - R[i, i + 1:] @ a[i + 1:]) / R[i, i]
    return a


def test_refinement_converged_at_the_smallest_shape():
    """The refined truth against a longdouble Cholesky of the normal equations, to 2^-60 relative.  That Cholesky is itself good to kappa 2^-64
    only, so it can vouch for 2^-60 where kappa <= 16: k = 1 and most of k = 2 at the smallest shape.  The others (the square systems k = M - L = 4
    above all, kappa up to some hundreds) are held to 4 kappa 2^-64, which is all that this witness can see."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than double here"
    M, L = SHAPES[0]
    mix = mixing_np(M, L)
    sharp = 0
    for k in ks_of(M, L):
        for p in PATTERNS:
            miss, y = case_vector(M, L, k, p)
            a, kap = cholesky_ld(mix, y, miss), kappa_of(mix.U, miss)
            rel = float(np.max(np.abs(truth_a(mix, y, miss) - a)) / np.max(np.abs(a)))
            print(f"k = {k} {p}: kappa {kap:.1f}, truth against longdouble Cholesky {rel:.2e}")
            if kap <= 16:
                sharp += 1
                assert rel <= 2.0 ** -60, (k, p, rel)
            else:
                assert rel <= 4 * kap * 2.0 ** -64, (k, p, rel)
    assert sharp >= 4


def test_refinement_converged_at_the_largest_shape():
    """Where the start vector is not lstsq's.  The error of a is at most kappa |g|_2 with g the residual U0^T (y0 - U0 a) that is left, and one
    unit of the bar is 2^-52 kappa max |a*|: what is left of g (the rounding of its own longdouble sums) is below an eighth of such a unit."""
    M, L = BIG
    mix = mixing_np(M, L)
    for k, p in [(64, "head"), (100, "ends"), (63, "rand")]:
        miss, y = case_vector(M, L, k, p)
        a = truth_a(mix, y, miss)
        g = residual_ld(mix, a, y, miss)
        left = float(np.sqrt(g @ g) / np.max(np.abs(a))) / EPS
        print(f"k = {k} {p}: |g|_2 / (2^-52 max |a*|) = {left:.3f}")
        assert left <= 0.125, (k, p, left)


STREAM_SHAPES = set(SHAPES) | {(128, 65)}


def route_constants():
    """Worst err / (2^-52 kappa max |a*|) of the two routes in numpy fp64, with the case: "normal" over every case with L <= 257, "woodbury" over
    the stream path's shapes, "woodbury_per_tick" over the per-tick cases (not part of the rule, see the head of this file)."""
    worst = {"normal": (0.0, None), "woodbury": (0.0, None), "woodbury_per_tick": (0.0, None)}
    for M, L, k, p in CASES:
        mix = mixing_np(M, L)
        miss, y = case_vector(M, L, k, p)
        a = truth_a(mix, y, miss).astype(np.float64)
        scale = EPS * kappa_of(mix.U, miss) * np.max(np.abs(a))
        routes = [("woodbury" if (M, L) in STREAM_SHAPES else "woodbury_per_tick", woodbury_np)] + ([("normal", normal_np)] if L <= 257 else [])
        for name, route in routes:
            worst[name] = max(worst[name], (float(np.max(np.abs(route(mix.U, y, miss) - a)) / scale), (M, L, k, p)))
    return worst


def test_route_constants_and_the_bar():
    """C_BAR follows its rule: four times the larger of the two routes' worst err / (2^-52 kappa max |a*|) -- to a factor two, on whatever BLAS
    this runs; and the recorded figures are what they are here, to the same factor."""
    worst = route_constants()
    print("routes: " + ", ".join(f"{name} {v:.2f} at {case}" for name, (v, case) in worst.items()) + f"; C_BAR {C_BAR}")
    rule = 4 * max(worst["normal"][0], worst["woodbury"][0])
    assert rule / 2 <= C_BAR <= 2 * rule, (worst, C_BAR)
    assert ROUTE_NORMAL / 2 <= worst["normal"][0] <= 2 * ROUTE_NORMAL and ROUTE_WOODBURY / 2 <= worst["woodbury"][0] <= 2 * ROUTE_WOODBURY


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import MOIHGP, streams
    from multioutputihgp_amd._lib import c_double_p, last_error, load_library
    return dict(torch=torch, streams=streams, MOIHGP=MOIHGP, lib=load_library(), c_double_p=c_double_p, last_error=last_error, models={})


def set_mixing(env, gp, U, S, sigma=0.04):
    U, S = np.ascontiguousarray(U), np.ascontiguousarray(S)
    rc = env["lib"].moihgp_set_mixing(gp.handle, U.ctypes.data_as(env["c_double_p"]), S.ctypes.data_as(env["c_double_p"]), C.c_double(sigma))
    assert rc == 0, env["last_error"](env["lib"])


def model(env, M, L):
    """(handle, its mixing read back): update() and its polar factor, moihgp_set_mixing from the QR factor at BIG; one per shape and session."""
    if (M, L) not in env["models"]:
        gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
        A, S, sigma, igp = raw_params(M, L)
        if (M, L) == BIG:
            set_mixing(env, gp, mixing_np(M, L).U, S, sigma)
        else:
            gp.update(np.concatenate([A.ravel(), S, [sigma], igp.ravel()]))
        p = gp.params.copy()
        mix = Mix(p[:M * L].reshape(M, L), p[M * L:M * L + L], "dev")
        assert np.max(np.abs(mix.U.T @ mix.U - np.eye(L))) < 1e-12
        env["models"][(M, L)] = (gp, mix)
    return env["models"][(M, L)]


def tdt_of(env, dtype):
    return env["torch"].float64 if dtype == "f64" else env["torch"].float32


def project(env, gp, Yd, layout):
    """The stream projection into a buffer full of sentinels: (Ty [L, T] as fp64 numpy, whether everything outside the T ticks kept the sentinel).
    series: rows of ld = T + 8 > T;  tiled: a whole sentinel tile behind the stream, and the ticks >= T of the last tile."""
    torch, streams, lib = env["torch"], env["streams"], env["lib"]
    T, L = Yd.shape[0], gp.num_latent
    if layout == "series":
        ld = T + 8
        buf = torch.full((L, ld), SENT, dtype=Yd.dtype, device="cuda")
        rc = lib.moihgp_project_stream(gp.handle, 0 if Yd.dtype == torch.float64 else 1, C.c_void_p(Yd.data_ptr()), T, C.c_void_p(buf.data_ptr()), ld,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, env["last_error"](lib)
        torch.cuda.synchronize()
        return buf[:, :T].double().cpu().numpy(), bool((buf[:, T:] == SENT).all())
    seg = streams.seg_ticks(Yd.dtype)
    nseg = (T + seg - 1) // seg
    slab = torch.full((nseg + 1, L, seg), SENT, dtype=Yd.dtype, device="cuda")
    out = streams.project_stream_tiled(gp, Yd, out=slab[:nseg])
    torch.cuda.synchronize()
    assert out.data_ptr() == slab.data_ptr()
    got = slab[:nseg].permute(1, 0, 2).reshape(L, nseg * seg)
    return got[:, :T].double().cpu().numpy(), bool((got[:, T:] == SENT).all()) and bool((slab[nseg] == SENT).all())


def stream_of(M, L, T, slots, plan, dtype):
    """Y [T, M] fp64 (already rounded to the stream type) with the vectors of `plan` = [(k, pattern)] at the ticks `slots`, every other tick fully
    observed."""
    rng = np.random.default_rng([SEED, M, L, T])
    Y = rng.standard_normal((T, M))
    for t, (k, p) in zip(slots, plan):
        Y[t] = case_vector(M, L, k, p)[1]
    return rounded(Y, dtype)


def check_columns(env, gp, mix, Y, slots, plan, got, dtype, what):
    """Every affected column: solved at the bars where k <= 64 and M - k >= L, an all-NaN column otherwise.  Prints the worst err / bar."""
    M, L = mix.U.shape
    worst = (0.0, None)
    for t, (k, p) in zip(slots, plan):
        if k > 64 or M - k < L:
            assert np.isnan(got[:, t]).all(), (what, t, k, p, "not refused")
            continue
        miss = np.nonzero(np.isnan(Y[t]))[0]
        assert len(miss) == k
        Ty, kap = truth_Ty(mix, Y[t], miss, key=(k, p, dtype))
        assert kap <= KAPPA_CAP
        err, bar = np.abs(got[:, t] - Ty), bars(Ty, kap, dtype)
        assert np.isfinite(got[:, t]).all(), (what, t, k, p)
        worst = max(worst, (float(np.max(err / bar)), (t, k, p, f"kappa {kap:.2e}")))
        assert (err <= bar).all(), (what, t, k, p, f"kappa {kap:.2e}", float(np.max(err / bar)), float(np.max(err) / np.max(np.abs(Ty))))
    print(f"{what}: worst err / bar {worst[0]:.3f} at {worst[1]}")
    return worst[0]


def plan_of(M, L):
    return [(k, p) for k in ks_of(M, L) for p in PATTERNS]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_stream_path_series_major(env, M, L, dtype):
    """Every (k, pattern) of the shape in one stream of 40 ticks, t = 0, 1, T - 2 and T - 1 among them: the affected columns at the bars, the
    fully observed ones bit for bit what they are when the affected ticks hold finite values instead, the rows' padding untouched."""
    torch = env["torch"]
    gp, mix = model(env, M, L)
    T, plan = T_STREAM, plan_of(M, L)
    slots = ([0, 1, T - 1, T - 2] + list(range(3, T - 3, 2)))[:len(plan)]
    Y = stream_of(M, L, T, slots, plan, dtype)
    got, pad_ok = project(env, gp, torch.from_numpy(Y).to(tdt_of(env, dtype)).cuda(), "series")
    assert pad_ok
    check_columns(env, gp, mix, Y, slots, plan, got, dtype, f"series {M}x{L} {dtype}")
    filled = Y.copy()
    filled[slots] = np.where(np.isnan(Y[slots]), 0.5, Y[slots])
    ref, _ = project(env, gp, torch.from_numpy(filled).to(tdt_of(env, dtype)).cuda(), "series")
    rest = np.setdiff1d(np.arange(T), slots)
    assert np.isfinite(got[:, rest]).all() and np.array_equal(got[:, rest], ref[:, rest])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_stream_path_tiled(env, M, L, dtype):
    """The same vectors against the same truth (not against the series-major result) in the segment-major layout, T = SEG + 40: affected ticks at
    SEG - 1, SEG and T - 1, i.e. on both sides of the tile edge and at the end of the ragged tile; a sentinel tile behind the stream and sentinels
    in the ticks >= T of the last tile."""
    torch = env["torch"]
    gp, mix = model(env, M, L)
    seg = env["streams"].seg_ticks(tdt_of(env, dtype))
    T, plan = seg + 40, plan_of(M, L)
    slots = ([seg - 1, seg, T - 1] + list(range(seg + 2, T - 2, 2)))[:len(plan)]
    Y = stream_of(M, L, T, slots, plan, dtype)
    got, pad_ok = project(env, gp, torch.from_numpy(Y).to(tdt_of(env, dtype)).cuda(), "tiled")
    assert pad_ok
    check_columns(env, gp, mix, Y, slots, plan, got, dtype, f"tiled {M}x{L} {dtype}")
    rest = np.setdiff1d(np.arange(T), slots)
    assert np.isfinite(got[:, rest]).all()


def limit_plan(M, L):
    """Around both limits: k = 65 (first past the wavefront), 64, M - L + 1 (first past the rank), M - L, two ticks with 83 and 100 NaNs
    (65 .. 100: miss[] and the LDS system would be overrun) between solvable neighbours."""
    d = M - L
    return [(65, "head"), (64, "ends"), (d + 1, "tail"), (d, "rand"), (2, "rand"), (83, "rand"), (min(d, 64), "head"), (100, "rand"), (1, "head"), (1, "tail")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["series", "tiled"])
@pytest.mark.parametrize("M,L", LIMIT_SHAPES)
def test_limits_of_the_stream_path(env, M, L, layout, dtype):
    """Refused (an all-NaN column, a missing tick to the later kernels): k = 65, k = 64 with M - k = L - 1 (at (128, 65)), k = M - L + 1.  Solved at
    the bars: k = 64 and k = M - L where the other limit allows it.  With 65 .. 100 NaNs in a tick the neighbouring affected ticks are still right."""
    torch = env["torch"]
    gp, mix = model(env, M, L)
    T, plan = T_STREAM, limit_plan(M, L)
    slots = list(range(len(plan) - 1)) + [T - 1]
    Y = stream_of(M, L, T, slots, plan, dtype)
    solved = [(k, p) for k, p in plan if k <= 64 and M - k >= L]
    assert len(solved) >= 5 and len(solved) <= len(plan) - 4
    if (M, L) == (128, 65):
        assert (64, "ends") not in solved and (63, "rand") in solved
    got, pad_ok = project(env, gp, torch.from_numpy(Y).to(tdt_of(env, dtype)).cuda(), layout)
    assert pad_ok
    check_columns(env, gp, mix, Y, slots, plan, got, dtype, f"limits {layout} {M}x{L} {dtype}")
    rest = np.setdiff1d(np.arange(T), slots)
    assert np.isfinite(got[:, rest]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M,L,widths", SHARD_CASES)
def test_shard_pair_in_one_process(env, M, L, widths, dtype):
    """moihgp_ls_shard_gram / _apply on their own: the columns of one orthonormal U split into shards of unequal width (one of them a single
    latent), one handle per shard, the packed records summed with torch in place of the all-reduce.  kmax = 64 with ticks of k = 1, 2, 63 and 64
    in the same call (padding, k < kmax records); the tick list unsorted, t = 0 and T - 1 in it.  fp32: Ty is the correctly rounded fp32 image
    of the fp64 projection, so that the bar's input term is all that enters."""
    torch, streams, lib = env["torch"], env["streams"], env["lib"]
    assert sum(widths) == L
    mix = mixing_np(M, L)
    T, kmax = T_STREAM, 64
    plan = [(k, p) for k in KS for p in PATTERNS]
    slots = ([0, T - 1] + list(range(2, T - 2, 2)))[:len(plan)]
    Y = stream_of(M, L, T, slots, plan, dtype)
    tdt = tdt_of(env, dtype)
    Yd = torch.from_numpy(Y).to(tdt).cuda()
    Y0 = torch.from_numpy(np.where(np.isnan(Y), 0.0, Y)).cuda()
    order = np.random.default_rng(SEED).permutation(len(slots))
    ticks = torch.tensor([slots[i] for i in order], dtype=torch.int32, device="cuda")
    n, rec = len(slots), kmax + kmax * kmax
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = 0 if dtype == "f64" else 1
    shards, lo = [], 0
    for w in widths:
        gp = env["MOIHGP"](0.1, M, w, kernel="Matern32")
        set_mixing(env, gp, mix.U[:, lo:lo + w], mix.S[lo:lo + w])
        Ty = streams.project_stream(gp, Y0)[:, :T].to(tdt).contiguous()
        packed = torch.full((n, rec), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.moihgp_ls_shard_gram(gp.handle, dt, C.c_void_p(Yd.data_ptr()), C.c_void_p(ticks.data_ptr()), n, kmax, C.c_void_p(Ty.data_ptr()), Ty.stride(0),
                                      C.c_void_p(packed.data_ptr()), stream)
        assert rc == 0, env["last_error"](lib)
        shards.append((gp, Ty, packed))
        lo += w
    torch.cuda.synchronize()
    total = torch.stack([s[2] for s in shards]).sum(dim=0)
    assert bool(torch.isfinite(total).all())
    before = torch.cat([s[1] for s in shards]).double().cpu().numpy()
    for gp, Ty, _ in shards:
        rc = lib.moihgp_ls_shard_apply(gp.handle, dt, C.c_void_p(Yd.data_ptr()), C.c_void_p(ticks.data_ptr()), n, kmax, C.c_void_p(total.data_ptr()),
                                       C.c_void_p(Ty.data_ptr()), Ty.stride(0), stream)
        assert rc == 0, env["last_error"](lib)
    torch.cuda.synchronize()
    got = torch.cat([s[1] for s in shards]).double().cpu().numpy()
    rest = np.setdiff1d(np.arange(T), slots)
    assert np.array_equal(got[:, rest], before[:, rest])
    worst = (0.0, None)
    for t, (k, p) in zip(slots, plan):
        miss = np.nonzero(np.isnan(Y[t]))[0]
        Ty, kap = truth_Ty(mix, Y[t], miss, key=(k, p, dtype))
        extra = 0.0
        if dtype == "f32":
            r = mix.U.T @ np.where(np.isnan(Y[t]), 0.0, Y[t])
            extra = U32 * kap * np.linalg.norm(r) / np.sqrt(mix.S)
        err, bar = np.abs(got[:, t] - Ty), bars(Ty, kap, dtype, extra)
        worst = max(worst, (float(np.max(err / bar)), (t, k, p, f"kappa {kap:.2e}")))
        assert (err <= bar).all(), (t, k, p, f"kappa {kap:.2e}", float(np.max(err / bar)))
    print(f"shards {M}x{L} {widths} {dtype}: worst err / bar {worst[0]:.3f} at {worst[1]}")
    # argument errors: kmax outside 1 .. 64
    gp, Ty, packed = shards[0]
    for bad in (0, 65):
        for entry in (lib.moihgp_ls_shard_gram, lib.moihgp_ls_shard_apply):
            args = (C.c_void_p(Ty.data_ptr()), Ty.stride(0), C.c_void_p(packed.data_ptr())) if entry is lib.moihgp_ls_shard_gram else \
                   (C.c_void_p(packed.data_ptr()), C.c_void_p(Ty.data_ptr()), Ty.stride(0))
            assert entry(gp.handle, dt, C.c_void_p(Yd.data_ptr()), C.c_void_p(ticks.data_ptr()), n, bad, *args, stream) == 1
            assert "kmax" in env["last_error"](lib)
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat([s[1] for s in shards]).double().cpu().numpy(), got)


def gains_of(env, gp):
    """K [L, d] of every latent (moihgp_get_latent)."""
    L, d = gp.num_latent, gp.igp_dim
    K = np.zeros((L, d))
    row = np.zeros(d)
    for l in range(L):
        assert env["lib"].moihgp_get_latent(gp.handle, l, None, row.ctypes.data_as(env["c_double_p"]), None, None, None, None, None, None, None, None, None) == 0
        K[l] = row
    return K


@pytest.mark.gpu
@pytest.mark.parametrize("L", TICK_L)
def test_per_tick_path(env, L):
    """gp.step(x = 0, y): the new state is K_l Ty_l, held to K_l Ty*_l at the fp64 bar (the route is the normal equations: the same scale).
    L on both sides of the solve's workgroup width; k = 65 and k = M - L = 70, which only this path accepts."""
    M = L + 70
    gp, mix = model(env, M, L)
    K = gains_of(env, gp)
    x0 = np.zeros((L, gp.igp_dim))
    worst = (0.0, None)
    for k in TICK_K:
        for p in PATTERNS:
            miss, y = case_vector(M, L, k, p)
            xnew, _ = gp.step(x0, y)
            Ty, kap = truth_Ty(mix, y, miss, key=(k, p, "f64"))
            assert kap <= KAPPA_CAP
            err, bar = np.abs(xnew - K * Ty[:, None]), np.abs(K) * bars(Ty, kap, "f64")[:, None]
            assert np.isfinite(xnew).all(), (k, p)
            worst = max(worst, (float(np.max(err / bar)), (k, p, f"kappa {kap:.2e}")))
            assert (err <= bar).all(), (k, p, f"kappa {kap:.2e}", float(np.max(err / bar)))
    print(f"per tick {M}x{L}: worst err / bar {worst[0]:.3f} at {worst[1]}")


@pytest.mark.gpu
@pytest.mark.parametrize("L", TICK_L)
def test_per_tick_path_with_fewer_observed_outputs_than_latents(env, L):
    """k = M - L + 1: L - 1 observed rows, the normal equations are singular (the reference factors a singular matrix there, moihgp.h:177).  Pinned
    as it is today: the per-tick ABI does not refuse the tick as the stream path does -- the elimination meets a pivot that is rounding noise,
    not zero, and the call returns a finite vector, the same bit for bit when repeated; the handle is none the worse for it.  The vector is one
    solution of the consistent system plus an arbitrary multiple of the null vector (entries of some hundreds for data of size one): callers
    with such ticks should treat them as missing."""
    M = L + 70
    gp, mix = model(env, M, L)
    K = gains_of(env, gp)
    x0 = np.zeros((L, gp.igp_dim))
    full = np.random.default_rng([SEED, L]).standard_normal(M)
    before = gp.step(x0, full)
    for p in PATTERNS:
        miss, y = case_vector(M, L, M - L + 1, p)
        x1, y1 = gp.step(x0, y)
        x2, y2 = gp.step(x0, y)
        assert np.isfinite(x1).all() and np.isfinite(y1).all(), p
        assert np.array_equal(x1, x2) and np.array_equal(y1, y2), p
        obs = ~np.isnan(y)
        a = np.sqrt(mix.S) * x1[:, 0] / K[:, 0]
        print(f"per tick {M}x{L} k = {M - L + 1} {p}: max |a| {np.max(np.abs(a)):.3e}, observed rows reproduced to {np.max(np.abs(mix.U[obs] @ a - y[obs])):.2e}")
    after = gp.step(x0, full)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
