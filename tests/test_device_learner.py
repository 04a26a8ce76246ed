"""The device-resident learner below the objective: the vector kernels (csrc/vecops.hip, `moihgp_dvec_*`) at the edges of their grids, and
the solver and BFGS matrix on them (include/moihgp_cxx/lbfgsb_dev.hpp) against the host solver and a long-double recursion.

CPU: tests/cxx/lbfgsb_dev_test.cpp linked with the plain-C++ stand-in tests/cxx/dvec_cpu.cpp runs the device solver's host logic under four
summation orders of the reductions.  What those orders do to the iterates is the measure of what rounding order alone may do; ten times
that is the bar for the real kernels.
GPU: the same program linked with the library, and the kernels themselves through ctypes.

Roundings on a term's way through a device sum (vecops.hip; adding to the 0.0 an accumulator starts from is exact):
    thread's fma chain            ceil(n / 262144)
    block_sum                     6 (butterfly over 64 lanes) + 3 (four wavefront sums)
    finish_kernel                 3 (four partials per thread) + 6 + 3
so SUM_ROUNDINGS(n) = ceil(n / 262144) + 21, and a sum is within gamma(SUM_ROUNDINGS + 2) * sum |term| of the exact one: 1 for the one
rounding of a term that is not a bare product (`gradp (xt - xp)`), 1 for the long-double reference's own roundings (2^-64 per term and
per pairwise level: under u for every n here)."""
import ctypes as C
import functools
import math
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from cxx_support import _cxx, _lines
from parity_support import env  # noqa: F401  (env: fixture)

U = 2.0 ** -53
K = 1024 * 256                       # kRedBlocks * kRedThreads: where a reduction thread takes its second term
SIZES = [0, 63, 64, 65, 255, 256, 257, K - 1, K, K + 1, 1 << 20, (1 << 20) + 1, (1 << 21) + 77]
ld = np.longdouble


def sum_roundings(n):
    return -(-n // K) + 21


def sum_bar(n, abs_terms):
    k = sum_roundings(n) + 2
    return k * U / (1 - k * U) * float(abs_terms)


def special(n):
    """Indices where a reduction changes hands: first and last lane of a workgroup, last thread of the grid, its first second term, the end."""
    return sorted({i for i in (0, 255, 256, K - 1, K, n - 1) if 0 <= i < n})


# ================================================================================================ solver and BFGS matrix
PROBLEMS = {"a": (0, 10, 0), "b40": (1, 40, 0), "b300000": (1, 300000, 8), "c": (2, 1100000, 0)}     # prob, n, max_iterations
ORDERS = {0: "sequential", 1: "long double", 2: "reversed", 3: "device order"}
SPREAD_CAP = 1e-10
CXX_FLAGS = ["-pthread", "-ffp-contract=off"]


def _cpu_exe():
    return _cxx("lbfgsb_dev_test", None, extra=[os.path.join(ROOT, "tests", "cxx", "dvec_cpu.cpp")] + CXX_FLAGS, out="lbfgsb_dev_test_cpu")


def _solve(exe, name, order):
    prob, n, maxit = PROBLEMS[name]
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "x.bin")
        out = _lines(exe, f"solve {prob} {n} {maxit} {order} {dump}\n")
        x = np.fromfile(dump).reshape(2, n)
    h, d, p = out[0].split(), out[1].split(), out[2].split()
    assert h[0] == "host" and d[0] == "dev" and p[0] == "points"
    r = dict(host_it=int(h[1]), host_ev=int(h[2]), host_fx=float(h[3]), dev_it=int(d[1]), dev_ev=int(d[2]), dev_fx=float(d[3]),
             compared=int(p[1]), worst=float(p[2]), unmatched=int(p[3]), backend=out[3], n=n)
    if name == "c":                                                  # (8.8 MB per iterate: keep the figures, not the vectors)
        i = np.arange(n)
        t, c, lb, ub = 1.5 * np.sin(0.37 * (i % 1013)), 1.0 + i % 97, -0.7, 0.9
        inside = (t > lb) & (t < ub)
        xd = x[1]
        r.update(free_worst=float(np.max(np.abs(xd - t)[inside] * c[inside])), bound_share=float(1 - inside.mean()),
                 off_bound=int((xd[t >= ub] != ub).sum() + (xd[t <= lb] != lb).sum()))
    else:
        r.update(x=x[1] if n <= 64 else None)
    return r


@functools.lru_cache(maxsize=None)
def _cpu_runs(name):
    exe = _cpu_exe()
    with ThreadPoolExecutor(len(ORDERS)) as pool:
        return dict(zip(ORDERS, pool.map(lambda o: _solve(exe, name, o), ORDERS)))


def _cpu_spread(name):
    """Largest difference of an evaluation point between the host solver and the stand-in, over all summation orders."""
    return max(r["worst"] for r in _cpu_runs(name).values())


def _scipy_fun(name):
    from scipy.optimize import minimize
    prob, n, _ = PROBLEMS[name]
    if prob == 0:
        def f(x):
            a, b = x[1:] - x[:-1] ** 2, 1 - x[:-1]
            g = np.zeros_like(x); g[:-1] += -400 * a * x[:-1] - 2 * b; g[1:] += 200 * a
            return float(np.sum(100 * a ** 2 + b ** 2)), g
        lb, ub = -2 * np.ones(n), np.r_[0.5, 2 * np.ones(n - 1)]
    else:
        def f(x):
            ax = 2.5 * x.copy(); ax[1:] -= x[:-1]; ax[:-1] -= x[1:]; b = 3 * np.sin(np.arange(1, n + 1))
            return float(0.5 * x @ ax - b @ x), ax - b
        lb, ub = -0.7 * np.ones(n), 0.9 * np.ones(n)
    r = minimize(f, np.zeros(n), jac=True, method="L-BFGS-B", bounds=list(zip(lb, ub)), options=dict(ftol=1e-15, gtol=1e-10, maxiter=5000))
    return r.fun, lb, ub


def _check_solve(name, r, bar, what):
    print(f"{name} [{what}]: iterations {r['dev_it']} (host {r['host_it']}), evaluations {r['dev_ev']} (host {r['host_ev']}), "
          f"worst evaluation-point difference {r['worst']:.3g}, bar {bar:.3g}, ratio {r['worst'] / bar:.3g}")
    assert r["dev_it"] == r["host_it"] and r["dev_ev"] == r["host_ev"], (name, what)
    assert r["unmatched"] == 0 and r["compared"] == r["dev_ev"], (name, what)         # every evaluation point is in the comparison
    assert r["worst"] <= bar, (name, what, r["worst"], bar)
    if name in ("a", "b40"):
        fun, lb, ub = _scipy_fun(name)
        assert abs(r["dev_fx"] - fun) < 1e-9 * max(1.0, abs(fun)), (name, what)
        assert np.all(r["x"] >= lb) and np.all(r["x"] <= ub)
        if name == "b40":
            assert ((r["x"] <= lb) | (r["x"] >= ub)).sum() == 25
    if name == "c":                                                  # the minimiser is clip(t, lb, ub): c_i |x_i - t_i| <= epsilon on the free ones
        assert r["free_worst"] <= 1e-10 and r["off_bound"] == 0 and 0.63 < r["bound_share"] < 0.65, (name, what, r)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_device_solver_logic_follows_the_host_solver_under_every_summation_order(name):
    """DevLBFGSBSolver on the CPU stand-in: same iteration and evaluation counts as the host solver under each order, every evaluation point
    within the spread cap, the minimum SciPy's (a, b at n = 40) or the known one (c).  Measured here (worst evaluation-point difference
    per order sequential / long double / reversed / device): a 6.7e-16 / 2.1e-15 / 1.5e-15 / 7.4e-15, b40 6.1e-16 / 6.7e-16 / 6.7e-16 /
    6.7e-16, b300000 (8 iterations) <= 1.3e-13, c 2.7e-14 .. 2.5e-12."""
    runs = _cpu_runs(name)
    spread = _cpu_spread(name)
    print(f"{name}: spread over orders {spread:.3g}")
    assert 0 < spread <= SPREAD_CAP
    for order, r in runs.items():
        assert r["backend"] == "cpu"
        _check_solve(name, r, SPREAD_CAP, ORDERS[order])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_device_solver_follows_the_host_solver(hip_built, name):
    """The same with the real kernels; the bar for the evaluation points is 10 x what the summation orders differ by on the CPU."""
    spread = _cpu_spread(name)
    assert 0 < spread <= SPREAD_CAP
    r = _solve(_cxx("lbfgsb_dev_test", hip_built, extra=CXX_FLAGS), name, 0)
    assert r["backend"] == "device"
    _check_solve(name, r, 10 * spread, "device")


BFGS_LEGS = ["apply_Hv", "free_60", "free_skip_mid", "free_skip_newest", "free_none"]


def _check_bfgs(out, what):
    for k, leg in enumerate(BFGS_LEGS):
        f = out[k].split()
        assert f[0] == leg
        err_dev, err_host, scale, outside = float(f[1]), float(f[2]), float(f[3]), int(f[4])
        print(f"{what} {leg}: |dev - ld| {err_dev:.3g}, |host - ld| {err_host:.3g}, ratio to bar {err_dev / (10 * err_host) if err_host else 0:.3g}")
        assert outside == 0, (what, leg)                              # exactly 0 outside the mask
        assert err_dev <= 10 * err_host, (what, leg)                  # (free_none: both exactly zero)
        assert (scale > 0.05 and err_host < 1e-12 * scale) if leg != "free_none" else scale == 0.0, (what, leg)       # the reference is one
    assert out[len(BFGS_LEGS)].split() == ["copy", "1"], what


@pytest.mark.parametrize("n", [70001, K + 1])
def test_device_bfgs_matrix_logic_vs_long_double_recursion(n):
    """DevBFGSMat on the stand-in (m = 4, 7 corrections, so the storage wraps): a H v with a != 1 and the masked recursion under four
    masks -- 60 %, one with a stored pair to skip, one with the newest pair to skip (theta from the next), none free -- within 10 x the
    host BFGSMat's own distance from a long-double recursion, and a copy taken before reset() keeps applying the old pairs."""
    exe = _cpu_exe()
    for order, what in ORDERS.items():
        _check_bfgs(_lines(exe, f"bfgs {n} {order}\n"), what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [70001, K + 1])
def test_device_bfgs_matrix_vs_long_double_recursion(hip_built, n):
    _check_bfgs(_lines(_cxx("lbfgsb_dev_test", hip_built, extra=CXX_FLAGS), f"bfgs {n} 0\n"), "device")


# ================================================================================================ vector kernels
class Vec:
    """The library's vector entries on one context.  Every vector is a slice that starts one element into a guarded allocation (NaN for
    doubles, 7 for masks), so that a read past the ends poisons a result and a write past them shows."""

    def __init__(self, env):
        import torch
        self.torch, self.lib = torch, env["lib"]
        self.lib.moihgp_dvec_ctx_new.restype = C.c_void_p
        self.lib.moihgp_dvec_ctx_del.argtypes = [C.c_void_p]
        self.ctx = self.lib.moihgp_dvec_ctx_new()
        assert self.ctx

    def close(self):
        self.lib.moihgp_dvec_ctx_del(self.ctx)

    def dev(self, a):
        a = np.ascontiguousarray(a)
        mask = a.dtype == np.uint8
        whole = self.torch.full((a.size + 2,), 7 if mask else float("nan"), dtype=self.torch.uint8 if mask else self.torch.float64, device="cuda")
        whole[1:-1] = self.torch.from_numpy(a).cuda()
        return whole

    @staticmethod
    def p(whole):
        return None if whole is None else C.c_void_p(whole.data_ptr() + whole.element_size())

    def host(self, whole):
        """The n entries, after checking that the guards still stand."""
        self.lib.moihgp_dvec_sync(C.c_void_p(self.ctx))
        h = whole.cpu().numpy()
        assert (h[0] == 7 and h[-1] == 7) if h.dtype == np.uint8 else (np.isnan(h[0]) and np.isnan(h[-1])), "written outside the vector"
        return h[1:-1].copy()

    def call(self, name, n, *args):
        self.torch.cuda.synchronize()                                 # (torch fills on its own stream, the kernels run on the context's)
        conv = [C.c_double(a) if isinstance(a, float) else a if isinstance(a, (type(None), type(C.byref(C.c_double())))) else self.p(a) for a in args]
        assert getattr(self.lib, "moihgp_dvec_" + name)(C.c_void_p(self.ctx), C.c_size_t(n), *conv) == 0, name

    def reduce(self, name, n, *args):
        """A reduction, called twice: the same bits both times."""
        r1, r2 = C.c_double(float("inf")), C.c_double(float("-inf"))
        self.call(name, n, *args, C.byref(r1))
        self.call(name, n, *args, C.byref(r2))
        assert np.float64(r1.value).tobytes() == np.float64(r2.value).tobytes(), name
        return r1.value


@pytest.fixture(scope="module")
def vec(env):
    v = Vec(env)
    yield v
    v.close()


def _box(n, rng):
    lb, ub = -0.5 * np.ones(n), 0.7 * np.ones(n)
    lb[::7] = ub[::7] = 0.1                                           # fixed variables
    return lb, ub


def _masks(n, rng):
    return {"absent": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "random": (rng.random(n) < 0.6).astype(np.uint8)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_elementwise_kernels_at_grid_edges(vec, n):
    """sub, clamp, scale, axpy, active_set and the xt of proj_step.  One rounding per entry: with alpha (step) a power of two the result is
    numpy's float64 one exactly (sub, clamp, scale and active_set always are); with a general alpha the fused a x + y is within
    u (|alpha x| + |y|) of the long-double value (2^-9 of slack for the reference's own two roundings at 2^-64).  Nothing outside the n
    entries changes.  n = 2^20 is where the grid saturates: beyond it a thread takes a second entry."""
    rng = np.random.default_rng(n)
    a, b, x0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    lb, ub = _box(n, rng)
    da, db, dlb, dub = vec.dev(a), vec.dev(b), vec.dev(lb), vec.dev(ub)
    out = vec.dev(np.zeros(n))
    vec.call("sub", n, da, db, out)
    assert np.array_equal(vec.host(out), a - b)
    dx = vec.dev(x0)
    vec.call("clamp", n, dx, dlb, dub)
    x = np.minimum(np.maximum(x0, lb), ub)
    assert np.array_equal(vec.host(dx), x)
    slack = 1 + 2.0 ** -9
    for mname, mask in _masks(n, rng).items():
        dm = None if mask is None else vec.dev(mask)
        on = np.ones(n, bool) if mask is None else mask > 0
        for alpha in (0.5, -1.7):
            vec.call("scale", n, alpha, da, out, dm)
            assert np.array_equal(vec.host(out), np.where(on, alpha * a, 0.0)), (mname, alpha)
        y = vec.dev(b)
        vec.call("axpy", n, -2.0, da, y, dm)
        assert np.array_equal(vec.host(y), np.where(on, b - 2.0 * a, b)), mname
        y = vec.dev(b)
        vec.call("axpy", n, -1.7, da, y, dm)
        got = vec.host(y)
        assert np.array_equal(got[~on], b[~on]), mname
        err = np.abs(got.astype(ld) - (ld(-1.7) * a.astype(ld) + b.astype(ld)))
        assert np.all(err[on] <= (slack * U * (np.abs(1.7 * a) + np.abs(b)))[on]), mname
    res = vec.dev(a)
    vec.call("scale", n, 1.0 / 3.0, res, res, None)                   # in place, as the solver's `scale(1 / theta, res, res)`
    assert np.array_equal(vec.host(res), (1.0 / 3.0) * a)

    # active set: x exactly on lb, exactly on ub, inside, lb == ub; g = +0.0, -0.0, +-denormal, +-1
    i = np.arange(n)
    lb2, ub2 = -0.5 * np.ones(n), 0.7 * np.ones(n)
    lb2[i % 4 == 3] = ub2[i % 4 == 3] = 0.1
    xa = np.where(i % 4 == 0, lb2, np.where(i % 4 == 1, ub2, np.where(i % 4 == 2, 0.5 * (lb2 + ub2), 0.1)))
    g = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0])[(i // 4) % 6] if n else np.zeros(0)
    free = vec.dev(np.full(n, 9, np.uint8))
    vec.call("active_set", n, vec.dev(xa), vec.dev(g), vec.dev(lb2), vec.dev(ub2), free)
    want = ~(((xa <= lb2) & (g > 0)) | ((xa >= ub2) & (g < 0)) | (lb2 == ub2))
    assert np.array_equal(vec.host(free), want.astype(np.uint8))
    if n >= 24:
        assert not want[0 + 4 * 2] and want[0 + 4 * 0] and want[0 + 4 * 1] and want[0 + 4 * 3]      # on lb: fixed by a denormal g > 0, free at +-0 and g < 0
        assert not want[1 + 4 * 3] and want[1 + 4 * 2]                                             # on ub: fixed by a denormal g < 0

    # projected step: xt = clamp(xp + step drt, lb, ub)
    dg = vec.dev(b)
    for step in (0.25, 0.3):
        xt, dec = vec.dev(np.zeros(n)), C.c_double()
        vec.call("proj_step", n, dx, da, step, dlb, dub, dg, xt, C.byref(dec))
        got = vec.host(xt)
        if step == 0.25:
            assert np.array_equal(got, np.minimum(np.maximum(x + 0.25 * a, lb), ub))
        else:
            want_ld = np.minimum(np.maximum(x.astype(ld) + ld(step) * a.astype(ld), lb.astype(ld)), ub.astype(ld))      # (clamping does not widen an error)
            assert np.all(np.abs(got.astype(ld) - want_ld) <= slack * U * (np.abs(step * a) + np.abs(x)))
        assert np.all(got >= lb) and np.all(got <= ub) and (n < 7 or ((got == lb) | (got == ub)).sum() > n // 7)     # proj_step clamps


def _sum_ref(terms_ld):
    return float(np.sum(terms_ld)), float(np.sum(np.abs(terms_ld)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_reductions_at_grid_edges(vec, n):
    """dot (masked and not) and the `dec` of proj_step against long-double sums of the same terms, within gamma(SUM_ROUNDINGS(n) + 2) of the
    sum of absolute terms (module docstring); every reduction twice with the same bits.  Inputs: random; all terms equal; one 1e16 among
    ones at each index where the sum changes hands; +-1e8 in the two terms of one thread (i, i + 262144), which must cancel; a single
    non-zero at each of those indices, whose dot is that product exactly -- the leg that catches a finish pass which skips partials."""
    rng = np.random.default_rng(1000 + n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    da, db, dm = vec.dev(a), vec.dev(b), vec.dev(mask)
    terms = a.astype(ld) * b.astype(ld)
    worst = 0.0

    def check(got, terms_ld, what):
        nonlocal worst
        ref, tot = _sum_ref(terms_ld)
        bar = sum_bar(n, tot)
        assert abs(ld(got) - np.sum(terms_ld)) <= bar, (what, got, ref, bar)
        if bar:
            worst = max(worst, float(abs(ld(got) - np.sum(terms_ld))) / bar)

    check(vec.reduce("dot", n, da, db, None), terms, "random")
    check(vec.reduce("dot", n, da, db, dm), terms * (mask > 0), "random, masked")
    if n == 0:
        assert vec.reduce("dot", n, da, db, None) == 0.0
        return
    c1, c2 = vec.dev(np.full(n, 0.1)), vec.dev(np.full(n, 0.3))
    check(vec.reduce("dot", n, c1, c2, None), np.full(n, ld(0.1) * ld(0.3)), "all terms equal")

    ones, ones2, zeros, zeros2 = vec.dev(np.ones(n)), vec.dev(np.ones(n)), vec.dev(np.zeros(n)), vec.dev(np.zeros(n))
    ones_m, zeros_m = vec.dev(np.ones(n, np.uint8)), vec.dev(np.zeros(n, np.uint8))
    for i in special(n):
        ones[1 + i] = 1e16                                            # (index 0 of the vector is element 1 of the guarded allocation)
        t = np.ones(n, ld); t[i] = ld(1e16)
        check(vec.reduce("dot", n, ones, ones2, None), t, ("1e16 among ones", i))
        ones[1 + i] = 1.0
        zeros[1 + i], zeros2[1 + i] = 3.7, -1.3
        for m, want in ((None, 3.7 * -1.3), (ones_m, 3.7 * -1.3), (zeros_m, 0.0)):
            assert vec.reduce("dot", n, zeros, zeros2, m) == want, ("single non-zero", i)
        if i + K < n:
            zeros[1 + i], zeros2[1 + i], zeros[1 + i + K], zeros2[1 + i + K] = 1e8, 1.0, -1e8, 1.0      # (products exact: nothing but 0.0 is right)
            assert vec.reduce("dot", n, zeros, zeros2, None) == 0.0, ("pair alone", i)
            zeros[1 + i + K], zeros2[1 + i + K] = 0.0, 0.0
            keep = da[1 + i].item(), db[1 + i].item(), da[1 + i + K].item(), db[1 + i + K].item()
            da[1 + i], db[1 + i], da[1 + i + K], db[1 + i + K] = 1e8, 1.0, -1e8, 1.0
            t = terms.copy(); t[i], t[i + K] = ld(1e8), ld(-1e8)
            check(vec.reduce("dot", n, da, db, None), t, ("+-1e8 in one thread's two terms", i))
            da[1 + i], db[1 + i], da[1 + i + K], db[1 + i + K] = keep
        zeros[1 + i], zeros2[1 + i] = 0.0, 0.0

    # dec = sum gradp (xt - xp) over the xt the kernel wrote
    lb, ub = _box(n, rng)
    x = np.minimum(np.maximum(rng.standard_normal(n), lb), ub)
    dx, dlb, dub = vec.dev(x), vec.dev(lb), vec.dev(ub)
    for step in (0.25, 0.3):
        xt = vec.dev(np.zeros(n))
        dec = vec.reduce("proj_step", n, dx, da, step, dlb, dub, db, xt)
        check(dec, b.astype(ld) * (vec.host(xt).astype(ld) - x.astype(ld)), ("dec", step))
    print(f"n = {n}: worst reduction error / bar {worst:.3g} ({sum_roundings(n) + 2} roundings)")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_projected_gradient_norm_at_grid_edges(vec, n):
    """max_i |clamp(x_i - g_i, lb_i, ub_i) - x_i| equals numpy's maximum exactly, wherever the maximum sits; a NaN in g at any index comes
    back as NaN (`block_max` and the kernel promise that a NaN sticks)."""
    rng = np.random.default_rng(2000 + n)
    lb, ub = _box(n, rng)
    x, g = np.minimum(np.maximum(rng.standard_normal(n), lb), ub), rng.standard_normal(n)
    dx, dg, dlb, dub = vec.dev(x), vec.dev(g), vec.dev(lb), vec.dev(ub)

    def want(x, g, lb, ub):
        return float(np.abs(np.minimum(np.maximum(x - g, lb), ub) - x).max()) if n else 0.0

    assert vec.reduce("proj_grad_norm", n, dx, dg, dlb, dub) == want(x, g, lb, ub)
    wide_l, wide_u = vec.dev(np.full(n, -100.0)), vec.dev(np.full(n, 100.0))
    for i in special(n):
        keep = g[i]
        dg[1 + i] = -50.0 - 1e-5 * i; g[i] = -50.0 - 1e-5 * i
        w = want(x, g, np.full(n, -100.0), np.full(n, 100.0))
        assert w == abs((x[i] - g[i]) - x[i]) and vec.reduce("proj_grad_norm", n, dx, dg, wide_l, wide_u) == w, ("maximum", i)
        dg[1 + i] = float("nan")
        assert math.isnan(vec.reduce("proj_grad_norm", n, dx, dg, wide_l, wide_u)), ("NaN in g, wide box", i)
        assert math.isnan(vec.reduce("proj_grad_norm", n, dx, dg, dlb, dub)), ("NaN in g", i)
        dg[1 + i] = keep; g[i] = keep
    assert vec.reduce("proj_grad_norm", n, dx, dg, dlb, dub) == want(x, g, lb, ub)
