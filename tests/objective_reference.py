"""Shared by the tests of the full objective gradient (test_objective_entries): a float64 numpy restatement of one tick of
MOIHGP::negLogLikelihood with gradient (moihgp.h:460-611 in its closed U-gradient form, oracle/moihgp_numpy.py::MOIHGP.nll with
literal_ugrad=False) followed by MOIHGP::step (moihgp.h:148-226), vectorised over latents for any d and P on the C oracle's own per-latent
matrices and polar factor, summed over a window of W ticks (W = 1 is the per-tick ABI), together with the conditioning scale of every entry.
Not a test; pytest does not rewrite the asserts of this module, so each carries its own message.

The vector is [U (M L) | S (L) | sigma (1) | per-latent (L P)].  Along the trajectory every entry accumulates the magnitudes of what is added
to it, cancelling or not.  With A_t = |U|^T |y_t| (the absolute terms of U^T y_t) and
Pbar_{t,c} = (|y_{t,c}| + |HA| |x_{t,c}|) |1 - HA K| / S_igp (the scale of pv, which takes the raw y(l), sic moihgp.h:510):
    grad_U[r, c]      sum_t |y_{t,r}| (Pbar_{t,c} / sqrt(S_c) + A_{t,c} / sigma)
    grad_S[l]         sum_t [ 1/2 / S_l + 1/2 S_l^-3/2 Pbar_{t,l} A_{t,l} + sigma / S_l^2 G_{t,l,noise} ]
    grad_sigma        sum_t [ 1/2 m_n / sigma + 1/2 R_t / sigma^2 + sum_l G_{t,l,noise} / S_l ],  R_t = || |y_t| + |U| A_t ||_2  (the error of a norm
                      is at most the norm of the error, which also holds at M = L where r_t itself is rounding noise)
    per-latent [l, p] G = sum_t (|v dv_p| + 1/2 |v^2 / S - 1| |dS_p|) / S, the G of test_gradient_entries
    loss              W (1/2 |log sum S| + 1/2 m_n |log sigma|) + 1/2 sum_t R_t / sigma, plus sum 1/2 (v^2 / S + |log S|) where the latent losses
                      are included (threading on, and the overload without gradient)
    x[l, i], dx[l, p, i]   the largest magnitude the entry took at any tick, start state included
A tick with missing outputs is projected by least squares over the observed rows (moihgp.h:167-178); its dense products with y_t are NaN as
in the reference, so the loss and the U / S / sigma blocks (and their scales) are NaN from that tick on, the per-latent block and the state
finite.
u_rounding_bound is a second, far tighter hold on the U block alone: the first-order bound of its rounding error in fp64, for a reference run
on the evaluation's own mixing matrix (its docstring derives it; scale[`u_hist`] is the share of the carried state)."""
import functools

import numpy as np

from conftest import rel_err
from parity_support import synth_params, synth_params_stacked

DT = 0.1
HIDDEN = 1e-2                                            # an entry below this share of its case's largest is invisible to the old bar of 1e-8
MATS = ("K", "S", "HA", "AKHA", "dS", "dK", "dAKHA", "HdA")
BLOCKS = ("U", "S", "sigma", "lat")                      # the blocks of the gradient vector
QUANTITIES = BLOCKS + ("loss", "x", "dx")


def blocks(M, L, P):
    n = M * L + L + 1 + L * P
    return dict(U=slice(0, M * L), S=slice(M * L, M * L + L), sigma=slice(M * L + L, M * L + L + 1), lat=slice(M * L + L + 1, n))


def fused_lik_fits(M, L, P=3):
    """csrc/tick.hip fused_lik_fits restated: M L <= 8192, M >= L and 2 M + (4 + P) L + 256 doubles of LDS within 48 KiB."""
    return M * L <= 8192 and M >= L and (2 * M + (4 + P) * L + 256) * 8 <= 48 * 1024


class Model:
    """What one tick needs, taken from a cref.GP after update(): its polar factor, S, sigma and the per-latent matrices, stacked over latents."""

    def __init__(self, gp, U=None):
        M, L = gp.M, gp.L
        self.M, self.L, self.d, self.P = M, L, gp.igp_dim, gp.num_igp_param
        self.U = gp.U if U is None else np.array(U, dtype=np.float64).reshape(M, L)     # (U: the device's own polar factor, for u_rounding_bound)
        p = gp.params
        self.S = p[M * L:M * L + L].copy()
        self.sigma = float(p[M * L + L])
        m = {k: np.stack([np.asarray(gp.latent(l).mat(k), dtype=np.float64) for l in range(L)]) for k in MATS}
        self.K, self.Sg, self.HA, self.AKHA, self.dS, self.dK, self.dAKHA, self.HdA = (m[k] for k in MATS)
        self.f = (1.0 - np.einsum("li,li->l", self.HA, self.K)) / self.Sg          # moihgp.h:511


def tick_np(m, x, y, dx, dhx=None):
    """One tick on the pre-step state (x, dx): the two losses, the gradient vector, the scale of every entry, and the state after the step.
    dhx [L]: what the error of HA x is bounded by, in units of the state's per-step rounding (u_rounding_bound)."""
    M, L, P = m.M, m.L, m.P
    U, S, sigma = m.U, m.S, m.sigma
    obs = ~np.isnan(y)
    with np.errstate(invalid="ignore"):
        Uty = U.T @ y                                                           # all NaN when an output is missing (moihgp.h:499-563)
        if obs.all():
            a = Uty
        else:                                                                   # moihgp.h:167-178
            U0 = U[obs]
            a = np.linalg.solve(U0.T @ U0, U0.T @ y[obs])
        sq = np.sqrt(S)
        Ty = a / sq
        hx = np.einsum("li,li->l", m.HA, x)
        v = Ty - hx                                                             # ihgp.h:204-222
        dv = -np.einsum("lpi,li->lp", m.HdA, x) - np.einsum("li,lpi->lp", m.HA, dx)
        w = v * v / m.Sg
        lat_loss = 0.5 * (w + np.log(m.Sg))
        g = (v[:, None] * dv - 0.5 * (w - 1.0)[:, None] * m.dS) / m.Sg[:, None]
        dn = g[:, P - 1]
        pv = (y[:L] - hx) * m.f                                                 # moihgp.h:505-512 (raw y(l), sic)
        r = np.linalg.norm(y - U @ Uty)                                         # moihgp.h:501
        m_n = max(float(M - L), 0.0)
        loss = 0.5 * np.log(S.sum()) + 0.5 * m_n * np.log(sigma) + 0.5 * r / sigma       # moihgp.h:503
        grad = np.concatenate([np.outer(y, pv / sq - Uty / sigma).ravel(),                  # moihgp.h:538-552, closed form
                               0.5 / S - 0.5 * S ** -1.5 * pv * Uty - dn * sigma / S ** 2,  # moihgp.h:555-561, :604
                               [0.5 * (m_n - r / sigma) / sigma + (dn / S).sum()],          # moihgp.h:563, :605
                               g.ravel()])                                                  # moihgp.h:608-609
        # the magnitudes of what was added
        ay = np.abs(y)
        A = np.abs(U).T @ ay
        Pbar = (ay[:L] + np.einsum("li,li->l", np.abs(m.HA), np.abs(x))) * np.abs(m.f)
        G = (np.abs(v[:, None] * dv) + 0.5 * np.abs(w - 1.0)[:, None] * np.abs(m.dS)) / m.Sg[:, None]
        R = np.linalg.norm(ay + np.abs(U) @ A)
        s_grad = np.concatenate([np.outer(ay, Pbar / sq + A / sigma).ravel(),
                                 0.5 / S + 0.5 * S ** -1.5 * Pbar * A + sigma / S ** 2 * G[:, P - 1],
                                 [0.5 * m_n / sigma + 0.5 * R / sigma ** 2 + (G[:, P - 1] / S).sum()],
                                 G.ravel()])
        s_loss = 0.5 * abs(np.log(S.sum())) + 0.5 * m_n * abs(np.log(sigma)) + 0.5 * R / sigma
        s_lat = (0.5 * (w + np.abs(np.log(m.Sg)))).sum()
        # u_rounding_bound: what an error of HA x adds to grad_U through pv, and the magnitudes that this step's own rounding is a share of
        u_hist = np.outer(ay, np.abs(m.f) / sq * (0.0 if dhx is None else dhx)).ravel()
        xi = np.einsum("lij,lj->li", np.abs(m.AKHA), np.abs(x)) + np.abs(m.K) * (A / sq)[:, None]
    # ihgp.h:37-57 on the projected observation
    xn = np.einsum("lij,lj->li", m.AKHA, x) + m.K * Ty[:, None]
    dxn = np.einsum("lpij,lj->lpi", m.dAKHA, x) + np.einsum("lij,lpj->lpi", m.AKHA, dx) + m.dK * Ty[:, None, None]
    return dict(loss=loss, loss_on=loss + lat_loss.sum(), grad=grad, x=xn, dx=dxn,
                scale=dict(grad=s_grad, loss=s_loss, loss_on=s_loss + s_lat, u_hist=u_hist), xi=xi)


def window_np(m, Y, x0, dx0):
    """tick_np summed over the ticks of Y [W, M], the state carried; `ticks` keeps every tick's own result (for the per-tick ABI)."""
    x, dx = np.array(x0, dtype=np.float64), np.array(dx0, dtype=np.float64)
    xs, dxs = np.abs(x), np.abs(dx)
    tot = None
    ticks = []
    SUMMED = ("grad", "loss", "loss_on", "u_hist")
    xis, resp, pw = [], [], m.HA                                                # resp[k] = |HA AKHA^k|: how HA x answers a state error k steps old
    for y in Y:
        dhx = sum(np.einsum("li,li->l", resp[len(xis) - 1 - j], xis[j]) for j in range(len(xis))) if xis else None
        t = tick_np(m, x, y, dx, dhx)
        x, dx = t["x"], t["dx"]
        xis.append(t.pop("xi")); resp.append(np.abs(pw)); pw = np.einsum("li,lij->lj", pw, m.AKHA)
        xs = np.maximum(xs, np.abs(x)); dxs = np.maximum(dxs, np.abs(dx))
        t["scale"].update(x=xs, dx=dxs)
        ticks.append(t)
        if tot is None:
            tot = dict(loss=t["loss"], loss_on=t["loss_on"], grad=t["grad"].copy(), scale={k: np.array(t["scale"][k], dtype=np.float64) for k in SUMMED})
        else:
            tot["loss"] += t["loss"]; tot["loss_on"] += t["loss_on"]; tot["grad"] += t["grad"]
            for k in SUMMED:
                tot["scale"][k] += t["scale"][k]
    tot.update(x=x, dx=dx)
    tot["scale"].update(x=xs, dx=dxs)
    tot["ticks"] = ticks
    return tot


# ------------------------------------------------------------------------------------------------ the draws
def stack_J(kern):
    return int(kern[-1]) if "x" in kern else 0


def draw(kern, M, L, W, nan=False):
    """test_window_objective_vs_oracle_loop's draw (seed M + 3 L + W, plus J for a stacked kernel): mixing parameter eye + 0.2 randn (update
    takes its polar factor), S uniform in [0.5, 2], sigma = 0.04, synth_params / synth_params_stacked, Y = 0.5 randn, x0 = 0.2 randn,
    dx0 = 0.05 randn.  nan: NaN at tick 0 row 0 and at tick W / 2 in rows 1, M / 2 and M - 1."""
    J = stack_J(kern)
    rng = np.random.default_rng(M + 3 * L + W + J)
    d = (2 if kern.startswith("Matern32") else 3) * max(J, 1)
    P = 2 * J + 1 if J else 3
    mix = (np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel()
    S = rng.uniform(0.5, 2, L)
    igp = synth_params_stacked(L, J, rng) if J else synth_params(L, rng)
    params = np.concatenate([mix, S, [0.04], igp.ravel()])
    Y = rng.standard_normal((W, M)) * 0.5
    x0 = 0.2 * rng.standard_normal((L, d)); dx0 = 0.05 * rng.standard_normal((L, P, d))
    if nan:
        assert M - 3 >= L and len({1, M // 2, M - 1}) == 3, "the partially observed draw needs three distinct rows and L observed outputs"
        Y[0, 0] = np.nan; Y[W // 2, [1, M // 2, M - 1]] = np.nan
    return params, Y, x0, dx0


@functools.lru_cache(maxsize=None)
def case(kern, M, L, W, nan=False):
    """Inputs, the C oracle's object and the float64 reference with its scales of one case: computed once, left unchanged."""
    from oracle import cref
    params, Y, x0, dx0 = draw(kern, M, L, W, nan)
    gp = cref.GP(DT, M, L, kern); gp.set_literal_ugrad(0)
    gp.update(params)
    ref = window_np(Model(gp), Y, x0, dx0)
    frozen = [params, Y, x0, dx0]
    for r in [ref] + ref["ticks"]:
        frozen += [r["grad"], r["x"], r["dx"]] + [np.asarray(v) for v in r["scale"].values()]
    for a in frozen:
        if isinstance(a, np.ndarray) and a.ndim:
            a.setflags(write=False)
    return dict(kern=kern, M=M, L=L, W=W, d=x0.shape[1], P=dx0.shape[1], params=params, Y=Y, x0=x0, dx0=dx0, gp=gp, ref=ref)


def oracle_loop(C, threading=False):
    """The learners' loop on the C oracle (cref.GP.negLogLikelihood then step, per tick): the totals and every tick's own result."""
    from oracle import cref
    gp = C["gp"]
    if threading:
        gp = cref.GP(DT, C["M"], C["L"], C["kern"], threading=True); gp.set_literal_ugrad(0)
        gp.update(C["params"])
    x, dx, loss, grad, ticks = C["x0"], C["dx0"], 0.0, np.zeros(gp.num_param), []
    for y in C["Y"]:
        l1, g1 = gp.negLogLikelihood(x, y, dx)
        l2 = gp.negLogLikelihood(x, y)
        x, _, dx = gp.step(x, y, dx)
        loss += l1; grad += g1
        ticks.append(dict(loss=l1, lik2=l2, grad=g1, x=x, dx=dx))
    return dict(loss=loss, grad=grad, x=x, dx=dx, ticks=ticks)


# ------------------------------------------------------------------------------------------------ the measure
def _worst(a, b, s, what):
    """max |a - b| / s over the entries where b is finite; the NaN pattern of a must be b's; a zero scale demands an exact zero."""
    a, b, s = (np.asarray(v, dtype=np.float64) for v in (a, b, s))
    assert a.shape == b.shape == s.shape, (what, a.shape, b.shape, s.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "NaN pattern differs from the reference's")
    fin = ~np.isnan(b)
    a, b, s = a[fin], b[fin], s[fin]
    zero = s == 0
    assert np.all(a[zero] == b[zero]), (what, "differs where nothing can have been added")
    e = np.abs(a - b)[~zero] / s[~zero]
    assert np.all(np.isfinite(e)), (what, "not finite")
    return float(e.max()) if e.size else 0.0


def entry_errors(got, ref, M, L, P, loss_key="loss"):
    """Worst |got - ref| / scale per quantity, entry by entry.  got: dict with any of loss, grad, x, dx; ref: a result of window_np or one of
    its ticks; loss_key: `loss` (threading off) or `loss_on` (the latent losses included)."""
    out = {}
    sc = ref["scale"]
    if got.get("grad") is not None:
        for k, sl in blocks(M, L, P).items():
            out[k] = _worst(np.asarray(got["grad"])[sl], ref["grad"][sl], sc["grad"][sl], k)
    if got.get("loss") is not None:
        out["loss"] = _worst(got["loss"], ref[loss_key], sc[loss_key], "loss")
    for q in ("x", "dx"):
        if got.get(q) is not None:
            out[q] = _worst(np.asarray(got[q]).reshape(ref[q].shape), ref[q], sc[q], q)
    return out


EPS = 2.0 ** -52


def u_rounding_bound(ref, M, L, W, d):
    """First-order bound of the rounding error of every grad_U entry of a correct fp64 evaluation in any order of summation, for a reference that
    was run on the evaluation's own mixing matrix (Model(gp, U=...)), so that no input differs: per entry [r, c]
        grad_U = sum_t y_tr (pv_tc / sqrt(S_c) - (U^T y_t)_c / sigma),     scale s = sum_t |y_tr| (Pbar_tc / sqrt(S_c) + A_tc / sigma)
    (i)  the sum over W ticks, the product with y, the difference and the division by sigma: (W + 3) eps s
    (ii) (U^T y_t)_c, an inner product of M terms, on the window route through S^-1/2 and back: (M + 3) eps of A_tc / sigma, at most (M + 3) eps s
    (iii) pv = (y_c - HA x) f / sqrt(S): the inner products HA x and HA K of d terms, 1 - HA K, the division by S_igp, 1 / sqrt(S) and
          the products: (2 d + 8) eps of Pbar_tc / sqrt(S_c), at most (2 d + 8) eps s
    (iv) the carried state: x_t of the evaluation differs from the reference's.  One step x' = AKHA x + K Ty adds at most
          (M + d + 5) eps xi, xi = |AKHA| |x| + |K| A / sqrt(S) (Ty within (M + 3) eps A / sqrt(S), the d-term products and sums), and an
          error made k steps ago reaches HA x as HA AKHA^k times it: |delta HA x_t| <= (M + d + 5) eps sum_j |HA AKHA^(t-1-j)| xi_j (window_np;
          the powers of AKHA itself, which decay, not of |AKHA|, which need not).  Through pv it adds
          (M + d + 5) eps sum_t |y_tr| |f_c| / sqrt(S_c) |delta HA x_t|_c / eps = (M + d + 5) eps u_hist
    The sum, doubled: a comparison of two such evaluations, the device's and the restatement's."""
    sl = blocks(M, L, 1)["U"]
    s = ref["scale"]["grad"][sl]
    return 2 * EPS * ((W + M + 2 * d + 14) * s + (M + d + 5) * ref["scale"]["u_hist"])


def old_measure(grad, gref):
    """What every test of the vector used before: max |a - b| over max |b| of the whole concatenated vector (finite entries)."""
    fin = ~np.isnan(gref)
    return rel_err(np.asarray(grad)[fin], gref[fin])


def hidden(ref, M, L, P):
    """Per block: (number of finite entries below HIDDEN of the largest finite entry of the whole vector, number of finite entries)."""
    g = np.abs(ref["grad"])
    fin = ~np.isnan(g)
    top = g[fin].max()
    return {k: (int((g[sl][fin[sl]] < HIDDEN * top).sum()), int(fin[sl].sum())) for k, sl in blocks(M, L, P).items()}
