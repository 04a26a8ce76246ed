"""The numpy definitions the whole-stream sweeps of include/moihgp.h are held to: smoother, forecasts, fixed-lag and off-grid smoothers, slopes,
the seeded sampler, and the OILMM projection of observations to latents.  CPU only (numpy, scipy and the numpy oracle; no torch): the test
modules import from here and never from each other.  The independent cross-checks of these definitions (textbook loops, dense GP posteriors)
live in the test module of the sweep they vouch for."""
import numpy as np
import scipy.linalg as sl

from oracle.moihgp_numpy import IHGP


# ------------------------------------------------------------------------------------------------ smoother
def model(kern, dt, prm):
    g = IHGP(dt, kern)
    g.update(np.asarray(prm, dtype=np.float64))
    A, Pinf = g.A, g.ss.Pinf
    Q = Pinf - A @ Pinf @ A.T
    return A, (Q + Q.T) / 2.0, float(prm[2]), Pinf


def tables(kern, dt, prm):
    """Kalman DARE (scipy), K, G = PF A^T P^-1, Ps from the d^2 x d^2 Stein system; None where scipy's solver fails (its residual)."""
    A, Q, R, Pinf = model(kern, dt, prm)
    d = A.shape[0]
    H = np.zeros((1, d)); H[0, 0] = 1.0
    try:
        P = sl.solve_discrete_are(A.T, H.T, Q, np.array([[R]]))
    except (np.linalg.LinAlgError, ValueError):
        return None
    res = A @ P @ A.T - np.outer(A @ P[:, 0], A @ P[:, 0]) / (P[0, 0] + R) + Q - P
    if not np.all(np.isfinite(P)) or np.max(np.abs(res)) > 1e-10 * np.max(np.abs(P)):
        return None
    S = P[0, 0] + R
    K = P[:, 0] / S
    PF = P - np.outer(K, P[0])
    G = PF @ A.T @ np.linalg.inv(P)
    Ps = np.linalg.solve(np.eye(d * d) - np.kron(G, G), (PF - G @ P @ G.T).ravel()).reshape(d, d)
    return dict(A=A, Q=Q, R=R, Pinf=Pinf, P=P, S=S, K=K, PF=PF, G=G, Ps=(Ps + Ps.T) / 2, var_f=PF[0, 0], var_s=Ps[0, 0])


def smooth_np(tbs, Ty, x_in=None):
    """The two sweeps of include/moihgp.h, vectorised over latents: tbs one table dict per row of Ty [L][T]."""
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs]); G = np.stack([t["G"] for t in tbs])
    L, T = Ty.shape
    d = A.shape[1]
    x = np.zeros((L, d)) if x_in is None else np.array(x_in, dtype=np.float64)
    p = np.zeros((L, T)); v = np.zeros((L, T))
    for t in range(T):
        xp = np.einsum("lij,lj->li", A, x)
        p[:, t] = xp[:, 0]
        y = Ty[:, t]
        v[:, t] = np.where(np.isnan(y), 0.0, y - p[:, t])
        x = xp + K * v[:, t:t + 1]
    s = np.zeros((L, d)); ys = np.zeros((L, T))
    for t in range(T - 1, -1, -1):
        s = np.einsum("lij,lj->li", G, s) + K * v[:, t:t + 1]
        ys[:, t] = p[:, t] + s[:, 0]
    return ys, x


# ------------------------------------------------------------------------------------------------ forecasts
def gain_tables(kern, dt, prm, gains):
    """A, K, M of include/moihgp.h: "kalman" from the smoother's numpy tables (plus Pinf, PF for the variances), "handle" from the numpy
    oracle's IHGP.update (the reference's literal DARE)."""
    if gains == "kalman":
        tb = tables(kern, dt, prm)
        assert tb is not None, prm
        return dict(A=tb["A"], K=tb["K"], M=tb["A"] - np.outer(tb["K"], tb["A"][0]), Pinf=tb["Pinf"], PF=tb["PF"], R=tb["R"])
    g = IHGP(dt, kern)
    g.update(np.asarray(prm, dtype=np.float64))
    return dict(A=g.A, K=g.K[:, 0], M=g.AKHA)


def states_np(tbs, Ty, x_in=None):
    """x[t] = M x[t-1] + K y[t], or A x[t-1] where y[t] is NaN, vectorised over latents: [L][T][d]."""
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs]); M = np.stack([t["M"] for t in tbs])
    L, T = Ty.shape
    d = A.shape[1]
    x = np.zeros((L, d)) if x_in is None else np.array(x_in, dtype=np.float64)
    xs = np.zeros((L, T, d))
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):
            y = Ty[:, t]
            miss = np.isnan(y)
            xo = np.einsum("lij,lj->li", M, x) + K * np.where(miss, 0.0, y)[:, None]
            xm = np.einsum("lij,lj->li", A, x)
            x = np.where(miss[:, None], xm, xo)
            xs[:, t] = x
    return xs


def forecast_np(tbs, Ty, horizons, x_in=None):
    """fc[k][l][t] = H A^h_k x_l[t]; also the end state and each latent's scale max_t |H x_l[t]| (the h = 0 row the errors are taken against)."""
    xs = states_np(tbs, Ty, x_in)
    L, T, d = xs.shape
    c = np.array([[np.linalg.matrix_power(t["A"], int(h))[0] for t in tbs] for h in horizons])          # [K][L][d]
    with np.errstate(over="ignore", invalid="ignore"):
        fc = np.einsum("kld,ltd->klt", c, xs)
    xe = xs[:, -1] if T else (np.zeros((L, d)) if x_in is None else np.array(x_in, dtype=np.float64))
    scale = np.max(np.abs(xs[:, :, 0]), axis=1) if T else np.ones(L)
    return fc, xe, scale


def forecast_var_np(tb, h):
    Ah = np.linalg.matrix_power(tb["A"], int(h))
    return (tb["Pinf"] - Ah @ (tb["Pinf"] - tb["PF"]) @ Ah.T)[0, 0]


# ------------------------------------------------------------------------------------------------ fixed-lag smoother
def forward_np(tbs, Ty, x_in=None, state_at=None):
    """The smoother's forward pass, vectorised over latents: p, v [L][T] and the filtered state after tick state_at - 1 (default T; 0: x_in)."""
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs])
    L, T = Ty.shape
    x = np.zeros((L, A.shape[1])) if x_in is None else np.array(x_in, dtype=np.float64)
    state_at = T if state_at is None else state_at
    p = np.zeros((L, T)); v = np.zeros((L, T)); xs = x.copy()
    for t in range(T):
        xp = np.einsum("lij,lj->li", A, x)
        p[:, t] = xp[:, 0]
        y = Ty[:, t]
        v[:, t] = np.where(np.isnan(y), 0.0, y - p[:, t])
        x = xp + K * v[:, t:t + 1]
        if t + 1 == state_at:
            xs = x.copy()
    return p, v, xs


_WCACHE = {}


def _window_gain(tb, l):
    key = (tb["G"].tobytes(), tb["K"].tobytes(), int(l))
    if key not in _WCACHE:
        _WCACHE[key] = np.linalg.matrix_power(tb["G"], int(l) + 1) @ tb["K"]
    return _WCACHE[key]


def lagged_np(tbs, Ty, lags, x_in=None, state_at=None):
    """The fixed-lag mean by the backward recursion s_k[t] = G s_k[t+1] + K v[t] - G^(l_k+1) K v[t+l_k+1], vectorised over lags and latents.
    Returns (lag [K][L][T], p [L][T], the filtered state after tick state_at - 1)."""
    p, v, xs = forward_np(tbs, Ty, x_in, state_at)
    L, T = Ty.shape
    G = np.stack([t["G"] for t in tbs]); K = np.stack([t["K"] for t in tbs])
    W = np.array([[_window_gain(t, l) for t in tbs] for l in lags])                    # [K][L][d]
    nk = len(lags)
    s = np.zeros((nk, L, G.shape[1])); out = np.zeros((nk, L, T)); vs = np.zeros((nk, L))
    for t in range(T - 1, -1, -1):
        for k, l in enumerate(lags):
            vs[k] = v[:, t + l + 1] if t + l + 1 < T else 0.0
        s = np.einsum("lij,klj->kli", G, s) + K[None] * v[None, :, t, None] - W * vs[:, :, None]
        out[:, :, t] = p[None, :, t] + s[:, :, 0]
    return out, p, xs


def lagged_var_np(tb, l):
    Gl = np.linalg.matrix_power(tb["G"], int(l))
    return (tb["Ps"] + Gl @ (tb["PF"] - tb["Ps"]) @ Gl.T)[0, 0]


# ------------------------------------------------------------------------------------------------ off-grid smoother
def F_of(kern, dt, prm):
    g = IHGP(dt, kern)
    g.update(np.asarray(prm, dtype=np.float64))
    return np.array(g.ss.F, dtype=np.float64)


def interp_rows_np(tb, F, dt, phi):
    """(a_phi, g_phi, var) of one latent and one offset, from the definition."""
    Ap, Bp = sl.expm(F * (phi * dt)), sl.expm(F * ((1.0 - phi) * dt))
    Pp = Ap @ tb["PF"] @ Ap.T + tb["Pinf"] - Ap @ tb["Pinf"] @ Ap.T
    Gp = Pp @ Bp.T @ np.linalg.inv(tb["P"])
    return Ap[0], Gp[0], (Pp + Gp @ (tb["Ps"] - tb["P"]) @ Gp.T)[0, 0]


def interp_np(tbs, F_list, dt, fracs, Ty, x_in=None):
    """fine[k][l][t] = a_k . xf[t] + g_k . s[t+1] with the smoother's two passes, vectorised over latents.
    Returns (fine [K][L][T], ys [L][T], the end state [L][d], var [K][L])."""
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs]); G = np.stack([t["G"] for t in tbs])
    L, T = Ty.shape
    d = A.shape[1]
    rows = [[interp_rows_np(tb, F, dt, phi) for tb, F in zip(tbs, F_list)] for phi in fracs]
    a = np.array([[r[0] for r in rk] for rk in rows]); g = np.array([[r[1] for r in rk] for rk in rows])     # [K][L][d]
    var = np.array([[r[2] for r in rk] for rk in rows])
    x = np.zeros((L, d)) if x_in is None else np.array(x_in, dtype=np.float64)
    p = np.zeros((L, T)); v = np.zeros((L, T)); xf = np.zeros((L, T, d))
    for t in range(T):
        xp = np.einsum("lij,lj->li", A, x)
        p[:, t] = xp[:, 0]
        y = Ty[:, t]
        v[:, t] = np.where(np.isnan(y), 0.0, y - p[:, t])
        x = xp + K * v[:, t:t + 1]
        xf[:, t] = x
    s = np.zeros((L, d)); ys = np.zeros((L, T)); fine = np.zeros((len(fracs), L, T))
    for t in range(T - 1, -1, -1):
        fine[:, :, t] = np.einsum("kld,ld->kl", a, xf[:, t]) + np.einsum("kld,ld->kl", g, s)
        s = np.einsum("lij,lj->li", G, s) + K * v[:, t:t + 1]
        ys[:, t] = p[:, t] + s[:, 0]
    return fine, ys, x, var


# ------------------------------------------------------------------------------------------------ slopes
def slope_rows_np(tb, F, dt, phi, given="all"):
    """(a, gd, var) of one latent and one offset, from the definition."""
    Ap, Bp = sl.expm(F * (phi * dt)), sl.expm(F * ((1.0 - phi) * dt))
    Pinf, P = tb["Pinf"], tb["P"]
    Pp = Ap @ tb["PF"] @ Ap.T + Pinf - Ap @ Pinf @ Ap.T
    if given == "past":
        return Ap[1], np.zeros(F.shape[0]), Pp[1, 1]
    gd = ((F @ (Pp - Pinf) - Pinf @ F.T) @ Bp.T @ np.linalg.inv(P))[0]
    return Ap[1], gd, Pp[1, 1] + gd @ (tb["Ps"] - P) @ gd


def sweeps_np(tbs, a, g, Ty, x_in=None, emulate32=False):
    """plane[k][l][t] = a[k][l] . xf[t] + g[k][l] . s[t+1] with the smoother's two passes, vectorised over latents; returns (planes, ys, end state).
    emulate32: p, v, the planes between the two passes and the results are rounded to fp32 where the kernels stage an fp32 stream (the forward
    pass itself keeps v in fp64; the data are taken to be fp32 numbers already)."""
    r32 = (lambda z: np.asarray(z, dtype=np.float32).astype(np.float64)) if emulate32 else (lambda z: z)
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs]); G = np.stack([t["G"] for t in tbs])
    L, T = Ty.shape
    d = A.shape[1]
    x = np.zeros((L, d)) if x_in is None else np.array(x_in, dtype=np.float64)
    p = np.zeros((L, T)); q = np.zeros((a.shape[0], L, T))
    for t in range(T):
        xp = np.einsum("lij,lj->li", A, x)
        p[:, t] = xp[:, 0]
        y = Ty[:, t]
        x = xp + K * np.where(np.isnan(y), 0.0, y - p[:, t])[:, None]
        q[:, :, t] = np.einsum("kld,ld->kl", a, x)
    p, q = r32(p), r32(q)
    v = r32(np.where(np.isnan(Ty), 0.0, Ty - p))
    s = np.zeros((L, d)); ys = np.zeros((L, T))
    for t in range(T - 1, -1, -1):
        q[:, :, t] += np.einsum("kld,ld->kl", g, s)
        s = np.einsum("lij,lj->li", G, s) + K * v[:, t:t + 1]
        ys[:, t] = r32(p[:, t] + r32(s[:, 0]))
    return r32(q), ys, r32(x)


def slope_np(tbs, F_list, dt, fracs, Ty, x_in=None, given="all", emulate32=False):
    """Returns (slope [K][L][T], ys [L][T], the end state [L][d], var [K][L])."""
    rows = [[slope_rows_np(tb, F, dt, phi, given) for tb, F in zip(tbs, F_list)] for phi in fracs]
    a = np.array([[r[0] for r in rk] for rk in rows]); g = np.array([[r[1] for r in rk] for rk in rows])     # [K][L][d]
    planes, ys, x = sweeps_np(tbs, a, g, Ty, x_in, emulate32)
    return planes, ys, x, np.array([[r[2] for r in rk] for rk in rows])


# ------------------------------------------------------------------------------------------------ sampler: the generator
def philox4x32_10(ctr, key):
    """Random123's Philox4x32-10: ctr [..., 4], key [..., 2] (uint32) -> [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def _pair_normals(a, b):
    """The header's word pair -> two normals: u1, u2 and the angle in fp32 as on the device, the functions in fp64 (the reference)."""
    f = np.float32
    u1 = ((a >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    u2 = ((b >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    rho = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = (f(6.283185307179586) * u2).astype(np.float64)
    return rho * np.cos(ang), rho * np.sin(ang)


def normals4(seed, q, latent, sample, tag):
    """[..., 4] normals of the counters (q, latent, sample, tag) (broadcast), key = the seed's two words."""
    q, latent, sample, tag = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in (q, latent, sample, tag)])
    ctr = np.stack([q, latent, sample, tag], axis=-1) & np.uint64(0xFFFFFFFF)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), ctr.shape[:-1] + (2,))
    w = philox4x32_10(ctr, key)
    n0, n1 = _pair_normals(w[..., 0], w[..., 1])
    n2, n3 = _pair_normals(w[..., 2], w[..., 3])
    return np.stack([n0, n1, n2, n3], axis=-1)


def noise_np(seed, latent0, L, sample0, S, T):
    """(noise [S, L, T], start [S, L, 4]) of moihgp_sample_noise."""
    s = sample0 + np.arange(S)[:, None, None]
    l = latent0 + np.arange(L)[None, :, None]
    nq = (T + 3) // 4
    noise = normals4(seed, np.arange(nq)[None, None, :], l, s, 0).reshape(S, L, 4 * nq)[:, :, :T]
    return noise, normals4(seed, 0, l[:, :, 0], s[:, :, 0], 1)


# ------------------------------------------------------------------------------------------------ sampler: the realization
def realization(G, Ps, nfix=64, nnewton=8):
    """Sigma with sigma^2 = r0 - Sigma_00, B = G (N - Sigma h) / sigma^2, Sigma = G Sigma G^T + sigma^2 B B^T: 64 steps of the iteration from zero,
    then up to 8 Newton steps dSigma - Ac dSigma Ac^T = F(Sigma), Ac = G - B h^T; and the header's acceptance figure."""
    d = G.shape[0]
    N, r0 = Ps[:, 0].copy(), Ps[0, 0]
    Sg = np.zeros((d, d))

    def parts(Sg):
        s2 = r0 - Sg[0, 0]
        B = G @ (N - Sg[:, 0]) / s2
        F = G @ Sg @ G.T + s2 * np.outer(B, B) - Sg
        return s2, B, (F + F.T) / 2

    with np.errstate(all="ignore"):
        for _ in range(nfix):
            Sg = Sg + parts(Sg)[2]
        for _ in range(nnewton):
            s2, B, F = parts(Sg)
            m = np.max(np.abs(Sg))
            if not np.isfinite(m) or not np.max(np.abs(F)) > 1e-15 * m:      # relative to max |Sigma|, not r0
                break
            Ac = G.copy(); Ac[:, 0] -= B
            try:
                dS = np.linalg.solve(np.eye(d * d) - np.kron(Ac, Ac), F.ravel()).reshape(d, d)
            except np.linalg.LinAlgError:
                break
            if not np.all(np.isfinite(dS)):
                break
            Sg = Sg + (dS + dS.T) / 2
        s2, B, _ = parts(Sg)
        r, rh = acov(G, N, 64), acov_hat(G, Sg, s2, B, 64)
        err = float(np.max(np.abs(rh - r)) / r0)
    ok = np.isfinite(err) and err <= 1e-9 and s2 > 0 and np.all(np.isfinite(Sg)) and np.all(np.isfinite(B))
    return dict(B=B, sigma2=float(s2), Sigma=Sg, Lc=chol_zero(Sg), err=err, status=0 if ok else 2)


def acov(G, N, n):
    """r[k] = H G^k Ps H^T, k < n."""
    out, v = np.zeros(n), N.copy()
    for k in range(n):
        out[k] = v[0]; v = G @ v
    return out


def acov_hat(G, Sg, s2, B, n):
    """r^[0] = Sigma_00 + sigma^2, r^[k] = (G^(k-1) (G Sigma h + sigma^2 B))_0."""
    out, w = np.zeros(n), G @ Sg[:, 0] + s2 * B
    out[0] = Sg[0, 0] + s2
    for k in range(1, n):
        out[k] = w[0]; w = G @ w
    return out


def chol_zero(S):
    """Lower Cholesky factor of sym(S); a pivot <= 0 gives a zero column."""
    d = S.shape[0]
    S, Lc = (S + S.T) / 2, np.zeros((d, d))
    for j in range(d):
        p = S[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not p > 0:
            continue
        Lc[j, j] = np.sqrt(p)
        for i in range(j + 1, d):
            Lc[i, j] = (S[i, j] - Lc[i, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def deviations_np(G, B, sigma, Lc, noise, start):
    """o [S, L, T] of the header's backward recursion: G [L, d, d], B [L, d], sigma [L], Lc [L, d, d], noise [S, L, T], start [S, L, 4]."""
    S, L, T = noise.shape
    d = G.shape[1]
    u = np.einsum("lij,slj->sli", Lc, start[:, :, :d])
    o = np.zeros((S, L, T))
    for t in range(T - 1, -1, -1):
        e = sigma[None, :] * noise[:, :, t]
        o[:, :, t] = u[:, :, 0] + e
        u = np.einsum("lij,slj->sli", G, u) + B[None] * e[:, :, None]
    return o


# ------------------------------------------------------------------------------------------------ OILMM projection
def project_np(gp, Y, nan_below_L=False):
    """The projection of the observations Y [T][M] of a full model to its latents' streams: per tick the least-squares solve on the observed
    outputs, scaled by 1 / sqrt(S).  With nan_below_L a tick with fewer than L outputs observed is a missing tick (NaN) of every latent.
    Returns (U [M][L], S [L], the latents' parameters [L][3], Ty [L][T])."""
    M, L = gp.num_output, gp.num_latent
    prm = gp.params
    U, S = prm[:M * L].reshape(M, L), prm[M * L:M * L + L]
    igp = prm[-3 * L:].reshape(L, 3)
    Ty = np.zeros((L, Y.shape[0]))
    for t, y in enumerate(Y):
        obs = ~np.isnan(y)
        if nan_below_L and obs.sum() < L:
            Ty[:, t] = np.nan
            continue
        U0 = U[obs]
        Ty[:, t] = np.linalg.solve(U0.T @ U0, U0.T @ y[obs]) / np.sqrt(S)
    return U, S, igp, Ty


def smooth_outputs_np(gp, Y, kern):
    """smooth_outputs in numpy: the smoothed outputs [M][T] and their variances [M]."""
    U, S, igp, Ty = project_np(gp, Y)
    tbs = [tables(kern, 0.1, igp[l]) for l in range(len(igp))]
    ys, _ = smooth_np(tbs, Ty)
    return (U * np.sqrt(S)) @ ys, (U ** 2) @ (S * np.array([t["var_s"] for t in tbs]))
