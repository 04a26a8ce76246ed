"""The numpy definition of exact smoothing across missing ticks (include/moihgp.h moihgp_posterior_stream): the time-varying Kalman filter from the
model's own prior N(0, Pinf) and the RTS backward pass, with no update at a NaN tick; and the dense GP posterior and log likelihood over the
observed ticks it is held against.  CPU only (numpy and stream_reference).  The d x d algebra is written out (einsum and an elimination with
partial pivoting, no LAPACK), vectorised over the latents, so that the same lines evaluate in np.float64 and in np.longdouble: the second is
the yardstick for the rounding error of the first."""
import numpy as np

from stream_reference import model


def model_tables(kern, dt, prm):
    """What the definition needs of one parameter draw: dict(A, Pinf, R) -- no DARE.  Q is part of the definition (posterior_np forms it)."""
    A, _, R, Pinf = model(kern, dt, prm)
    return dict(A=A, Pinf=Pinf, R=R)


def _sym(X):
    return (X + np.swapaxes(X, -1, -2)) / 2


def _mm(A, B):
    return np.einsum("lij,ljk->lik", A, B)


def _mv(A, x):
    return np.einsum("lij,lj->li", A, x)


def _solve(A, B):
    """A^-1 B per latent ([L][d][d] both) by Gaussian elimination with partial pivoting (the first largest entry), in the dtype of A."""
    A = A.copy(); B = B.copy()
    L, n, _ = A.shape
    idx = np.arange(L)
    for k in range(n):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        for M in (A, B):
            rk, rp = M[idx, k].copy(), M[idx, p].copy()
            M[idx, k], M[idx, p] = rp, rk
        for i in range(k + 1, n):
            f = A[:, i, k] / A[:, k, k]
            A[:, i, k:] = A[:, i, k:] - f[:, None] * A[:, k, k:]
            B[:, i] = B[:, i] - f[:, None] * B[:, k]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        s = B[:, i].copy()
        for k in range(i + 1, n):
            s = s - A[:, i, k, None] * X[:, k]
        X[:, i] = s / A[:, i, i, None]
    return X


def posterior_np(tbs, Ty, dtype=np.float64):
    """The definition, for the rows of Ty [L][T] (NaN = missing tick) and one dict(A, Pinf, R) per row.  Returns dict(mean [L][T], var [L][T],
    x [L][d], P_end [L][d][d], nll [L], status [L]) in `dtype`; a latent whose recursion breaks down (S <= 0 at an observed tick, or anything not
    finite) has status 5 and NaN everywhere."""
    Ty = np.asarray(Ty, dtype=np.float64)
    L, T = Ty.shape
    A = np.stack([np.asarray(t["A"], dtype=dtype) for t in tbs])
    Pinf = np.stack([np.asarray(t["Pinf"], dtype=dtype) for t in tbs])
    R = np.array([t["R"] for t in tbs], dtype=dtype)
    d = A.shape[1]
    AT = np.swapaxes(A, 1, 2)
    two_pi = dtype(2.0) * (np.pi if dtype is np.float64 else 4 * np.arctan(dtype(1.0)))
    half = dtype(0.5)
    with np.errstate(all="ignore"):
        Q = _sym(Pinf - _mm(_mm(A, Pinf), AT))
        xf = np.zeros((T, L, d), dtype=dtype); PF = np.zeros((T, L, d, d), dtype=dtype)
        nll = np.zeros(L, dtype=dtype); bad = np.zeros(L, dtype=bool)
        x, Pf = np.zeros((L, d), dtype=dtype), Pinf.copy()
        for t in range(T):
            if t == 0:
                xp, P = np.zeros((L, d), dtype=dtype), Pinf.copy()
            else:
                xp, P = _mv(A, x), _sym(_mm(_mm(A, Pf), AT) + Q)
            y = Ty[:, t].astype(dtype)
            obs = ~np.isnan(y)
            S = P[:, 0, 0] + R
            v = y - xp[:, 0]
            K = P[:, :, 0] / S[:, None]
            U = _sym(P - K[:, :, None] * P[:, None, 0, :])
            x = np.where(obs[:, None], xp + K * v[:, None], xp)
            Pf = np.where(obs[:, None, None], U, P)
            nll = nll + np.where(obs, half * (np.log(two_pi * S) + v * v / S), dtype(0.0))
            bad |= (obs & ~(S > 0)) | ~np.all(np.isfinite(x), axis=1) | ~np.all(np.isfinite(Pf), axis=(1, 2)) | ~np.isfinite(nll)
            xf[t], PF[t] = x, Pf
        mean = np.zeros((L, T), dtype=dtype); var = np.zeros((L, T), dtype=dtype)
        xs, Ps = x, Pf
        for t in range(T - 1, -1, -1):
            if t < T - 1:
                xpn, Pn = _mv(A, xf[t]), _sym(_mm(_mm(A, PF[t]), AT) + Q)
                GT = _solve(Pn, _mm(A, PF[t]))                     # G^T = P[t+1]^-1 A PF[t]
                G = np.swapaxes(GT, 1, 2)
                xs = xf[t] + _mv(G, xs - xpn)
                Ps = _sym(PF[t] + _mm(_mm(G, Ps - Pn), GT))
            bad |= ~np.all(np.isfinite(xs), axis=1) | ~np.all(np.isfinite(Ps), axis=(1, 2))
            mean[:, t], var[:, t] = xs[:, 0], Ps[:, 0, 0]
        bad |= ~np.all(np.isfinite(x), axis=1) | ~np.all(np.isfinite(Pf), axis=(1, 2))
    x, Pf = x.copy(), Pf.copy()
    for a in (mean, var, x, Pf, nll):
        a[bad] = np.nan
    return dict(mean=mean, var=var, x=x, P_end=Pf, nll=nll, status=np.where(bad, 5, 0).astype(np.int32), Q=Q)


def covariances(tb, n):
    """c[k] = (A^k Pinf)_00, k < n: the model's covariance function on the grid."""
    A, Pinf = tb["A"], tb["Pinf"]
    c = np.zeros(n); M = np.eye(A.shape[0])
    for k in range(n):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    return c


def dense_posterior_np(tb, y, ahead=1):
    """The dense GP posterior given the observed ticks of y [T] (NaN = missing): (mean [T + ahead], var [T + ahead]) of the latent function at
    every tick and at `ahead` ticks past the end.  No observed tick: the prior."""
    T = len(y)
    c = covariances(tb, T + ahead)
    i = np.arange(T + ahead)
    Cm = c[np.abs(i[:, None] - i[None, :])]
    o = np.flatnonzero(~np.isnan(y))
    if len(o) == 0:
        return np.zeros(T + ahead), np.diag(Cm).copy()
    Kd = Cm[np.ix_(o, o)] + tb["R"] * np.eye(len(o))
    Cao = Cm[:, o]
    return Cao @ np.linalg.solve(Kd, y[o]), np.diag(Cm - Cao @ np.linalg.solve(Kd, Cao.T))


def dense_nll_np(tb, y):
    """-log N(y_obs; 0, C_oo + R I)."""
    o = np.flatnonzero(~np.isnan(y))
    if len(o) == 0:
        return 0.0
    c = covariances(tb, len(y))
    Kd = c[np.abs(o[:, None] - o[None, :])] + tb["R"] * np.eye(len(o))
    _, logdet = np.linalg.slogdet(Kd)
    return 0.5 * (y[o] @ np.linalg.solve(Kd, y[o]) + logdet + len(o) * np.log(2 * np.pi))
