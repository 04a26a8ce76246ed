"""The numpy definition the seeded forecast paths of include/moihgp.h (moihgp_forecast_paths) are held to: the innovations recursion in its two
forms, the covariance across horizons from its taps, its noise, and the dense GP predictive covariance that vouches for it.  CPU only (numpy and
stream_reference); test modules import from here, never from each other."""
import numpy as np

from stream_reference import normals4

PATH_TAG = 2          # the paths' counter tag (0 and 1 are the sampler's)


def _start(start, S):
    start = np.asarray(start, dtype=np.float64)
    return np.broadcast_to(start, (S,) + start.shape).copy() if start.ndim == 2 else start.copy()


def paths_np(A, K, Sv, start, noise):
    """The header's recursion, vectorised over samples and latents: A [L, d, d], K [L, d], Sv [L], start [L, d] (shared by the samples) or
    [S, L, d], noise [S, L, n].  e = sqrt(Sv) n; u <- A u + K e; paths = u_0 + (1 - K_0) e.  Returns (paths [S, L, n], states [S, L, d])."""
    S, L, n = noise.shape
    u = _start(start, S)
    out = np.zeros((S, L, n))
    sd = np.sqrt(Sv)
    for j in range(n):
        e = sd[None, :] * noise[:, :, j]
        u = np.einsum("lij,slj->sli", A, u) + K[None] * e[:, :, None]
        out[:, :, j] = u[:, :, 0] + (1.0 - K[None, :, 0]) * e
    return out, u


def paths_filter_form_np(A, K, Sv, start, noise):
    """The same draws as "predict, add the innovation, update": xp = A u, y = xp_0 + e, u = xp + K (y - xp_0)."""
    S, L, n = noise.shape
    u = _start(start, S)
    out = np.zeros((S, L, n))
    sd = np.sqrt(Sv)
    for j in range(n):
        xp = np.einsum("lij,slj->sli", A, u)
        y = xp[:, :, 0] + sd[None, :] * noise[:, :, j]
        u = xp + K[None] * (y - xp[:, :, 0])[:, :, None]
        out[:, :, j] = y
    return out, u


def table_arrays(tbs):
    """(A [L, d, d], K [L, d], Sv [L]) of a list of stream_reference.tables dicts."""
    return np.stack([t["A"] for t in tbs]), np.stack([t["K"] for t in tbs]), np.array([t["S"] for t in tbs])


def path_taps_np(tb, n):
    """lam_0 = 1, lam_k = (A^k K)_0."""
    taps, v = np.ones(n), tb["K"].copy()
    for k in range(1, n):
        v = tb["A"] @ v
        taps[k] = v[0]
    return taps


def path_cov_np(tb, n):
    """C = Sv Lam Lam^T, Lam lower-triangular Toeplitz of the taps."""
    taps = path_taps_np(tb, n)
    i = np.arange(n)
    Lam = np.where(i[:, None] >= i[None, :], taps[np.abs(i[:, None] - i[None, :])], 0.0)
    return tb["S"] * (Lam @ Lam.T)


def tail_mean_np(tb, x, n):
    """H A^(j+1) x, j < n."""
    out, v = np.zeros(n), np.asarray(x, dtype=np.float64)
    for j in range(n):
        v = tb["A"] @ v
        out[j] = v[0]
    return out


def dense_predictive_cov(tb, T, n):
    """The GP predictive covariance of the observations y[T .. T+n) given y[0 .. T): the stationary kernel c[k] = (A^k Pinf)_00 plus R on the
    diagonal, conditioned densely."""
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    N = T + n
    c = np.zeros(N); M = np.eye(A.shape[0])
    for k in range(N):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    i = np.arange(N)
    Cy = c[np.abs(i[:, None] - i[None, :])] + R * np.eye(N)
    return Cy[T:, T:] - Cy[T:, :T] @ np.linalg.solve(Cy[:T, :T], Cy[:T, T:])


def paths_noise_np(seed, latent0, L, sample0, S, step0, n):
    """noise [S, L, n] of moihgp_forecast_paths_noise: the normal of step step0 + j is element (step0 + j) % 4 of the block (step0 + j) // 4."""
    s = sample0 + np.arange(S)[:, None, None]
    l = latent0 + np.arange(L)[None, :, None]
    q0, q1 = step0 // 4, (step0 + n + 3) // 4
    blocks = normals4(seed, np.arange(q0, q1)[None, None, :], l, s, PATH_TAG).reshape(S, L, 4 * (q1 - q0))
    return blocks[:, :, step0 - 4 * q0:step0 - 4 * q0 + n]
