"""The numpy definition of exact-edge smoothing (include/moihgp.h moihgp_smooth_stream_exact): the steady-state sweeps from a zero start state,
then the rank-d correction that swaps the prior N(0, P) the steady sweeps put on the first state for the model's N(0, Pinf), and the
time-varying smoothed covariance at the two ends.  CPU only (numpy and stream_reference).  The d x d algebra is written out (no LAPACK) so that
the same lines evaluate in np.float64 and in np.longdouble: the second is the yardstick for the rounding error of the first."""
import numpy as np

EDGE_CAP = 1 << 20          # head and tail are capped here; the cap means "never reached"
EDGE_EPS = 2.0 ** -60
SCRATCH_TICKS = 4096        # overlapping edges are walked up to this many ticks (status 3 beyond)


def _solve(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting, in the dtype of A."""
    A = A.copy(); B = B.copy()
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]; B[[k, p]] = B[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] = A[i, k:] - f * A[k, k:]
            B[i] = B[i] - f * B[k]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X


def edge_lengths_np(tb):
    """(head, tail): the smallest n with ||G^n||inf <= 2^-60 and the smallest k with ||G^k||inf^2 <= 2^-60, both capped at 2^20."""
    G = tb["G"]
    M = np.eye(G.shape[0])
    head = tail = EDGE_CAP
    for n in range(1, EDGE_CAP):
        M = G @ M
        nrm = float(np.max(np.sum(np.abs(M), axis=1)))
        if not np.isfinite(nrm):
            break
        if tail == EDGE_CAP and nrm * nrm <= EDGE_EPS:
            tail = n
        if nrm <= EDGE_EPS:
            head = n
            break
    return head, tail


_TERMS = {}


def edge_terms(tb, T, dtype=np.float64, full=False):
    """What the correction of one latent needs beside the sweeps, a function of its tables and T alone: R [T][d] the rows r_t (zero outside the
    head), Z [d][d], var [T], XE [d][d] = PF (G^T)^(T-1) (zero when tick T-1 lies outside the head), and (head, tail).  full: every tick by the
    formulas, no edge lengths."""
    key = (tb["G"].tobytes(), tb["P"].tobytes(), tb["Pinf"].tobytes(), int(T), np.dtype(dtype).name, bool(full))
    if key in _TERMS:
        return _TERMS[key]
    G, P, PF, Ps, Pinf = (np.asarray(tb[k], dtype=dtype) for k in ("G", "P", "PF", "Ps", "Pinf"))
    d = G.shape[0]
    I = np.eye(d, dtype=dtype)
    head, tail = edge_lengths_np(tb)
    n_tail = T if full else min(tail, T)            # ticks T - n_tail .. T - 1 take Ps_t from the recursion
    n_head = T if full else min(head, T)            # ticks 0 .. n_head - 1 take the correction
    rows = np.tile(Ps[0], (T, 1))
    Pst = PF.copy()
    for t in range(T - 1, T - 1 - n_tail, -1):
        if t < T - 1:
            Pst = PF + G @ (Pst - P) @ G.T
        rows[t] = Pst[0]
    Ps0 = Pst if n_tail == T else Ps
    E = _solve(Pinf, I) - _solve(P, I)
    Z = -_solve(I + E @ Ps0, E)
    R = np.zeros((T, d), dtype=dtype)
    var = rows[:, 0].copy()
    M = I.copy()                                     # (G^T)^t
    XE = np.zeros((d, d), dtype=dtype)
    for t in range(n_head):
        R[t] = rows[t] @ M
        var[t] = rows[t, 0] + R[t] @ Z @ R[t]
        if t == T - 1:
            XE = PF @ M
        M = M @ G.T
    out = dict(R=R, Z=Z, var=var, XE=XE, head=head, tail=tail)
    _TERMS[key] = out
    return out


def sweeps_zero_np(tbs, Ty):
    """The two steady-state sweeps from a zero start state, vectorised over latents: (ys [L][T], xf[T-1] [L][d], s[0] [L][d])."""
    A = np.stack([t["A"] for t in tbs]); K = np.stack([t["K"] for t in tbs]); G = np.stack([t["G"] for t in tbs])
    L, T = Ty.shape
    d = A.shape[1]
    x = np.zeros((L, d))
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
    return ys, x, s


def exact_np(tbs, Ty, dtype=np.float64, full=False):
    """The definition: returns dict(ys [L][T], var [L][T], x [L][d], status [L], head [L], tail [L], ys_steady, x_steady).  A latent whose edges
    overlap in a stream longer than 4096 ticks has status 3 and keeps the steady sweeps' row and end state and the steady variance."""
    L, T = Ty.shape
    ys0, x0, s0 = sweeps_zero_np(tbs, Ty)
    ys = ys0.astype(dtype); x = x0.astype(dtype); var = np.zeros((L, T), dtype=dtype)
    status = np.zeros(L, dtype=np.int32); head = np.zeros(L, dtype=np.int64); tail = np.zeros(L, dtype=np.int64)
    for l, tb in enumerate(tbs):
        head[l], tail[l] = edge_lengths_np(tb)
        if not full and head[l] + tail[l] > T and T > SCRATCH_TICKS:
            status[l] = 3
            var[l] = tb["var_s"]
            continue
        e = edge_terms(tb, T, dtype, full)
        c = e["Z"] @ s0[l].astype(dtype)
        ys[l] = ys[l] + e["R"] @ c
        var[l] = e["var"]
        x[l] = x[l] + e["XE"] @ c
    return dict(ys=ys, var=var, x=x, status=status, head=head, tail=tail, ys_steady=ys0, x_steady=x0)


def dense_posterior_np(tb, y, ahead=0):
    """The GP posterior of a gap-free stream: (mean [T], var [T] of the latent function, predictive mean of the `ahead` ticks past the end)."""
    A, Pinf, R = tb["A"], tb["Pinf"], tb["R"]
    T = len(y)
    c = np.zeros(T + ahead); M = np.eye(A.shape[0])
    for k in range(T + ahead):
        c[k] = (M @ Pinf)[0, 0]; M = A @ M
    i = np.arange(T)
    Cm = c[np.abs(i[:, None] - i[None, :])]
    Kd = Cm + R * np.eye(T)
    w = np.linalg.solve(Kd, y)
    Ca = c[np.abs((T + np.arange(ahead))[:, None] - i[None, :])]
    return Cm @ w, np.diag(Cm - Cm @ np.linalg.solve(Kd, Cm)), Ca @ w
