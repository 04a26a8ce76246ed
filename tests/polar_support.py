"""Cases, references and the bar of tests/test_polar_factor.py, shared with its child process tests/polar_child.py: NumPy only, so that the
figures of the module's docstring can be measured without a device (`python tests/polar_support.py` prints them).

Every matrix is A = Q1 diag(sigma) Q2^T with Q1 (M x L) and Q2 (L x L) from QR of seeded normal draws and sigma = 1 + 3e-11 randn except for
the planted values.  Two references: LAPACK's svdU svdV^T of A (the one the device is held to) and the constructed Q1 Q2^T.  Errors are
max-abs over the conditioning scale of the polar factor, s(A) = eps ||A||_F / sigma_min(A)."""
import numpy as np

from parity_support import synth_params

EPS = 2.220446049250313e-16
LEARNER = [4.684, 1.2004, 1.081, 1.0364, 1.0213, 1.0125, 1.0075, 1.0036, 0.99947]      # test_gpu_parity's learner spectrum
PLANTED = {
    "learner": LEARNER,
    "one_small": [0.05],
    "mixed": [3.0, 0.2, 0.5, 1.7],
    "repeated": [2.0] * 5 + [0.5] * 5,
    "many": list(1.0 + np.logspace(0.5, -7, 40)),
    "near_sqrt3": [1.7320508, 1.74, 1.70],
    "gate_above": [1.001] * 3,
    "gate_below": [1.0003],
    "ill": [1e-4],
}
SPECTRA = list(PLANTED) + ["wide"]
# (M, L): one below the deflation's minimum 2 NB = 64; the minimum; lda % 4 = 1, 2, 3; either side of the 128-row block of the column
# reductions; past the 256-column block of the rank updates; tall, ending the 16- and 32-row tiles mid-tile
SHAPES = [(63, 63), (64, 64), (65, 65), (70, 66), (81, 67), (127, 127), (130, 129), (257, 257), (300, 258), (97, 65)]
ALL_SPECTRA_AT = [(70, 66), (130, 129)]
ILL_AT = (97, 65)
FAST = ("learner", "one_small", "mixed")       # at most 32 outliers, one of them >= 3 or <= 0.2: 0 < steps <= 3
TRACED_SHAPES = [(65, 65), (70, 66), (130, 129), (257, 257)]
TRACED_SPECTRA = ["learner", "mixed", "repeated"]
WARM_SHAPES = [(70, 66), (130, 129)]
# the bar, in units of s(A): four times the worst disagreement of the two references over every case of the module (0.70, measured on the
# CPU: test_polar_factor's docstring; test_polar_support.py recomputes it), floor 4; the factor 4 is for the summation order of the MFMA products and the two-stage reductions
REF_WORST = 0.70
BAR = max(4.0 * REF_WORST, 4.0)


def spectrum_cases():
    """(M, L, spectrum) of every constructed case of the module."""
    cases = [(M, L, "learner") for M, L in SHAPES]
    for M, L in ALL_SPECTRA_AT:
        cases += [(M, L, s) for s in SPECTRA if s not in ("learner", "ill")]
    return cases + [ILL_AT + ("ill",)]


class Case(object):
    """A, the parameter vector update() is handed, both references, the scale and the bar (absolute)."""

    def __init__(self, M, L, spectrum, seed=0, A=None, old_rel=1e-10):
        rng = np.random.default_rng([M, L, SPECTRA.index(spectrum) if spectrum in SPECTRA else 99, seed])
        self.M, self.L, self.spectrum = M, L, spectrum
        self.n_planted = len(PLANTED.get(spectrum, []))
        if A is None:
            Q1, _ = np.linalg.qr(rng.standard_normal((M, L)))
            B2 = rng.standard_normal((L, L))
            if spectrum.startswith("gate"):
                # the gate of polar_factor_device is on max_ij |G - I|_ij: the planted directions are coordinate axes, so that it sees
                # sigma^2 - 1 itself (2.0e-3 / 6.0e-4) and not that figure times the squared entries of a random vector
                B2[:, :3] = np.eye(L, 3)
            Q2, _ = np.linalg.qr(B2)
            sig = np.ones(L) + 3e-11 * rng.standard_normal(L)
            if spectrum == "wide":
                sig = rng.uniform(0.5, 1.5, L)
            else:
                sig[:self.n_planted] = PLANTED[spectrum]
            self.Q1, self.Q2, self.sig = Q1, Q2, sig
            A = (Q1 * sig) @ Q2.T
            self.ref_q = Q1 @ Q2.T
        else:
            self.ref_q = None
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.params = np.concatenate([self.A.ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])
        u, sv, vt = np.linalg.svd(self.A, full_matrices=False)
        self.ref = u @ vt
        self.scale = EPS * np.linalg.norm(self.A) / sv.min()
        # never looser than the flat bars of test_gpu_parity (relative to max|ref|: 1e-10 on planted spectra, 1e-11 on eye + noise)
        self.bar = min(BAR * self.scale, old_rel * np.max(np.abs(self.ref)))

    def with_A(self, A):
        """The same shape and tail of the parameter vector around another matrix (warm-start sequences)."""
        c = Case(self.M, self.L, self.spectrum, A=A)
        c.params = np.concatenate([c.A.ravel(), self.params[self.M * self.L:]])
        c.n_planted = self.n_planted
        return c

    def judge(self, U):
        """(max-abs error over s(A), max-abs error, max|U^T U - I|)"""
        U = np.asarray(U, dtype=np.float64).reshape(self.M, self.L)
        err = float(np.max(np.abs(U - self.ref)))
        return err / self.scale, err, float(np.max(np.abs(U.T @ U - np.eye(self.L))))

    def ref_ratio(self):
        return float(np.max(np.abs(self.ref - self.ref_q))) / self.scale


def noisy_case(M, L, noise):
    """eye + noise randn, as test_polar_factor_device_vs_svd draws it; held to its 1e-11 as well."""
    rng = np.random.default_rng(M + L)
    return Case(M, L, "eye+noise", A=np.eye(M, L) + noise * rng.standard_normal((M, L)), old_rel=1e-11)


def warm_sequence(M, L):
    """The warm-start sequence: [(label, Case)] -- A0 (cold), A1 = A0 + 0.02 rank one inside the outlying subspace (warm), B from another seed
    (the kept basis captures nothing: cold restart), B (warm), a near-orthonormal matrix (no attempt: the flag is reset), A1 (cold)."""
    c0 = Case(M, L, "learner")
    rng = np.random.default_rng([M, L, 7])
    k = c0.n_planted
    a, b = rng.standard_normal(k), rng.standard_normal(k)
    u, v = c0.Q1[:, :k] @ (a / np.linalg.norm(a)), c0.Q2[:, :k] @ (b / np.linalg.norm(b))
    c1 = c0.with_A(c0.A + 0.02 * np.outer(u, v))
    cb = Case(M, L, "learner", seed=1)
    cn = Case(M, L, "gate_below")
    return [("A0", c0), ("A1", c1), ("B", cb), ("B", cb), ("near", cn), ("A1", c1)]


def worst_ref_ratio():
    """The worst disagreement of the two references over every constructed case of the module, in units of s(A)."""
    cases = [Case(M, L, s) for M, L, s in spectrum_cases()] + [c for M, L in WARM_SHAPES for _, c in warm_sequence(M, L) if c.ref_q is not None]
    return max(c.ref_ratio() for c in cases)


if __name__ == "__main__":
    worst = 0.0
    for M, L, s in spectrum_cases():
        c = Case(M, L, s)
        r = c.ref_ratio(); worst = max(worst, r)
        print(f"({M}, {L}) {s:11s} refs disagree by {r:8.3g} s(A)   s(A) {c.scale:.2e}   bar {c.bar:.2e} = {c.bar / c.scale:.3g} s(A)")
    for M, L in WARM_SHAPES:
        for lab, c in warm_sequence(M, L):
            if c.ref_q is not None:
                worst = max(worst, c.ref_ratio())
            print(f"({M}, {L}) warm {lab:5s} s(A) {c.scale:.2e}   bar {c.bar:.2e} = {c.bar / c.scale:.3g} s(A)")
    print(f"worst disagreement of the two references: {worst:.3g} s(A)  ->  bar {max(4 * worst, 4.0):.3g} s(A)")
