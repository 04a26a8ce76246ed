"""The polar factor of update() (csrc/polar.hip, csrc/polar_deflate.hip) where test_gpu_parity's polar tests do not reach: an ACCEPTED
deflation at ragged sizes (lda % 4 != 0: the scalar remainder of ts_mm_kernel; partial last blocks of ts_gram / colstats (128 rows),
ts_rotate (8), ts_mm (16), rank_update / gram_update (256 columns, 32 rows)), the warm start the device-resident learner switches on, plain
Newton-Schulz on the same spectra (MOIHGP_POLAR_DEFLATE=0), degenerate / two-sided / too many / barely outlying / tiny singular values, the
device-resident entry, and the single-workgroup kernel at its limits.

Inputs and references: polar_support.py.  A = Q1 diag(sigma) Q2^T, held to LAPACK's svdU svdV^T in fp64; the constructed Q1 Q2^T is a second
reference.  Errors are max-abs over the conditioning scale s(A) = eps ||A||_F / sigma_min(A).

The bar.  On the CPU the two references disagree, in units of s(A) (python tests/polar_support.py):
    learner   (63,63) 0.70  (64,64) 0.53  (65,65) 0.55  (70,66) 0.54  (81,67) 0.56  (127,127) 0.30  (130,129) 0.36  (257,257) 0.20
              (300,258) 0.20  (97,65) 0.56
    (70,66)   one_small 0.031  mixed 0.13  repeated 0.41  many 0.49  near_sqrt3 0.50  gate_above 0.65  gate_below 0.65  wide 0.24
    (130,129) one_small 0.018  mixed 0.064 repeated 0.21  many 0.31  near_sqrt3 0.40  gate_above 0.39  gate_below 0.34  wide 0.19
    (97,65)   ill 0.0076
worst 0.70, times 4 (summation order of the MFMA products and of the two-stage reductions) = 2.8, below the floor: the bar is 4 s(A) --
8.2e-15 .. 1.5e-14 absolute on the learner spectrum, 1.4e-13 / 2.0e-13 at one_small -- and nowhere looser than test_gpu_parity's flat bars
(1e-10 max|U| on planted spectra, which binds at `ill` alone: 3.8e-11 = 2.1 s(A); 1e-11 max|U| on eye + noise).  max|U^T U - I| < 1e-12.

gate_above / gate_below: polar_factor_device attempts a deflation when max_ij |G - I|_ij > 1e-3, an ENTRY-wise figure: three directions at
sigma = 1.001 along random right singular vectors give 2e-3 times the squared entries of those vectors, 3e-4 at L = 66 -- no attempt.  The
planted directions of these two spectra are therefore coordinate axes (polar_support.Case), where the figure is sigma^2 - 1 itself: 2.0e-3
above the gate, 6.0e-4 below; the trace child checks that the first is attempted and the second is not.

What the device gave (MI355X), error in units of s(A) and Newton-Schulz steps with / without the deflation (MOIHGP_POLAR_DEFLATE=0):
    learner    0.22 .. 0.72 over the ten shapes, 1 step / 9 (at (63, 63), below the deflation's minimum, 9 either way)
    mixed      0.046 .. 0.14, 1 / 11 .. 12          repeated   0.12 .. 0.41, 1 / 8 .. 9          many        0.73 .. 1.4, 2 steps
    one_small  0.022 .. 0.047, 1 step                near_sqrt3 0.41 .. 0.45, 1 step               gate_above  0.37 .. 0.62, 1 / 3
    gate_below 0.34 .. 0.67, 3 / 3                   wide       0.17 .. 0.28, 8 / 8                ill         0.054 (9.6e-13), 2 / 28
    warm start 0.34 .. 1.3 over the seven updates at both shapes, option on or off; on against off 0 (cold updates) .. 0.86
    single-workgroup kernel and its neighbours: 0 .. 0.45, but 3.0 = 6.7e-16 at (1, 1) on the multi-kernel path (three ulps of 1)
    max|U^T U - I| <= 1.0e-14 everywhere
Before this module `ill` gave 1770 s(A) = 3.1e-8 with max|U^T U - I| = 5.2e-8, one_small 3.9 s(A) and 2.3e-13, mixed 1.2 s(A) and 3.1e-14:
the deflation updated the Gram matrix by its rank-32 formula with d_i from 1 + lambda_i = sigma_i^2, a cancelling difference for a small
sigma_i, so the deflated value was 1 + O(eps / sigma_i^2) while the formula's matrix said 1 and the iteration never saw it.  polar_deflate
now forms the Gram matrix from X again when a deflated sigma_i^2 is below 1/2 (the figures above are with that).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import polar_support as ps
from parity_support import env  # noqa: F401  (env: fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS_LINE = re.compile(r"polar: deflation pass (\d+)( \(warm start\))?  \|lambda\|max \S+  captured (\S+) of .*converged pairs (\d+)")


def _install(gp, case):
    gp.update(case.params)
    return gp.params[:case.M * case.L].copy()


def _check(case, U, what):
    ratio, err, ortho = case.judge(U)
    print(f"{what}: error {ratio:.3g} s(A) = {err:.2e} (bar {case.bar:.2e}), max|U^T U - I| {ortho:.1e}")
    assert ortho < 1e-12, (what, ortho)
    assert err <= case.bar, (what, f"{ratio:.3g} s(A)", err, case.bar)
    return ratio


# ---------------------------------------------------------------------------------------------- the multi-kernel path, in this process
@pytest.mark.parametrize("M,L,spectrum", ps.spectrum_cases())
def test_planted_spectra_at_ragged_sizes(env, M, L, spectrum, monkeypatch):
    monkeypatch.setenv("MOIHGP_POLAR", "gemm")
    case = ps.Case(M, L, spectrum)
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    U = _install(gp, case)
    its = env["lib"].moihgp_polar_iterations(gp.handle)
    _check(case, U, f"{spectrum} ({M}, {L}), {its} steps")
    if spectrum in ps.FAST and L >= 64:                 # (below 2 NB = 64 columns no deflation is attempted: plain Newton-Schulz, nine steps)
        assert 0 < its <= 3, its
    assert its > 0


# ---------------------------------------------------------------------------------------------- the two child processes
def _child(**extra):
    e = dict(os.environ)
    e.pop("MOIHGP_POLAR_TRACE", None); e.pop("MOIHGP_POLAR_DEFLATE", None)
    e.update(MOIHGP_POLAR="gemm", **extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "polar_child.py")], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rec = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln); rec[d["key"]] = d
    passes, key = {}, None                        # key -> [(pass number, warm, captured share of ||E||_F^2, converged pairs)]
    for ln in r.stderr.splitlines():
        if ln.startswith("case "):
            key = ln[5:].strip()
            if key != "-":                        # ("-": a constructor's own polar factor)
                passes[key] = []
        m = PASS_LINE.search(ln)
        if m and key != "-":
            passes[key].append((int(m.group(1)), bool(m.group(2)), float(m.group(3)), int(m.group(4))))
    assert set(rec) == set(passes) and len(rec) == 12 + 6 + 1 + 2 * 7, sorted(rec)
    return rec, passes


@pytest.fixture(scope="module")
def traced(env):
    """(records, deflation passes per update) of the child with MOIHGP_POLAR_TRACE=1, the documented diagnostic."""
    return _child(MOIHGP_POLAR_TRACE="1")


@pytest.fixture(scope="module")
def plain(env):
    """The same with MOIHGP_POLAR_DEFLATE=0: plain Newton-Schulz (and no trace, so no passes)."""
    return _child(MOIHGP_POLAR_DEFLATE="0")


def _check_records(rec):
    for key, d in rec.items():
        print(f"{key}: error {d['ratio']:.3g} s(A) = {d['err']:.2e} (bar {d['bar']:.2e}), max|U^T U - I| {d['ortho']:.1e}, {d['its']} steps")
    for key, d in rec.items():
        assert d["ortho"] < 1e-12 and d["err"] <= d["bar"], (key, d)


def test_deflation_is_accepted_not_skipped(traced):
    """A deflation kernel that merely keeps pairs from converging leaves U right, in more steps: here every planted outlier has to be among
    the converged pairs of the last pass, with >= 90 % of ||E||_F^2 captured."""
    rec, passes = traced
    _check_records(rec)
    for M, L in ps.TRACED_SHAPES:
        for s in ps.TRACED_SPECTRA:
            key = f"{s}/{M}x{L}"
            assert passes[key], key
            _, warm, captured, pairs = passes[key][-1]
            assert not warm and pairs >= len(ps.PLANTED[s]) and captured >= 0.9, (key, passes[key])
            if s in ps.FAST:
                assert 0 < rec[key]["its"] <= 3, (key, rec[key])


def test_wide_spectrum_is_abandoned_and_the_gate_holds(traced):
    _, passes = traced
    for M, L in ps.ALL_SPECTRA_AT:
        wide = passes[f"wide/{M}x{L}"]
        assert [p[0] for p in wide] == [1, 2] and wide[-1][3] == 0 and wide[-1][2] < 0.9, wide     # abandoned at pass 2, no pairs
        assert passes[f"gate_above/{M}x{L}"], "max|G - I| = 2e-3: a deflation is attempted"
        assert passes[f"gate_below/{M}x{L}"] == [], "max|G - I| = 6e-4: none is"


def test_warm_start_trace(traced):
    """Option on: A0 cold, A1 warm, B starts warm on a basis that captures nothing and restarts cold, B warm, a near-orthonormal matrix
    attempts nothing and resets the flag, so A1 runs cold; moihgp_set_option resets it too, so the A1 after it runs cold as well."""
    _, passes = traced
    for M, L in ps.WARM_SHAPES:
        seq = [passes[k] for k in sorted(k for k in passes if k.startswith("warm") and k.endswith(f"/{M}x{L}"))]
        assert len(seq) == 7
        warm = [[p[1] for p in s] for s in seq]
        assert warm[0] and not any(warm[0]), warm[0]
        assert warm[1] and all(warm[1]), warm[1]
        assert len(warm[2]) >= 3 and warm[2][0] and not any(warm[2][1:]), warm[2]
        assert seq[2][0][2] < 0.9 and seq[2][1][0] == 1, seq[2]                 # the warm pass captured too little; pass 1 again, cold
        assert warm[3] and all(warm[3]), warm[3]
        assert seq[4] == [], seq[4]
        assert warm[5] and not any(warm[5]), warm[5]
        assert warm[6] and not any(warm[6]), warm[6]
        for k in (0, 1, 2, 3, 5, 6):                                            # and every one of them ends on an accepted deflation
            assert seq[k][-1][3] >= 9 and seq[k][-1][2] >= 0.9, (k, seq[k])


def test_plain_newton_schulz_on_the_same_spectra(plain, traced):
    """Without the deflation: the same factor to the same bar, in strictly more steps on the learner's spectrum."""
    rec, passes = plain
    _check_records(rec)
    assert all(p == [] for p in passes.values())
    for M, L in ps.TRACED_SHAPES:
        key = f"learner/{M}x{L}"
        print(f"{key}: {traced[0][key]['its']} steps with the deflation, {rec[key]['its']} without")
        assert rec[key]["its"] > traced[0][key]["its"] > 0, (key, rec[key]["its"], traced[0][key]["its"])


# ---------------------------------------------------------------------------------------------- warm start, in this process
@pytest.mark.parametrize("M,L", ps.WARM_SHAPES)
def test_warm_start_sequence_against_each_steps_own_factor(env, M, L, monkeypatch):
    monkeypatch.setenv("MOIHGP_POLAR", "gemm")
    lib, seq = env["lib"], ps.warm_sequence(M, L)
    on, off = env["MOIHGP"](0.1, M, L, kernel="Matern32"), env["MOIHGP"](0.1, M, L, kernel="Matern32")
    assert lib.moihgp_set_option(on.handle, b"polar_warm_start", 1) == 0

    def step(k, label, case):
        U_on, U_off = _install(on, case), _install(off, case)
        _check(case, U_on, f"step {k} {label} ({M}, {L}) warm start on"); _check(case, U_off, f"step {k} {label} ({M}, {L}) off")
        diff = float(np.max(np.abs(U_on - U_off)))
        print(f"step {k} {label} ({M}, {L}): on against off {diff / case.scale:.3g} s(A)")
        assert diff <= case.bar, (k, label, diff, case.bar)             # the two agree to the bar (not to the bit: another start block)

    for k, (label, case) in enumerate(seq):
        step(k + 1, label, case)
    assert lib.moihgp_set_option(on.handle, b"polar_warm_start", 0) == 0 and lib.moihgp_set_option(on.handle, b"polar_warm_start", 1) == 0
    step(len(seq) + 1, *seq[-1])


@pytest.mark.parametrize("M,L", ps.WARM_SHAPES)
def test_without_warm_start_update_is_a_function_of_its_argument(env, M, L, monkeypatch):
    """Option off (the default): the same matrix gives the same bits whatever was installed before, on any handle of the shape
    ((130, 129): two blocks in the two-stage reductions, which therefore have to sum in a fixed order)."""
    monkeypatch.setenv("MOIHGP_POLAR", "gemm")
    a0, b = ps.Case(M, L, "learner"), ps.Case(M, L, "learner", seed=1)
    gp, gp2 = env["MOIHGP"](0.1, M, L, kernel="Matern32"), env["MOIHGP"](0.1, M, L, kernel="Matern32")
    U0 = _install(gp, a0); Ub = _install(gp, b); U1 = _install(gp, a0)
    assert not np.array_equal(U0, Ub)
    assert np.array_equal(U0, U1)
    assert np.array_equal(U0, _install(gp2, a0))


def test_update_dev_gives_the_bits_of_update(env, monkeypatch):
    """"same kernels, bit-identical values" for the device-resident entry."""
    monkeypatch.setenv("MOIHGP_POLAR", "gemm")
    M, L = 81, 67
    case = ps.Case(M, L, "learner")
    gp, gpd = env["MOIHGP"](0.1, M, L, kernel="Matern32"), env["MOIHGP"](0.1, M, L, kernel="Matern32")
    U = _install(gp, case)
    gpd.update_dev(torch.from_numpy(case.params).cuda())
    Ud = gpd.params[:M * L].copy()
    _check(case, Ud, f"update_dev ({M}, {L})")
    assert np.array_equal(U, Ud)
    out = gpd.params_dev(torch.empty(gpd.num_param, dtype=torch.float64, device="cuda"))
    assert np.array_equal(out.cpu().numpy(), gpd.params)
    assert env["lib"].moihgp_polar_iterations(gpd.handle) == env["lib"].moihgp_polar_iterations(gp.handle)


# ---------------------------------------------------------------------------------------------- the single-workgroup kernel at its limits
@pytest.mark.parametrize("mode", ["", "gemm"])
@pytest.mark.parametrize("M,L,noise", [(4096, 1, 1.0), (2048, 2, 1.0), (128, 32, 0.2),      # M L = 4096: the largest LDS request
                                       (4097, 1, 1.0), (129, 32, 0.2),                      # just over: the multi-kernel path, once with L = 1
                                       (33, 33, 0.4),                                       # L > 32: multi-kernel below one tile
                                       (1, 1, 0.4), (32, 32, 0.4),                          # the remaining corners
                                       (128, 32, None)])                                    # (None: the `mixed` spectrum)
def test_single_workgroup_kernel_at_its_limits(env, M, L, noise, mode, monkeypatch):
    monkeypatch.delenv("MOIHGP_POLAR", raising=False)
    if mode:
        monkeypatch.setenv("MOIHGP_POLAR", mode)
    case = ps.Case(M, L, "mixed") if noise is None else ps.noisy_case(M, L, noise)
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    U = _install(gp, case)
    its = env["lib"].moihgp_polar_iterations(gp.handle)
    _check(case, U, f"({M}, {L}) noise {noise} mode '{mode}', {its} steps")
    single = M * L <= 4096 and L <= 32 and not mode
    assert (its == 0) == single, (its, single)          # (moihgp_polar_iterations counts the multi-kernel path's steps only)
