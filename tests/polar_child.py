"""Run by tests/test_polar_factor.py in a process of its own, because csrc/polar.hip reads MOIHGP_POLAR_TRACE and MOIHGP_POLAR_DEFLATE once
per process: the parent starts it once with the trace on and once with the deflation off (MOIHGP_POLAR=gemm both times).  It installs the
planted spectra of polar_support through update(), then the warm-start sequence with the option "polar_warm_start" on, and prints one JSON
record per update to stdout: the error against LAPACK's factor on the scale s(A) and in absolute terms, the bar, max|U^T U - I| and the
Newton-Schulz steps.  Before every update it writes a line `case <key>` to stderr, so that the parent can cut the library's trace (which
goes there) into the updates it belongs to."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polar_support as ps  # noqa: E402


def main():
    import torch
    torch.cuda.set_device(0)
    from multioutputihgp_amd import MOIHGP, load_library
    lib = load_library()

    def new(M, L):
        mark("-")                       # (the constructor draws U = polar(I + N(0, 1e-3)): its trace belongs to no case)
        return MOIHGP(0.1, M, L, kernel="Matern32")

    def mark(key):
        sys.stderr.write(f"case {key}\n"); sys.stderr.flush()

    def run(gp, key, case):
        mark(key)
        gp.update(case.params)
        ratio, err, ortho = case.judge(gp.params[:case.M * case.L])
        print(json.dumps(dict(key=key, ratio=ratio, err=err, bar=case.bar, ortho=ortho, its=int(lib.moihgp_polar_iterations(gp.handle)))), flush=True)

    cases = [(M, L, s) for M, L in ps.TRACED_SHAPES for s in ps.TRACED_SPECTRA]
    cases += [(M, L, s) for M, L in ps.ALL_SPECTRA_AT for s in ("wide", "gate_above", "gate_below")]
    cases += [ps.ILL_AT + ("ill",)]
    for M, L, s in cases:
        run(new(M, L), f"{s}/{M}x{L}", ps.Case(M, L, s))
    for M, L in ps.WARM_SHAPES:
        gp = new(M, L)
        assert lib.moihgp_set_option(gp.handle, b"polar_warm_start", 1) == 0
        seq = ps.warm_sequence(M, L)
        for k, (label, case) in enumerate(seq):
            run(gp, f"warm{k + 1}-{label}/{M}x{L}", case)
        # the option call itself resets the flag: the update after it starts cold although the one before it left a basis behind
        assert lib.moihgp_set_option(gp.handle, b"polar_warm_start", 0) == 0
        assert lib.moihgp_set_option(gp.handle, b"polar_warm_start", 1) == 0
        run(gp, f"warm{len(seq) + 1}-A1/{M}x{L}", seq[-1][1])


if __name__ == "__main__":
    main()
