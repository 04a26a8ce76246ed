"""polar_support.py's bar is a constant measured on the CPU: here it is measured again, so that it cannot drift from the cases it is for."""
import polar_support as ps


def test_bar_of_the_polar_tests_is_what_the_references_support():
    worst = ps.worst_ref_ratio()
    print(f"worst disagreement of LAPACK's factor and Q1 Q2^T: {worst:.3g} s(A)")
    assert worst <= ps.REF_WORST < worst + 0.01, (worst, ps.REF_WORST)
    assert ps.BAR == max(4.0 * ps.REF_WORST, 4.0)
