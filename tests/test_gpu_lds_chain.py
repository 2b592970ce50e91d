"""Serial LDS round trips taken out of a substep on the device (csrc/vnl_body.h: blk_apply in phases over the trips of a
product, factor_aba's pivot block writing only the line with V = U / D and 1/D1 left to one pass after the step loop and both
lane sets' line reads requested before either absorbs, the solver's qg1 / qg2 / Gauss scalars accumulated in the loops that
produce their operands): the product library against the regression build with the former forms (csrc/build.py --ldsplain).
The same operations on the same operands in another order of issue: every output bit for bit."""
import pytest

import variant_cases as V

pytestmark = pytest.mark.gpu
STEPS = 2


@pytest.mark.parametrize("domain", [None, V.damping_armature], ids=["plain", "damping_armature"])
def test_lds_round_trips_taken_out_change_no_bit_on_the_rodent(domain):
    """64 envs, the specialised kernels and their randomised instantiation."""
    n = 64
    new, old = V.rodent(n, None, domain), V.rodent(n, V.variant("ldsplain"), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(new, n, STEPS), V.rollout(old, n, STEPS), "plain" if domain is None else domain.__name__, STEPS)


def test_generic_kernels_equal_the_specialised_ones_on_the_rodent():
    """The generic kernels read the trip counts of the products at run time (the phase form's windows of two trips behind
    wave-uniform branches); the specialised ones have them as constants."""
    n = 64
    new, gen = V.rodent(n, None), V.rodent(n, V.variant("nospec"))
    assert int(new.dims.kernel_specialised) == 1 and int(gen.dims.kernel_specialised) == 0
    V.same(V.rollout(new, n, STEPS), V.rollout(gen, n, STEPS), "nospec", STEPS)


def test_lds_round_trips_taken_out_change_no_bit_on_the_humanoid():
    n = 64
    V.same(V.humanoid_rollout(None, n, STEPS), V.humanoid_rollout(V.variant("ldsplain"), n, STEPS), "humanoid", STEPS)


def test_graphed_unroll_equals_the_regression_build():
    """One 20-step replay of a captured unroll, 64 envs, with each library: the step kernel inside a graph, resets included."""
    V.same_unroll(V.small_unroll(None, 64, graphed=True), V.small_unroll(V.variant("ldsplain"), 64, graphed=True), tail=True)
