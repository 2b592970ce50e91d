"""SGPR spill traffic taken out of the substep loop (csrc/vnl_body.h, VNL_LOCAL / VNL_ROLLED / VNL_LANE_RANGE: lane predicates
computed where they are used instead of being hoisted to the top of the kernel, parked in VGPR lanes and read back at every
use; the debug trace's row walk as a loop instead of 156 hoisted literal addresses; lane < 64 stated, so that one-trip regions
carry no mask): the product library against the regression build with
the former forms (csrc/build.py --sgprplain).  The same compares on the same operands, issued in another place: every
output bit for bit."""
import pytest

import variant_cases as V

pytestmark = pytest.mark.gpu
STEPS = 3
N = 128  # (partially filled CUs; the rodent's 73 dofs take both trips of every product and the guest rows)


@pytest.mark.parametrize("domain", [None, V.damping_armature], ids=["plain", "with_domain"])
def test_predicates_computed_at_their_use_change_no_bit_on_the_rodent(domain):
    """128 envs, the specialised kernels (CG 6 / 6) and their randomised instantiation (VnlSpecDom)."""
    new, old = V.rodent(N, None, domain), V.rodent(N, V.variant("sgprplain"), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(new, N, STEPS), V.rollout(old, N, STEPS), "plain" if domain is None else "with_domain", STEPS)


def test_generic_kernels_with_the_new_forms_equal_the_former_specialised_ones():
    """The shipped `nospec` library is compiled from the same sources WITH the new forms (only -DVNL_SGPR_PLAIN switches them
    off): the generic kernels, whose bounds are run-time values the compiler cannot hoist as constants, against the former
    forms in the specialised kernel."""
    gen, old = V.rodent(N, V.variant("nospec")), V.rodent(N, V.variant("sgprplain"))
    assert int(gen.dims.kernel_specialised) == 0 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(gen, N, STEPS), V.rollout(old, N, STEPS), "nospec", STEPS)


def test_predicates_computed_at_their_use_change_no_bit_on_the_humanoid():
    """64 envs: a single lane set, the other factor routes."""
    n = 64
    V.same(V.humanoid_rollout(None, n, STEPS), V.humanoid_rollout(V.variant("sgprplain"), n, STEPS), "humanoid", STEPS)


def test_graphed_unroll_equals_the_eager_unroll_of_the_regression_build():
    """One 20-step replay of a captured unroll with the product library, 128 envs (the step kernel inside a graph, resets
    included), against the eager fused unroll of the regression build."""
    V.same_unroll(V.small_unroll(None, N, graphed=True), V.small_unroll(V.variant("sgprplain"), N, graphed=False), tail=True)
