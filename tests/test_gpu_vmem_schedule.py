"""The vector-memory accesses of a substep outside the solver loop on the device (csrc/vnl_body.h: factor_aba's schedule words
and deferred 1/D2 store, euler()'s batched reload of the second inverse factor, forward()'s warm start, the table reads of a
trip requested together): the product library against the regression build with the former accesses
(csrc/build.py --vmemplain).  The same values by another route: every output bit for bit."""
import pytest

import variant_cases as V

pytestmark = pytest.mark.gpu
STEPS = 2


@pytest.mark.parametrize("domain", [V.friction, V.damping_armature], ids=["friction", "damping_armature"])
def test_vector_memory_schedule_changes_no_bit_on_the_rodent(domain):
    """64 envs, the randomised instantiation of the specialised kernels."""
    n = 64
    new, old = V.rodent(n, None, domain), V.rodent(n, V.variant("vmemplain"), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(new, n, STEPS), V.rollout(old, n, STEPS), domain.__name__, STEPS)


def test_generic_kernels_equal_the_specialised_ones_on_the_rodent():
    """The generic kernels keep a four-word window of the schedule and refill it; the specialised ones hold the row."""
    n = 64
    new, gen = V.rodent(n, None), V.rodent(n, V.variant("nospec"))
    assert int(new.dims.kernel_specialised) == 1 and int(gen.dims.kernel_specialised) == 0
    V.same(V.rollout(new, n, STEPS), V.rollout(gen, n, STEPS), "nospec", STEPS)


def test_vector_memory_schedule_changes_no_bit_on_the_humanoid():
    n = 32
    V.same(V.humanoid_rollout(None, n, STEPS), V.humanoid_rollout(V.variant("vmemplain"), n, STEPS), "humanoid", STEPS)


def test_graphed_unroll_replay_equals_the_eager_fused_unroll():
    """One 20-step replay of a captured unroll, 64 envs: the step kernel inside a graph, resets included."""
    V.same_unroll(V.small_unroll(None, 64, graphed=False), V.small_unroll(None, 64, graphed=True))
