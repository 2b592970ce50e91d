"""Subtree sums over a compile-time body tree (csrc/vnl_body.h, EnvWaveT::tree_accumulate_const: the walk of the composite
inertias and of cfrc unrolled over VnlSpecRodent::body_parent, every index a constant): the product library against the
regression build that keeps the run-time walk in the specialised kernels (csrc/build.py --treeplain).  The same adds on the same
operands in the same order: every output bit for bit.  The walk is per env and does not depend on the env count."""
import pytest
import torch

import body_domain_cases as BD
import fresh_reset_cases as F
import helpers as H
import variant_cases as V

pytestmark = pytest.mark.gpu
STEPS = 3
N = 128


def _old():
    return V.variant("treeplain")


def _specialised(*envs):
    """A stale table must fail here, not fall back silently to the generic kernels."""
    for e in envs:
        assert int(e.dims.kernel_specialised) == 1


def test_the_packaged_rodent_runs_the_specialised_kernels():
    _specialised(V.rodent(N, None), V.rodent(N, _old()))


@pytest.mark.parametrize("domain", [None, V.damping_armature], ids=["plain", "with_domain"])
def test_constant_tree_changes_no_bit_on_the_rodent(domain):
    """The specialised kernels and their randomised instantiation (VnlSpecDom), reset and three control steps: velocities
    and contacts are not trivial (variant_cases.rodent_inputs).  The plain `reset` case is here: the first snapshot of
    V.rollout is the output of vnl_env_reset (vnl_reset_kernel calls forward() and holds both walks), compared like the steps."""
    new, old = V.rodent(N, None, domain), V.rodent(N, _old(), domain)
    _specialised(new, old)
    V.same(V.rollout(new, N, STEPS), V.rollout(old, N, STEPS), "plain" if domain is None else "with_domain", STEPS)


def _with_bodies(lib):
    """Per-env masses and centres of mass: the inertias the walk sums differ from env to env."""
    base = V.rodent(N, lib)
    with H.backend(lib):
        return base.with_body_domain(BD.random_body_domain(base.sys, N, 31, fields=("body_mass", "body_ipos")))


def test_constant_tree_changes_no_bit_with_a_body_domain():
    new, old = _with_bodies(None), _with_bodies(_old())
    _specialised(new, old)
    a, b = V.rollout(new, N, STEPS), V.rollout(old, N, STEPS)
    V.same(a, b, "body_domain", STEPS)
    plain = V.rollout(V.rodent(N, None), N, 1)
    assert not torch.equal(a[1]["ps.qvel"], plain[1]["ps.qvel"])  # (the bodies did change the dynamics)


@pytest.mark.parametrize("bodies", [False, True], ids=["plain", "body_domain"])
def test_constant_tree_changes_no_bit_in_a_fresh_reset_of_some_envs(bodies):
    """vnl_reset_done_kernel calls forward() and holds both walks: every third env starts a fresh episode two steps in."""
    mask = (torch.arange(N) % 3 == 0).float()
    snaps = []
    for lib in (None, _old()):
        env = _with_bodies(lib) if bodies else V.rodent(N, lib)
        _specialised(env)
        st = F.stepped_state(env, 7)
        before = F.snapshot(st)
        F.reset_done(env, st, mask)
        snaps.append((before, F.snapshot(st)))
    (b0, a0), (b1, a1) = snaps
    rows = torch.ones(N, dtype=torch.bool)
    F.same_rows(b0, b1, rows, tuple(b0))
    F.same_rows(a0, a1, rows, tuple(a0))
    assert not torch.equal(b0["qpos"][mask.bool()], a0["qpos"][mask.bool()])  # (the masked envs did start anew)
    assert torch.equal(b0["qpos"][~mask.bool()], a0["qpos"][~mask.bool()])


def test_graphed_unroll_equals_the_eager_unroll_of_the_regression_build():
    """One 20-step replay of a captured unroll with the product library (the step kernel inside a graph, resets included)
    against the eager fused unroll of the regression build."""
    V.same_unroll(V.small_unroll(None, N, graphed=True), V.small_unroll(_old(), N, graphed=False), tail=True)
