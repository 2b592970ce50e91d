"""The rollout post-processing as the epilogue of the env step kernel (vnl_env_step_post, acting._POST_EPILOGUE) on the
device, against the two launches it replaces: the entry itself on the case of tests/post_epilogue_cases.py, then unrolls
of T = 3 with episodes of 2 steps over 67 envs (more than one workgroup, no multiple of anything) on every route that
reaches a step kernel of its own -- the specialised and the generic instantiation, the randomised one, the fresh
auto-reset, the generator and the device-noise policy, the eager loop and the captured graph.  Every Transition leaf and
every carried state tensor, bit for bit."""
import functools

import pytest
import torch

import domain_cases as D
import helpers as H
import post_epilogue_cases as PE
from variant_cases import variant as _variant
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.rodent import RodentTracking

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 67


def _rodent(lib=None, domain=False, n=B):
    with H.backend(lib):
        base = RodentTracking(H.reference_clip(), num_envs=n, device=DEV, **H.env_kwargs())
    return base.with_domain(D.random_domain(base.sys, n, 12)) if domain else base


@functools.lru_cache(maxsize=None)
def _two_launches(route):
    """the reference of a route: computed once, shared, left unchanged"""
    return PE.unroll_case(*ROUTES[route][0], False, **ROUTES[route][1])


ROUTES = {
    "generator_policy": ((_rodent, DEV), {}),
    "device_noise_direct_log": ((_rodent, DEV), {"noise": "device"}),
    "fresh_auto_reset": ((_rodent, DEV), {"noise": "device", "mode": "fresh"}),
    "with_domain": ((lambda: _rodent(domain=True), DEV), {}),
    "generic_kernels": ((lambda: _rodent(lib=_variant("nospec")), DEV), {}),
}


def test_step_with_epilogue_equals_step_then_post_on_every_buffer():
    PE.assert_same(PE.direct_case(_rodent(), fused=True), PE.direct_case(_rodent(), fused=False))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_unroll_with_epilogue_equals_the_two_launch_unroll(route):
    (make, dev), kw = ROUTES[route]
    seen = []

    def hook(base):  # (counts the ops of the steps that carry a descriptor)
        orig = base.step

        def step(st, a):
            d = getattr(base, "_post_desc", None)
            seen.append(None if d is None else int(d.num_ops))
            return orig(st, a)

        base.step = step

    got = PE.unroll_case(make, dev, True, hook=hook, **kw)
    PE.assert_unrolls_same(got, _two_launches(route))
    assert len(seen) == 3 and all(n is not None and 0 <= n <= _lib.POST_MAX_OPS for n in seen), seen
    trunc = got[0][0][-1]
    assert trunc.shape == (3, B) and float(trunc.sum()) > 0  # episodes of 2 steps did end inside the unroll


def test_graphed_unroll_replayed_twice_equals_the_eager_unroll_run_twice():
    eager = PE.unroll_case(_rodent, DEV, True, calls=2)
    graph = PE.unroll_case(_rodent, DEV, True, calls=2, graphed=True)
    PE.assert_unrolls_same(graph, eager)
    PE.assert_unrolls_same(graph, PE.unroll_case(_rodent, DEV, False, calls=2))


def test_kernel_events_of_a_hooked_step_are_recorded_on_the_fused_path():
    """bench.py --full replaces base.step by a two-argument hook that arms base.kernel_events before the call"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
    fused = []

    def hook(base):
        orig, k = base.step, [0]

        def step_hook(st_, a_):
            base.kernel_events = pairs[k[0]]
            k[0] += 1
            fused.append(getattr(base, "_post_desc", None) is not None)
            return orig(st_, a_)

        base.step = step_hook

    PE.unroll_case(_rodent, DEV, True, hook=hook)
    torch.cuda.synchronize(DEV)
    assert fused == [True] * 3
    assert all(a.elapsed_time(b) > 0 for a, b in pairs)
