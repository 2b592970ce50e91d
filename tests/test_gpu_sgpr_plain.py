"""SGPR spill traffic taken out of the substep loop (csrc/vnl_body.h, VNL_LOCAL / VNL_ROLLED / VNL_LANE_RANGE: lane predicates
computed where they are used instead of being hoisted to the top of the kernel, parked in VGPR lanes and read back at every
use; the debug trace's row walk as a loop instead of 156 hoisted literal addresses; lane < 64 stated, so that one-trip regions
carry no mask): the product library against the regression build with
the former forms (csrc/build.py --sgprplain).  The same compares on the same operands, issued in another place: every
output bit for bit."""
import functools

import numpy as np
import pytest
import torch

import domain_cases as D
import helpers as H
import test_gpu_solver_staging as S
import test_humanoid as Hu
import test_solver_tail as T
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.envs.rodent import RodentTracking
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 3
N = 128  # (partially filled CUs; the rodent's 73 dofs take both trips of every product and the guest rows)


@functools.lru_cache(maxsize=None)
def _variant(name):
    from vnl_brax_imitation_amd.csrc import build as hip_build

    return _lib.load_library(hip_build.build(variant=name))


def _rodent(n, lib, domain=None):
    with H.backend(lib):
        base = RodentTracking(H.reference_clip(), num_envs=n, device=DEV, **H.env_kwargs())
        return base if domain is None else base.with_domain(domain(base.sys, n))


def _rollout(env, n):
    """reset + three control steps on the inputs of tests/test_gpu_solver_staging.py (several envs with contacts)."""
    sf, noise, acts = S._inputs(n)
    assert len(acts) >= STEPS
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    snaps = [T._outputs(st)]
    for a in acts[:STEPS]:
        st = env.step(st, torch.from_numpy(a))
        snaps.append(T._outputs(st))
    return snaps


def _same(a_snaps, b_snaps, tag):
    assert len(a_snaps) == len(b_snaps) == STEPS + 1
    for t, (a, b) in enumerate(zip(a_snaps, b_snaps)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (tag, t, k)
    assert not torch.equal(a_snaps[-1]["ps.qpos"], a_snaps[0]["ps.qpos"])
    assert all(torch.isfinite(v).all() for k, v in a_snaps[-1].items() if v.is_floating_point()), tag


def _damping_armature(sys, n):
    dom = D.random_domain(sys, n, 22)
    return {"dof_damping": dom["dof_damping"], "dof_armature": dom["dof_armature"]}


@pytest.mark.parametrize("domain", [None, _damping_armature], ids=["plain", "with_domain"])
def test_predicates_computed_at_their_use_change_no_bit_on_the_rodent(domain):
    """128 envs, the specialised kernels (CG 6 / 6) and their randomised instantiation (VnlSpecDom)."""
    new, old = _rodent(N, None, domain), _rodent(N, _variant("sgprplain"), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    _same(_rollout(new, N), _rollout(old, N), "plain" if domain is None else "with_domain")


def test_generic_kernels_with_the_new_forms_equal_the_former_specialised_ones():
    """The shipped `nospec` library is compiled from the same sources WITH the new forms (only -DVNL_SGPR_PLAIN switches them
    off): the generic kernels, whose bounds are run-time values the compiler cannot hoist as constants, against the former
    forms in the specialised kernel."""
    gen, old = _rodent(N, _variant("nospec")), _rodent(N, _variant("sgprplain"))
    assert int(gen.dims.kernel_specialised) == 0 and int(old.dims.kernel_specialised) == 1
    _same(_rollout(gen, N), _rollout(old, N), "nospec")


def test_predicates_computed_at_their_use_change_no_bit_on_the_humanoid():
    """64 envs: a single lane set, the other factor routes."""
    n = 64
    outs = []
    for lib in (None, _variant("sgprplain")):
        with H.backend(lib):
            env = Hu._env(n, device=DEV)
        rng = np.random.default_rng(3)
        st = env.reset(5)
        snaps = [T._outputs(st)]
        for _ in range(STEPS):
            st = env.step(st, torch.from_numpy(np.clip(0.3 * rng.standard_normal((n, 21)), -1, 1).astype(np.float32)))
            snaps.append(T._outputs(st))
        outs.append(snaps)
    _same(outs[0], outs[1], "humanoid")


def test_graphed_unroll_equals_the_eager_unroll_of_the_regression_build():
    """One 20-step replay of a captured unroll with the product library, 128 envs (the step kernel inside a graph, resets
    included), against the eager fused unroll of the regression build."""
    steps = 20
    out = []
    for lib, graphed in ((None, True), (_variant("sgprplain"), False)):
        base = _rodent(N, lib)
        with H.backend(lib):
            env = W.AutoResetWrapper(W.EpisodeWrapper(base, episode_length=8, action_repeat=1))
            nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                            preprocess_observations_fn=running_statistics.normalize,
                                                            intention_latent_size=16, encoder_layer_sizes=(32,),
                                                            decoder_layer_sizes=(32,))
            flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(DEV)
            policy = ppo_networks.make_inference_fn(nets)((running_statistics.init_state(base.observation_size, device=DEV), flat))
            torch.manual_seed(123)
            state = env.reset(torch.Generator().manual_seed(5))
            key = torch.Generator(device=DEV).manual_seed(11)
            if graphed:
                state, data = acting.GraphedUnroll(env, state, policy, key, steps, extra_fields=("truncation",))()
            else:
                state, data = acting.generate_unroll(env, state, policy, key, steps, extra_fields=("truncation",), fused=True)
        out.append((state, [x.clone() for x in acting._leaves(data)]))
    (s0, d0), (s1, d1) = out
    assert len(d0) == len(d1)
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n
    q = s0.pipeline_state.raw("qpos")
    assert torch.isfinite(q).all() and any(not torch.equal(x[0], x[-1]) for x in d0 if x.dim() > 1 and x.shape[0] == steps)
