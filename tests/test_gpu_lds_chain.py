"""Serial LDS round trips taken out of a substep on the device (csrc/vnl_body.h: blk_apply in phases over the trips of a
product, factor_aba's pivot block writing only the line with V = U / D and 1/D1 left to one pass after the step loop and both
lane sets' line reads requested before either absorbs, the solver's qg1 / qg2 / Gauss scalars accumulated in the loops that
produce their operands): the product library against the regression build with the former forms (csrc/build.py --ldsplain).
The same operations on the same operands in another order of issue: every output bit for bit."""
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
STEPS = 2


@functools.lru_cache(maxsize=None)
def _variant(name):
    from vnl_brax_imitation_amd.csrc import build as hip_build

    return _lib.load_library(hip_build.build(variant=name))


def _rodent(n, lib, domain=None):
    with H.backend(lib):
        base = RodentTracking(H.reference_clip(), num_envs=n, device=DEV, **H.env_kwargs())
        return base if domain is None else base.with_domain(domain(base.sys, n))


def _rollout(env, n):
    """reset + two control steps on the inputs of tests/test_gpu_solver_staging.py (several envs with contacts)."""
    sf, noise, acts = S._inputs(n)
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
    return {"dof_damping": dom["dof_damping"], "dof_armature": dom["dof_armature"]}  # (damping feeds D2, armature both pivots)


@pytest.mark.parametrize("domain", [None, _damping_armature], ids=["plain", "damping_armature"])
def test_lds_round_trips_taken_out_change_no_bit_on_the_rodent(domain):
    """64 envs, the specialised kernels and their randomised instantiation."""
    n = 64
    new, old = _rodent(n, None, domain), _rodent(n, _variant("ldsplain"), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    _same(_rollout(new, n), _rollout(old, n), "plain" if domain is None else domain.__name__)


def test_generic_kernels_equal_the_specialised_ones_on_the_rodent():
    """The generic kernels read the trip counts of the products at run time (the phase form's windows of two trips behind
    wave-uniform branches); the specialised ones have them as constants."""
    n = 64
    new, gen = _rodent(n, None), _rodent(n, _variant("nospec"))
    assert int(new.dims.kernel_specialised) == 1 and int(gen.dims.kernel_specialised) == 0
    _same(_rollout(new, n), _rollout(gen, n), "nospec")


def test_lds_round_trips_taken_out_change_no_bit_on_the_humanoid():
    n = 64
    outs = []
    for lib in (None, _variant("ldsplain")):
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


def test_graphed_unroll_equals_the_regression_build():
    """One 20-step replay of a captured unroll, 64 envs, with each library: the step kernel inside a graph, resets included."""
    B, steps = 64, 20
    out = []
    for lib in (None, _variant("ldsplain")):
        base = _rodent(B, lib)
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
            state, data = acting.GraphedUnroll(env, state, policy, key, steps, extra_fields=("truncation",))()
        out.append((state, [x.clone() for x in acting._leaves(data)]))
    (s0, d0), (s1, d1) = out
    assert len(d0) == len(d1)
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n
    q = s0.pipeline_state.raw("qpos")
    assert torch.isfinite(q).all() and any(not torch.equal(x[0], x[-1]) for x in d0 if x.dim() > 1 and x.shape[0] == steps)
