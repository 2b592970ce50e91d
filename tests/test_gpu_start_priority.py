"""Prioritised start frames on the device: the weighted draw of vnl_reset_done_kernel (a wave-wide 64-ary search: one, two
and three rounds) and its outcome counters in the four instantiations, vnl_priority_kernel, the captured unroll with a
priority against the eager one, and a short train() run."""
import functools

import pytest
import torch

import body_domain_cases as BD
import domain_cases as D
import fresh_reset_cases as F
import helpers as H
import start_priority_cases as S
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.rodent import RodentTracking
from vnl_brax_imitation_amd.envs.start_priority import StartPriority
from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DOM_TABLES = ("dom_mu", "dom_invw", "dom_gain", "dom_damp", "dom_arm", "dom_mass", "dom_ipos", "dom_inertia6", "dom_tminv")


def _mask(B):
    """roughly one env in three, from a fixed generator"""
    return (torch.rand(B, generator=torch.Generator().manual_seed(17)) < 1 / 3).float()


def _rodent(B, clip=None, **over):
    return RodentTracking(clip if clip is not None else F.three_clips(), num_envs=B, device=DEV, **{**H.env_kwargs(), **over})


def test_specialised_rodent_two_round_search_256_envs():
    """Checks 1 to 4 at 256 envs, three clips: 705 cells, two rounds."""
    env = _rodent(256)
    assert env.dims.kernel_specialised == 1 and S.ncells(env) == 705
    S.check_draws_and_reset(env, _mask(256))
    S.check_counters(_rodent(64, sub_clip_length=2))


def test_generic_ant_one_round_search_64_envs():
    """Checks 1 to 4 with AntTracking (start_hi == 1: a cell is a clip), the generic instantiation, one round."""
    env = S.ant_env(64, device="cuda:0")
    assert env.dims.kernel_specialised == 0 and env._start_hi() == 1 and S.ncells(env) == 3
    S.check_draws_and_reset(env, _mask(64))
    S.check_counters(env)


def test_three_round_search_64_envs_18_clips():
    """Checks 1 and 3 with the golden clip stacked 18 times: 4230 cells, three rounds."""
    c = H.reference_clip()
    clip = type(c).stack([c] * 18)
    env = _rodent(64, clip)
    assert S.ncells(env) == 4230
    S.check_draws_and_reset(env, _mask(64), reset_check=False, null_check=False)
    S.check_counters(_rodent(64, clip, sub_clip_length=2))


def test_randomised_env_keeps_its_tables_64_envs():
    """Checks 1 to 3 in a VnlSpecDom instantiation, a four-field and a body domain set: the per-env tables are
    bit-identical before and after."""
    def randomised(base):
        return base.with_domain(D.random_domain(base.sys, 64, 21)).with_body_domain(BD.random_body_domain(base.sys, 64, 22))

    env = randomised(_rodent(64))
    tables = {k: env.domain_table(k) for k in DOM_TABLES}
    S.check_draws_and_reset(env, _mask(64), null_check=False)
    for k, v in tables.items():
        assert torch.equal(env.domain_table(k), v), k
    S.check_counters(randomised(_rodent(64, sub_clip_length=2)))


def test_update_kernel_equals_its_integer_restatement():
    """Check 5 on vnl_priority_kernel, and the argument checks of its entry."""
    L = _lib.load_library()
    S.check_update(L, DEV)
    S.check_update_argument_errors(L, DEV)


def _setup(B=64, episode_length=150):
    base = _rodent(B, H.reference_clip())  # the reference's sub_clip_length = 10: episodes end inside a 12-step unroll
    prio = StartPriority(base)
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1), mode="fresh", seed=41,
                           start_priority=prio)
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(DEV)
    norm = running_statistics.init_state(base.observation_size, device=DEV)
    policy = ppo_networks.make_inference_fn(nets)((norm, flat), noise="device", seed=9)
    return env, prio, policy, env.reset(torch.Generator().manual_seed(5))


def _state_leaves(s):
    return [s.obs, s.done, s.reward] + [s.pipeline_state.raw(n) for n in s.pipeline_state._FIELDS] + \
        [s.info[k] for k in ("steps", "truncation", "traj", "cur_frame", "sub_clip_frame", "clip_id", "reset_step")]


def test_captured_unroll_equals_the_eager_unroll_with_a_priority():
    """After tests/test_gpu_fresh_reset.py: device-noise policy, B = 64, T = 12, two replays with update() between them;
    data, state, counters and table, bit for bit."""
    T, extra = 12, ("truncation", "traj")
    runs = []
    for graphed in (False, True):
        env, prio, policy, state = _setup()
        uniform = prio.cdf.clone()
        g = acting.GraphedUnroll(env, state, policy, None, T, extra_fields=extra) if graphed else None
        assert int(prio.ended.sum()) == 0 and int(state.info["reset_step"]) == 0  # building the graph counts and draws nothing
        datas, tables = [], []
        for k in range(2):
            state, data = g() if g else acting.generate_unroll(env, state, policy, None, T, extra_fields=extra, fused=True)
            datas.append([x.clone() for x in acting._leaves(data)])
            if k == 0:
                assert int(prio.ended.sum()) > 0
                prio.update()
                assert not torch.equal(prio.cdf, uniform)
            tables.append([x.clone() for x in (prio.cdf, prio.ended, prio.failed)])
        torch.cuda.synchronize(DEV)
        assert int(state.info["reset_step"]) == 2 * T
        runs.append((datas, tables, [x.clone() for x in _state_leaves(state)]))
    (d0, t0, s0), (d1, t1, s1) = runs
    for a_, b_ in zip(d0 + t0, d1 + t1):
        for a, b in zip(a_, b_):
            assert a.shape == b.shape and torch.equal(a, b)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)


def test_train_with_start_priority():
    """One train() call at the sizes of test_train_with_fresh_resets, with start_priority=True."""
    env = RodentTracking(H.reference_clip(), num_envs=64, device=DEV, **H.env_kwargs())
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=60,
                           encoder_layer_sizes=(128, 128), decoder_layer_sizes=(128, 128))
    log = []
    ppo.train(
        environment=env, num_timesteps=2 * 64 * 5, episode_length=150, num_envs=64, learning_rate=1e-3,
        entropy_cost=1e-2, discounting=0.95, unroll_length=5, batch_size=16, num_minibatches=4,
        num_updates_per_batch=2, num_evals=1, normalize_observations=True, network_factory=nf, num_eval_envs=0,
        eval_env=None, seed=3, policy_noise="device", auto_reset="fresh", start_priority=True,
        progress_fn=lambda s, m: log.append(m))
    st, prio = ppo.train.last_env_state, ppo.train.last_start_priority
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in log[-1].values())
    assert int(prio.ended.sum()) > 0
    uniform = S.as_words(philox.start_priority_table(torch.zeros(235, dtype=torch.int32), torch.zeros(235, dtype=torch.int32))[0])
    assert not torch.equal(prio.cdf.cpu(), uniform)
    start = (st.info["cur_frame"] - st.info["sub_clip_frame"]).cpu()
    assert bool(((start >= 0) & (start < 235)).all())
