"""Recorded rollouts (include/vnl.h vnl_record_desc) on the host build of the product source (float32): vnl_env_record against
a NumPy restatement, its validation, acting.RolloutRecorder through the generic and the fused eager evaluation loop against
a plain loop that clones the same tensors, the torch restatement against the kernel, the replay of recorded latents, and
Evaluator / train() with a recorder.  tests/test_gpu_rollout_record.py runs the same cases on the device."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import record_cases as RC
from vnl_brax_imitation_amd.ppo_imitation import ppo_networks
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

DEV = torch.device("cpu")


def _rodent(n=RC.B_ROD, **kw):
    return lambda: H.hostsim_env(n, "float", **kw)


@pytest.mark.parametrize("num_envs", [5, 70])
def test_standalone_recording_equals_the_sequential_restatement(num_envs):
    RC.check_standalone(H.hostsim_env(num_envs, "float", reference_clip=RC.two_clips()))


def test_validation_names_the_field_and_writes_nothing():
    RC.check_validation(H.hostsim_env(3, "float"))


@functools.lru_cache(maxsize=None)
def _clone_loop(mode, kind):
    return RC.clone_loop(_rodent(), DEV, mode, kind)


@pytest.mark.parametrize("route", ["generic", "eager"])
@pytest.mark.parametrize("mode,kind", [("first_state", "full"), ("fresh", "full"), ("fresh", "decoder"), ("first_state", "decoder")])
def test_recorder_equals_the_clone_loop(mode, kind, route):
    rows, base = _clone_loop(mode, kind)
    _, out = RC.recorded_case(_rodent(), DEV, mode, kind, route)
    RC.check_against_clone_loop(rows, base, out)
    RC.check_terminal_rows(out, mode)
    if kind == "decoder":
        assert "latent" in out.columns and out.latent.shape == (RC.B_ROD, RC.T_ROD + 1, 16)


@pytest.mark.parametrize("mode", ["first_state", "fresh"])
def test_recorder_stops_at_done_and_follows_its_env_index(mode):
    rows, base = _clone_loop(mode, "full")
    idx = [5, 0, -1, 5, RC.B_ROD, 2]
    _, out = RC.recorded_case(_rodent(), DEV, mode, "full", "eager", stop_at_done=True, env_index=idx)
    RC.check_against_clone_loop(rows, base, out, stop_at_done=True, env_index=idx)
    assert out.length.max() == RC.EPISODE + 1  # the reset row and an episode


@pytest.mark.parametrize("mode", ["first_state", "fresh"])
def test_torch_restatement_equals_the_kernel(mode):
    idx = [5, 0, -1, 5, RC.B_ROD, 2]
    for kw in (dict(), dict(stop_at_done=True, env_index=idx)):
        a, _ = RC.recorded_case(_rodent(), DEV, mode, "decoder", "eager", kernel=True, **kw)
        b, _ = RC.recorded_case(_rodent(), DEV, mode, "decoder", "eager", kernel=False, **kw)
        RC.same_recorder(a, b)


def test_recorded_latents_replay_the_rollout():
    RC.check_latent_replay(_rodent(), DEV)


@pytest.mark.parametrize("route", ["generic", "eager"])
def test_evaluator_records_two_envs_and_scores_as_without(route, tmp_path):
    RC.check_evaluator(_rodent(6, **RC.FALLING), DEV, route, tmp_path)


def _train(**kw):
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=16, encoder_layer_sizes=(32,),
                           decoder_layer_sizes=(32,), value_hidden_layer_sizes=(32,))
    _, _, metrics = ppo.train(environment=H.hostsim_env(4), num_timesteps=4 * 5 * 2, episode_length=6, num_envs=4,
                              unroll_length=5, batch_size=2, num_minibatches=2, num_updates_per_batch=1, num_evals=1,
                              network_factory=nf, num_eval_envs=4, **kw)
    return metrics


def test_train_hands_its_evaluators_recording_to_policy_params_fn(tmp_path):
    seen = []

    def policy_params_fn(step, make_policy, params):
        seen.append(ppo.train.last_evaluator.recorded)

    default = _train()
    plain = ppo.train.last_evaluator
    assert plain.recorded is None and plain._recorder is None
    m = _train(eval_record_envs=1, policy_params_fn=policy_params_fn)
    ev = ppo.train.last_evaluator
    assert sorted(m) == sorted(default)
    assert np.array_equal(RC.bits(ev.records), RC.bits(plain.records))  # the evaluation is what it is without a recorder
    out = ev.recorded
    assert len(seen) == 1 and seen[0] is out
    assert out.length.shape == (1,) and 2 <= out.length[0] <= 7 and out.qpos.shape == (1, 7, int(ev._env.unwrapped.dims.nq))
    assert out.length[0] == ev.records[0, 2] + 1 and out.done[0, out.length[0] - 1, 0] == 1
    out.save(tmp_path / "r.npz")
    back = type(out).load(tmp_path / "r.npz")
    assert all(np.array_equal(RC.bits(back.columns[k]), RC.bits(out.columns[k])) for k in out.columns)
    assert np.array_equal(RC.bits(back.render_qpos), RC.bits(out.render_qpos))
