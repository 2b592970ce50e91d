"""Scored evaluation episodes (include/vnl.h vnl_eval_desc) on the host build of the product source (float32): the
standalone launch vnl_rollout_eval against a NumPy restatement, the fused entry vnl_env_step_post_eval against the three
launches it replaces, the routes of acting.Evaluator against each other, the fresh-mode records against the reset draws,
the validation, and train() with several fresh episodes per eval env.  tests/test_gpu_eval_epilogue.py runs the same cases
on the device."""
import functools

import numpy as np
import pytest
import torch

import domain_redraw_cases as R
import eval_cases as E
import fresh_reset_cases as F
import helpers as H
import model_cases as M
import post_epilogue_cases as PE
from vnl_brax_imitation_amd.ppo_imitation import ppo_networks
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

DEV = torch.device("cpu")
FALLING = dict(healthy_z_range=(0.0, 0.5))  # envs fall out of the healthy range on their own (tests/test_wrappers.py)
# .. after 8 to 10 steps.  Episodes of 4 steps need a lower ceiling for some envs to end on their own: under this one an env
# ends after 1 step or runs its 4, depending on its start frame
FALLING_SOON = dict(healthy_z_range=(0.0, 0.08))


@pytest.mark.parametrize("num_envs", [1, 63, 64, 65, 257])
def test_standalone_scoring_equals_the_sequential_restatement(num_envs):
    E.check_standalone(H.hostsim_library("float"), DEV, num_envs)


def test_step_post_eval_equals_the_three_launches_on_every_buffer():
    three = E.direct_case(H.hostsim_env(5, "float"), fused=False)
    one = E.direct_case(H.hostsim_env(5, "float"), fused=True)
    PE.assert_same(one, three)


def _falling(n=6, **kw):
    return lambda: H.hostsim_env(n, "float", **FALLING, **kw)


def test_default_evaluation_is_the_same_by_the_generic_and_the_fused_route():
    """3 (a): K = 1 from the first state -- the dict of the generic loop (the evaluation as it was), bit for bit, and the
    wrapper's eval_metrics."""
    gen = E.evaluator_case(_falling(), DEV, "generic", episode_length=9)
    fus = E.evaluator_case(_falling(), DEV, "eager", episode_length=9)
    E.assert_same_evaluation(gen, fus)
    a, b = E.eval_metrics_of(gen[2]), E.eval_metrics_of(fus[2])
    assert sorted(a) == sorted(b) and all(np.array_equal(E.bits(a[k]), E.bits(b[k])) for k in a)
    assert set(gen[0]) == E.DEFAULT_EVAL_KEYS
    rec = fus[1]
    assert rec.shape == (6, 12) and (rec[:, 2] < 9).any() and (rec[:, 3] == 1).any()  # fell on their own; were truncated
    assert np.array_equal(rec[:, 2], a["steps"]) and np.array_equal(rec[:, 11], a["m.reward"])


def test_several_fresh_episodes_with_domain_ranges_are_the_same_by_both_routes():
    """3 (b): K = 3, fresh auto-reset, episodes of 4 steps, the domain redrawn at every reset."""
    make = lambda: H.hostsim_env(6, "float", reference_clip=F.three_clips(), **FALLING_SOON)  # noqa: E731
    ranges = R.ranges_for(H.model())
    gen = E.evaluator_case(make, DEV, "generic", K=3, mode="fresh", episode_length=4, ranges=ranges)
    fus = E.evaluator_case(make, DEV, "eager", K=3, mode="fresh", episode_length=4, ranges=ranges)
    E.assert_same_evaluation(gen, fus)
    m, rec = fus[0], fus[1]
    assert m["eval/episodes_scored"] == rec.shape[0] and 0 < m["eval/truncated_fraction"] < 1  # both ways of ending
    assert ((rec[:, 3] == 0) & (rec[:, 2] < 4)).any() and ((rec[:, 3] == 1) & (rec[:, 2] == 4)).any()
    count = fus[2].state.info["eval_count"].numpy()
    assert count.max() == 3 and rec.shape[0] == count.sum()
    per_env = np.split(rec, np.cumsum(count)[:-1])
    assert any(len(r) > 1 and len(set(r[:, 0])) > 1 for r in per_env)  # two records of one env differ in start frame


def test_some_env_is_through_while_another_is_still_scored():
    """3: with K > 1 an env reaches count == K while another is still being scored, and is ignored from then on."""
    make = lambda: H.hostsim_env(6, "float", reference_clip=F.three_clips(), **FALLING_SOON)  # noqa: E731
    _, st, dones, counts = E.unroll_states(make, DEV, K=3, mode="fresh", episode_length=4, T=10, fused=True)
    through = [(t, bool((counts[t] == 3).any() and (counts[t] < 3).any())) for t in range(10)]
    assert any(x for _, x in through), counts
    t0 = next(t for t, x in through if x)
    e = int((counts[t0] == 3).nonzero()[0])
    assert bool(dones[t0 + 1:, e].any()) and int(counts[-1, e]) == 3  # it went on ending episodes, which were not scored


def test_ant_scores_by_the_launch_of_its_own_with_the_switch_on_and_off():
    """3 (c): AntTracking.step works on the state after the kernel, so the scoring must be vnl_rollout_eval after it.  (Every
    ant starts from frame 0 without noise and stands through an episode of 3 steps: all twelve records are truncations, each
    env's two on clips of its own draw.)"""
    seen = []

    def hook(base):
        orig = base.step

        def step(st, a):
            seen.append(getattr(base, "_eval_desc", None) is not None)
            return orig(st, a)

        base.step = step

    runs = []
    for on in (True, False):
        with E.eval_epilogue(on):
            runs.append(E.evaluator_case(lambda: M.ant_env(6, clips=3), DEV, "eager", K=2, mode="fresh", episode_length=3, hook=hook))
    E.assert_same_evaluation(*runs)
    E.assert_same_evaluation(runs[0], E.evaluator_case(lambda: M.ant_env(6, clips=3), DEV, "generic", K=2, mode="fresh", episode_length=3))
    assert seen == [False] * 12 and runs[0][1].shape == (12, 12) and bool((runs[0][1][:, 3] == 1).all())


@pytest.mark.parametrize("fused", [False, True], ids=["wrappers", "fused"])
def test_fresh_records_carry_the_draws_of_the_reset_that_began_them(fused):
    make = lambda: H.hostsim_env(6, "float", reference_clip=F.three_clips(), **FALLING_SOON)  # noqa: E731
    E.check_fresh_records(make, DEV, fused)


def test_validation_names_the_field_and_launches_nothing():
    E.check_validation(H.hostsim_env(2, "float"))


def _train(**kw):
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=16, encoder_layer_sizes=(32,),
                           decoder_layer_sizes=(32,), value_hidden_layer_sizes=(32,))
    _, _, metrics = ppo.train(environment=H.hostsim_env(4), num_timesteps=4 * 5 * 2, episode_length=6, num_envs=4,
                              unroll_length=5, batch_size=2, num_minibatches=2, num_updates_per_batch=1, num_evals=1,
                              network_factory=nf, num_eval_envs=4, **kw)
    return metrics


def test_train_scores_two_fresh_episodes_per_eval_env():
    default = _train()
    m = _train(eval_episodes_per_env=2, eval_auto_reset="fresh")
    assert m["eval/episodes_scored"] == 8 and 0.0 <= m["eval/truncated_fraction"] <= 1.0
    assert {k for k in default if k.startswith("eval/")} == E.DEFAULT_EVAL_KEYS  # the default call's keys are what they were
    assert set(m) - set(default) == {"eval/episodes_scored", "eval/truncated_fraction"} and set(default) <= set(m)
    assert ppo.train.last_evaluator.records.shape == (8, 12)
    with pytest.raises(ValueError, match="eval_auto_reset"):
        _train(eval_auto_reset="sometimes")
