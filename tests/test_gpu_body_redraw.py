"""The body-domain redraw at fresh resets on the device: tests/body_redraw_cases.py on the randomised instantiations of
csrc/vnl_domain.hip -- the specialised rodent kernels (66 bodies as given: two lane trips) and the generic ones (the ant: a
five-member fold) at 64 envs --, the captured unroll against the eager wrapper, and a short train() run with body ranges.
The device's float64 fold against the host's, bit for bit: the test of the contraction pragma and of the member order."""
import functools
import os

import numpy as np
import pytest
import torch

import body_redraw_cases as R
import domain_cases as D
import fresh_reset_cases as F
import helpers as H
from vnl_brax_imitation_amd.envs.rodent import RodentTracking, body_domain_ranges_scaled
from vnl_brax_imitation_amd.model import mjcf
from vnl_brax_imitation_amd.ppo_imitation import ppo_networks
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 64


def _rodent(num_envs=B):
    return RodentTracking(F.three_clips(), num_envs=num_envs, device=DEV, **H.env_kwargs())


def _ant(num_envs=B):
    from vnl_brax_imitation_amd import envs

    m = mjcf.CompiledModel.load(os.path.join(H.ROOT, "vnl-brax-imitation_amd", "data", "ant.npz"))
    return envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(m),
                                model=m, num_envs=num_envs, device=DEV)


MAKERS = {"rodent": _rodent, "ant": _ant}
both = pytest.mark.parametrize("model", ["rodent", "ant"])


@both
def test_draw_is_the_restatement_and_the_tables_are_with_body_domain(model):
    """Case 1."""
    base = MAKERS[model]()
    assert int(base.dims.kernel_specialised) == (1 if model == "rodent" else 0)
    R.check_draw_is_the_restatement(base)


@both
def test_redrawn_env_is_the_env_set_by_hand(model):
    R.check_redrawn_env_is_the_env_set_by_hand(MAKERS[model]())


@both
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_redraw_inside_reset_done_is_the_separate_launch(model, weighted):
    """Case 3: the reset body of the fused launch reads the tables its own wave has just stored."""
    R.check_fused_is_separate(MAKERS[model](), weighted)


@both
def test_both_range_sets_together(model):
    R.check_both_range_sets_together(MAKERS[model]())


@both
def test_sharding_does_not_change_the_bodies_or_the_reset(model):
    R.check_sharding(MAKERS[model])


@both
def test_degenerate_and_absent_ranges(model):
    R.check_degenerate_and_absent_ranges(MAKERS[model]())


def test_errors_launch_nothing():
    R.check_errors_launch_nothing(_rodent(8))


def test_eager_wrapper_fused_unroll_and_graph_replay_agree_with_body_ranges():
    """Case 8: the eager wrapper, the fused unroll and one replay of GraphedUnroll per unroll length; body tables included (the
    graph's warm-up runs real resets: it has to put the body tables back)."""
    R.check_wrapper_paths(_rodent, DEV, graphed=True)


@both
def test_unfinished_envs_keep_their_first_bodies(model):
    R.check_unfinished_envs_keep_their_first_bodies(MAKERS[model], DEV)


def _train(env, **kw):
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=60,
                           encoder_layer_sizes=(128, 128), decoder_layer_sizes=(128, 128))
    _, params, metrics = ppo.train(
        environment=env, num_timesteps=2 * 64 * 5, episode_length=20, num_envs=64, learning_rate=1e-3, entropy_cost=1e-2,
        discounting=0.95, unroll_length=5, batch_size=16, num_minibatches=4, num_updates_per_batch=2, num_evals=2,
        normalize_observations=True, network_factory=nf, num_eval_envs=32, seed=1, auto_reset="fresh", **kw)
    return params, metrics, ppo.train.last_env_state, ppo.train.last_env.unwrapped


def test_training_with_body_domain_ranges():
    """Case 11, the sizes of test_training_with_domain_ranges: finite metrics; the training env's fused masses end inside the
    folded bounds (a fused mass is a sum of member masses: between the library's own folds of their bounds) and differ
    between envs."""
    env = _rodent(64)
    rg = body_domain_ranges_scaled(env.sys, mass=(0.7, 1.3))
    _, metrics, _, inner = _train(env, body_domain_ranges=rg, body_inertia_with_mass=True)
    for k in ("training/total_loss", "training/policy_loss", "training/v_loss", "eval/episode_reward"):
        assert k in metrics and np.isfinite(float(metrics[k])), k
    assert env.body_domain_ranges is None and inner is not env and inner.num_envs == 64  # the caller's env is left as it is
    assert inner.body_domain_ranges["inertia_with_mass"] is True
    # both bounds folded by the library itself: every drawn mass lies between its bounds, the float64 member sums run in the
    # same order and are monotone in every operand, and so is the cast -- no slack
    lo, hi = (_rodent(1).with_body_domain({"body_mass": x[None]}).domain_table("dom_mass")[0] for x in rg["body_mass"])
    t = inner.domain_table("dom_mass")
    assert bool((t >= lo).all()) and bool((t <= hi).all())
    assert bool((t[:, 1:].std(dim=0) > 0).all())  # the envs differ


def test_training_without_body_ranges_is_the_run_without_the_argument():
    """Case 11: body_domain_ranges=None changes nothing -- parameters, loss and the final env state, bit for bit."""
    a0, a1 = _train(_rodent(64), body_domain_ranges=None), _train(_rodent(64))
    assert torch.equal(a0[0][1], a1[0][1])
    assert a0[1]["training/total_loss"] == a1[1]["training/total_loss"]
    F.same_rows(F.snapshot(a0[2]), F.snapshot(a1[2]), torch.ones(64, dtype=torch.bool), F.WRITTEN + F.KEPT)
    assert a0[3].body_domain_ranges is None and a0[3].domain is None
