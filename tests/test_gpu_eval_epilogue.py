"""Scored evaluation episodes on the device (the cases of tests/eval_cases.py through the C-ABI of the product library):
vnl_rollout_eval against the NumPy restatement at one env, around the wave's 64 and over several workgroups;
vnl_env_step_post_eval against the three launches it replaces on the specialised, the generic and the randomised step
kernel; acting.Evaluator by the generic loop, the fused eager loop and the captured graph; the fresh-mode records against
the reset draws; the validation."""
import numpy as np
import pytest
import torch

import domain_cases as D
import domain_redraw_cases as R
import eval_cases as E
import fresh_reset_cases as F
import helpers as H
import model_cases as M
import post_epilogue_cases as PE
from variant_cases import variant as _variant
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.rodent import RodentTracking

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FALLING = dict(healthy_z_range=(0.0, 0.5))        # tests/test_eval_epilogue.py: envs fall after 7 to 10 steps
FALLING_SOON = dict(healthy_z_range=(0.0, 0.08))  # .. after 1 step, or not within 4


def _rodent(n, lib=None, domain=False, clip=None, **over):
    with H.backend(lib):
        base = RodentTracking(clip or H.reference_clip(), num_envs=n, device=DEV, **dict(H.env_kwargs(), **over))
    return base.with_domain(D.random_domain(base.sys, n, 12)) if domain else base


@pytest.mark.parametrize("num_envs", [1, 63, 64, 65, 257])
def test_standalone_scoring_equals_the_sequential_restatement(num_envs):
    E.check_standalone(_lib.load_library(), DEV, num_envs)


@pytest.mark.parametrize("kernel", ["specialised", "generic", "randomised"])
def test_step_post_eval_equals_the_three_launches_on_every_buffer(kernel):
    make = {"specialised": lambda: _rodent(5), "generic": lambda: _rodent(5, lib=_variant("nospec")),
            "randomised": lambda: _rodent(5, domain=True)}[kernel]
    base = make()
    assert int(base.dims.kernel_specialised) == (0 if kernel == "generic" else 1)
    PE.assert_same(E.direct_case(base, fused=True), E.direct_case(make(), fused=False))


def test_default_evaluation_is_the_same_by_the_generic_the_fused_and_the_graphed_route():
    """3 (a): K = 1 from the first state, episodes of at most 8 steps (the envs fall after 7 to 10); the graph replays 3 steps
    twice and leaves two to the eager tail, and a second evaluation reuses it on a new reset."""
    make = lambda: _rodent(6, **FALLING)  # noqa: E731
    runs = {r: E.evaluator_case(make, DEV, r, episode_length=8, noise="device", graph_steps=3, runs=2) for r in E.ROUTES}
    for r in ("eager", "graphed"):
        E.assert_same_evaluation(runs["generic"], runs[r])
        a, b = E.eval_metrics_of(runs["generic"][2]), E.eval_metrics_of(runs[r][2])
        assert sorted(a) == sorted(b) and all(np.array_equal(E.bits(a[k]), E.bits(b[k])) for k in a), r
    assert set(runs["generic"][0]) == E.DEFAULT_EVAL_KEYS
    rec = runs["graphed"][1]
    assert rec.shape == (6, 12) and (rec[:, 3] == 0).any() and (rec[:, 3] == 1).any()  # fell on their own; were truncated
    assert (runs["graphed"][2]._graph.replays, runs["graphed"][2]._graph.tail) == (2, 2)


def test_several_fresh_episodes_with_domain_ranges_are_the_same_by_all_routes():
    """3 (b): K = 3, fresh auto-reset, episodes of 4 steps, the domain redrawn at every reset; 12 steps = two replays of 5 and
    an eager tail of 2."""
    make = lambda: _rodent(6, clip=F.three_clips(), **FALLING_SOON)  # noqa: E731
    ranges = R.ranges_for(H.model())
    runs = {r: E.evaluator_case(make, DEV, r, K=3, mode="fresh", episode_length=4, ranges=ranges, noise="device", graph_steps=5)
            for r in E.ROUTES}
    for r in ("eager", "graphed"):
        E.assert_same_evaluation(runs["generic"], runs[r])
    m, rec, ev = runs["graphed"]
    assert (ev._graph.replays, ev._graph.tail) == (2, 2)
    assert m["eval/episodes_scored"] == rec.shape[0] and 0 < m["eval/truncated_fraction"] < 1
    assert ((rec[:, 3] == 0) & (rec[:, 2] < 4)).any() and ((rec[:, 3] == 1) & (rec[:, 2] == 4)).any()
    count = ev.state.info["eval_count"].cpu().numpy()
    assert count.max() == 3 and rec.shape[0] == count.sum()
    per_env = np.split(rec, np.cumsum(count)[:-1])
    assert any(len(r) > 1 and len(set(r[:, 0])) > 1 for r in per_env)  # two records of one env differ in start frame


def test_some_env_is_through_while_another_is_still_scored():
    make = lambda: _rodent(6, clip=F.three_clips(), **FALLING_SOON)  # noqa: E731
    _, st, dones, counts = E.unroll_states(make, DEV, K=3, mode="fresh", episode_length=4, T=10, fused=True)
    through = [bool((counts[t] == 3).any() and (counts[t] < 3).any()) for t in range(10)]
    assert any(through), counts
    t0 = through.index(True)
    e = int((counts[t0] == 3).nonzero()[0])
    assert bool(dones[t0 + 1:, e].any()) and int(counts[-1, e]) == 3  # it went on ending episodes, which were not scored


def test_ant_scores_by_the_launch_of_its_own_with_the_switch_on_and_off():
    """3 (c), as on the host build: the generic step kernel, the observation assembled after it, then the two launches."""
    seen = []

    def hook(base):
        orig = base.step

        def step(st, a):
            seen.append(getattr(base, "_eval_desc", None) is not None)
            return orig(st, a)

        base.step = step

    make = lambda: M.ant_env(6, device=DEV, clips=3)  # noqa: E731
    runs = []
    for on in (True, False):
        with E.eval_epilogue(on):
            runs.append(E.evaluator_case(make, DEV, "eager", K=2, mode="fresh", episode_length=3, hook=hook))
    E.assert_same_evaluation(*runs)
    E.assert_same_evaluation(runs[0], E.evaluator_case(make, DEV, "generic", K=2, mode="fresh", episode_length=3))
    assert seen == [False] * 12 and runs[0][1].shape == (12, 12) and bool((runs[0][1][:, 3] == 1).all())


def test_fresh_records_carry_the_draws_of_the_reset_that_began_them():
    E.check_fresh_records(lambda: _rodent(67, clip=F.three_clips(), **FALLING_SOON), DEV, fused=True)


def test_validation_names_the_field_and_launches_nothing():
    E.check_validation(_rodent(3))
