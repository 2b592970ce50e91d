"""Recorded rollouts on the device (the cases of tests/record_cases.py through the C-ABI of the product library):
vnl_env_record against the NumPy restatement at 5 and 70 envs, its validation, acting.RolloutRecorder through the generic
loop, the fused eager loop and the captured graph (two replays of 5 steps and a tail of 2) against a plain loop that clones
the same tensors, the torch restatement against the kernel, the replay of recorded latents, and Evaluator with a recorder by
every route."""
import functools

import pytest
import torch

import helpers as H
import record_cases as RC
from vnl_brax_imitation_amd.envs.rodent import RodentTracking

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rodent(n=RC.B_ROD, clip=None, **over):
    return lambda: RodentTracking(clip or H.reference_clip(), num_envs=n, device=DEV, **dict(H.env_kwargs(), **over))


@pytest.mark.parametrize("num_envs", [5, 70])
def test_standalone_recording_equals_the_sequential_restatement(num_envs):
    RC.check_standalone(_rodent(num_envs, clip=RC.two_clips())())


def test_validation_names_the_field_and_writes_nothing():
    RC.check_validation(_rodent(3)())


@functools.lru_cache(maxsize=None)
def _clone_loop(mode, kind):
    return RC.clone_loop(_rodent(), DEV, mode, kind)


@pytest.mark.parametrize("route", ["generic", "eager", "graphed"])
@pytest.mark.parametrize("mode,kind", [("first_state", "full"), ("fresh", "full"), ("fresh", "decoder"), ("first_state", "decoder")])
def test_recorder_equals_the_clone_loop(mode, kind, route):
    rows, base = _clone_loop(mode, kind)
    _, out = RC.recorded_case(_rodent(), DEV, mode, kind, route)
    RC.check_against_clone_loop(rows, base, out)
    RC.check_terminal_rows(out, mode)
    if kind == "decoder":
        assert "latent" in out.columns and out.latent.shape == (RC.B_ROD, RC.T_ROD + 1, 16)


@pytest.mark.parametrize("route", ["eager", "graphed"])
@pytest.mark.parametrize("mode", ["first_state", "fresh"])
def test_recorder_stops_at_done_and_follows_its_env_index(mode, route):
    rows, base = _clone_loop(mode, "full")
    idx = [5, 0, -1, 5, RC.B_ROD, 2]
    _, out = RC.recorded_case(_rodent(), DEV, mode, "full", route, stop_at_done=True, env_index=idx)
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


@pytest.mark.parametrize("route", ["generic", "eager", "graphed"])
def test_evaluator_records_two_envs_and_scores_as_without(route, tmp_path):
    ev = RC.check_evaluator(_rodent(6, **RC.FALLING), DEV, route, tmp_path, graph_steps=2)
    if route == "graphed":
        assert (ev._graph.replays, ev._graph.tail) == (2, 1)
