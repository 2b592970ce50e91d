"""The staged solver constants on the device (csrc/vnl_body.h: EnvWaveT::load_tables / with_solve_regs): the product library
against the regression build that reads them from global memory as before (csrc/build.py --plain).  Same values from another
place: every output bit for bit."""
import copy
import functools

import numpy as np
import pytest
import torch

import domain_cases as D
import helpers as H
import test_solver_tail as T
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.rodent import RodentTracking

pytestmark = pytest.mark.gpu
B = 256


@functools.lru_cache(maxsize=None)
def _plain():
    from vnl_brax_imitation_amd.csrc import build as hip_build

    return _lib.load_library(hip_build.build(variant="plain"))


@functools.lru_cache(maxsize=None)
def _inputs(n=B):
    """The inputs of tests/test_solver_tail.py's device test at this size."""
    rng = np.random.default_rng(9)
    sf = rng.integers(0, 235, n).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((n, 74))).astype(np.float32)
    acts = np.clip(0.3 * rng.standard_normal((3, n, 30)), -1, 1).astype(np.float32)
    return sf, noise, acts


def _kwargs(solver):
    kw = H.env_kwargs()
    if solver == "newton":
        kw["model"] = copy.deepcopy(H.model())
        kw["model"].scalars.update(solver_newton=1, iterations=1, ls_iterations=4)
    return kw


def _rollout(env, n=B, each=None):
    sf, noise, acts = _inputs(n)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    snaps = [T._outputs(st)]
    if each:
        each(env)
    for a in acts:
        st = env.step(st, torch.from_numpy(a))
        snaps.append(T._outputs(st))
        if each:
            each(env)
    return snaps


def _same(a_snaps, b_snaps, tag):
    for t, (a, b) in enumerate(zip(a_snaps, b_snaps)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (tag, t, k)
    assert not torch.equal(a_snaps[-1]["ps.qpos"], a_snaps[0]["ps.qpos"])


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_staged_constants_change_no_bit_on_the_device(solver):
    """Rodent CG 6 / 6 (specialised kernels) and Newton 1 / 4 (generic kernels), reset + three control steps."""
    outs = []
    for lib in (None, _plain()):
        with H.backend(lib):
            env = RodentTracking(H.reference_clip(), num_envs=B, device="cuda:0", **_kwargs(solver))
        assert int(env.dims.kernel_specialised) == (1 if solver == "cg" else 0)
        outs.append(_rollout(env))
    _same(outs[0], outs[1], solver)


def test_staged_friction_of_a_randomised_env_changes_no_bit():
    """Per-env friction (the randomised instantiation): what make_constraint stages is this env's own value."""
    n = 64
    outs = []
    for lib in (None, _plain()):
        with H.backend(lib):
            base = RodentTracking(H.reference_clip(), num_envs=n, device="cuda:0", **H.env_kwargs())
            env = base.with_domain({"cg_friction": D.random_domain(base.sys, n, 21)["cg_friction"]})
        outs.append(_rollout(env, n))
    _same(outs[0], outs[1], "friction domain")


def test_inputs_cover_the_one_row_per_lane_line_search_routes():
    """The inputs above reach both routes of the one-row-per-lane line search at every step: at least 200 of the 256 envs have at
    most 16 live constraint rows (all in one DPP row), at least 5 have 17 .. 64, none more than 64 (the float32 host build
    gives 232-243 and 13-24).  Read from a debug-enabled env of the product library."""
    env = RodentTracking(H.reference_clip(), num_envs=B, device="cuda:0", **H.env_kwargs())
    env.debug(2)
    ncon = int(env.sys.scalars["ncon"])
    counts = []

    def live(e):
        raw = np.ascontiguousarray(e.scratch("act_list").cpu().numpy()).view(np.int32)
        counts.append(raw[:, (ncon + 3) // 4 + 1].copy())

    _rollout(env, each=live)
    assert len(counts) == 4
    for t, nl in enumerate(counts):
        few, mid, many = int((nl <= 16).sum()), int(((nl > 16) & (nl <= 64)).sum()), int((nl > 64).sum())
        print(f"step {t}: <= 16 rows {few}, 17..64 {mid}, > 64 {many}")
        assert few >= 200 and mid >= 5 and many == 0, (t, few, mid, many)


def test_rodent_keeps_eight_workgroups_per_cu():
    env = RodentTracking(H.reference_clip(), num_envs=8, device="cuda:0", **H.env_kwargs())
    assert int(env.dims.workspace_floats_per_env) * 4 <= 20480
    assert int(env.dims.workgroups_per_cu) == 8
