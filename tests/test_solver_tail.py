"""The solver's last permitted iteration stops after constraint_force() (EnvWave::solve, csrc/vnl_body.h): its Gauss term,
cost, gradient, M^-1 grad (Newton: Hessian assembly + factorisation + inversion) and search update feed nothing -- the loop
cannot run again, and what follows reads only qacc and qfrc_constraint.  A host build of the same sources with the tail
forced back in (-DVNL_SOLVER_TAIL, the `tail` variant of csrc/build.py) must give the same bits on every output."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.model import mjcf

STEPS = 4  # control steps (the issue asks for at least 3), each of several substeps = several full-length solves


@functools.lru_cache(maxsize=None)
def _tail_library(real):
    src = os.path.join(H.ROOT, "vnl-brax-imitation_amd", "csrc")
    out = os.path.join(H.ROOT, "tests", "hostsim", "_build", f"libvnl_hostsim_{real}_tail.so")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(H.ROOT, "include", "vnl.h"), os.path.join(H.ROOT, "tests", "hostsim", "stub", "hip", "hip_runtime.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", f"-DVNL_REAL={real}", "-DVNL_SOLVER_TAIL",
                               "-I" + os.path.join(H.ROOT, "tests", "hostsim", "stub"), "-x", "c++",
                               os.path.join(src, "vnl_lib.hip"), "-o", out])
    return _lib.load_library(out, env_only=True)


def _rodent(solver):
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    def make(B):
        kw = H.env_kwargs()
        if solver == "newton":
            m = copy.deepcopy(H.model())
            m.scalars.update(solver_newton=1, iterations=1, ls_iterations=4)
            kw["model"] = m
        return RodentTracking(H.reference_clip(), num_envs=B, device="cpu", **kw), 30
    return make


def _ant(B):
    import test_ant_env as A
    from vnl_brax_imitation_amd import envs

    m = mjcf.CompiledModel.load(A.ANT_NPZ)
    return envs.get_environment("ant", params=A.PARAMS, clip_length=60, episode_length=20, reference_clip=A._clip(m), model=m,
                                num_envs=B, device="cpu"), 8


def _humanoid(B):
    import test_humanoid as Hu
    from vnl_brax_imitation_amd.envs.humanoid import HumanoidTracking

    m = Hu._model()
    return HumanoidTracking(Hu.PARAMS, clip_length=60, episode_length=20, reference_clip=Hu._clip(m), model=m, num_envs=B,
                            device="cpu"), 21


MODELS = {"rodent_cg_6_6": _rodent("cg"), "rodent_newton_1_4": _rodent("newton"), "ant": _ant, "humanoid": _humanoid}


def _outputs(st):
    out = {"obs": st.obs, "reward": st.reward, "done": st.done}
    out.update({"ps." + n: st.pipeline_state.raw(n) for n in st.pipeline_state._FIELDS})
    out.update({"info." + k: v for k, v in st.info.items() if torch.is_tensor(v)})
    out.update({"metrics." + k: v for k, v in st.metrics.items()})
    return {k: v.clone() for k, v in out.items()}


def _rollout(library, real, make, B):
    dtype = torch.float64 if real == "double" else torch.float32
    with H.backend(library, dtype):
        env, nu = make(B)
    rng = np.random.default_rng(3)
    st = env.reset(5)
    snaps = [_outputs(st)]
    for _ in range(STEPS):
        act = torch.from_numpy(np.clip(0.3 * rng.standard_normal((B, nu)), -1, 1)).to(dtype)
        st = env.step(st, act)
        snaps.append(_outputs(st))
    return env, snaps


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(MODELS))
def test_skipped_tail_of_the_last_solver_iteration_changes_no_bit(name, real):
    B = 4
    env, skip = _rollout(H.hostsim_library(real), real, MODELS[name], B)
    _, full = _rollout(_tail_library(real), real, MODELS[name], B)
    # the case is only a test if solves do run to the iteration count (where the tail is skipped): all four do
    assert int(env.sys.scalars["iterations"]) >= 1
    moved = False
    for t, (a, b) in enumerate(zip(skip, full)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (name, real, t, k)
        moved = moved or (t > 0 and not torch.equal(a["ps.qpos"], skip[0]["ps.qpos"]))
    assert moved


def test_debug_image_keeps_the_full_last_iteration():
    """With the debug image on, the solver runs its last iteration in full: the sections grad / Mgrad / search of the image are
    those of the build with the tail forced in, bit for bit (and are not left over from the iteration before)."""
    real = "double"
    imgs = []
    for lib in (H.hostsim_library(real), _tail_library(real)):
        with H.backend(lib, torch.float64):
            env, _ = MODELS["rodent_cg_6_6"](1)
        env.debug(True)
        env.reset(5)
        imgs.append({k: env.scratch(k).clone() for k in ("grad", "Mgrad", "search", "mv", "Ma", "qacc", "qfrc_constraint")})
    for k in imgs[0]:
        assert torch.equal(imgs[0][k], imgs[1][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_skipped_tail_changes_no_bit_on_the_device(solver):
    """The product library against the regression build with the tail forced in (csrc/build.py --tail), 1024 envs, reset + three
    control steps, rodent CG 6 / 6 (specialised kernels) and Newton 1 / 4 (generic kernels): every output bit for bit."""
    from vnl_brax_imitation_amd.csrc import build as hip_build
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    B = 1024
    rng = np.random.default_rng(9)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((B, 74))).astype(np.float32)
    acts = np.clip(0.3 * rng.standard_normal((3, B, 30)), -1, 1).astype(np.float32)
    kw = H.env_kwargs()
    if solver == "newton":
        kw["model"] = copy.deepcopy(H.model())
        kw["model"].scalars.update(solver_newton=1, iterations=1, ls_iterations=4)
    outs = []
    for lib in (None, _lib.load_library(hip_build.build(variant="tail"))):
        with H.backend(lib):
            env = RodentTracking(H.reference_clip(), num_envs=B, device="cuda:0", **kw)
        st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
        snaps = [_outputs(st)]
        for a in acts:
            st = env.step(st, torch.from_numpy(a))
            snaps.append(_outputs(st))
        outs.append(snaps)
    for t, (a, b) in enumerate(zip(*outs)):
        for k in a:
            assert torch.equal(a[k], b[k]), (solver, t, k)
    assert not torch.equal(outs[0][-1]["ps.qpos"], outs[0][0]["ps.qpos"])
