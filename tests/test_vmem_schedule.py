"""The vector-memory accesses of a substep outside the solver loop, taken off the critical path (csrc/vnl_body.h): factor_aba
loads its schedule as 32-bit words (four steps each, one word ahead in registers) and stores 1/D2 once after its loop, euler()
reloads the second inverse factor four elements at a time with every load requested before the first LDS write, forward()
reads the warm start into LO(qacc) directly and skips the copy of LO(qacc) onto itself on the later substeps.  Pure data
movement: a build with the former accesses (-DVNL_VMEM_PLAIN, the `vmemplain` variant of csrc/build.py) must give the same bits
on every output.

What this file covers: the host simulation (one 'lane', 64 row sets), so the word walk, the deferred store, the padded rows of
fac_match / fac2 and the reload's bounds.  Lane-parallel behaviour is covered by tests/test_gpu_vmem_schedule.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import test_solver_tail as T
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.model import mjcf
from vnl_brax_imitation_amd.preprocessing import mjx_preprocess as P

STEPS = 2
FAC_LINES = 6  # csrc/vnl_types.h: VNL_FAC_LINES


@functools.lru_cache(maxsize=None)
def _plain_library(real):
    src = os.path.join(H.ROOT, "vnl-brax-imitation_amd", "csrc")
    out = os.path.join(H.ROOT, "tests", "hostsim", "_build", f"libvnl_hostsim_{real}_vmemplain.so")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(H.ROOT, "include", "vnl.h"), os.path.join(H.ROOT, "tests", "hostsim", "stub", "hip", "hip_runtime.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", f"-DVNL_REAL={real}", "-DVNL_VMEM_PLAIN",
                               "-I" + os.path.join(H.ROOT, "tests", "hostsim", "stub"), "-x", "c++",
                               os.path.join(src, "vnl_lib.hip"), "-o", out])
    return _lib.load_library(out, env_only=True)


def _ant_as_rodent_tracking(B):
    """The ant (nv 14) under RodentTracking's glue, as in tests/test_generic_model.py: no factor pair, euler() factorises
    M + h D itself through factor_lds."""
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    m = mjcf.CompiledModel.load(os.path.join(H.ROOT, "vnl-brax-imitation_amd", "data", "ant.npz"))
    n = 40
    t = np.arange(n)[:, None] * 0.02
    qpos = np.zeros((n, 15))
    qpos[:, 2], qpos[:, 3] = 0.55, 1.0
    qpos[:, 0] = 0.2 * t[:, 0]
    qpos[:, 7:] = np.array([0.0, 1.0, 0.0, -1.0, 0.0, -1.0, 0.0, 1.0]) + 0.15 * np.sin(2 * np.pi * 1.5 * t + np.arange(8))
    clip = P.process_qpos(m, qpos, max_qvel=20.0, dt=0.02)
    aux = ["aux_1", "aux_2", "aux_3", "aux_4"]
    env = RodentTracking(clip, end_eff_names=aux, appendage_names=aux + ["torso"],
                         walker_body_names=[b for b in m.names["body"] if b != "world"], joint_names=m.names["joint"][1:],
                         center_of_mass="torso", model=m, clip_length=n, sub_clip_length=10, ref_traj_length=5,
                         healthy_z_range=(0.2, 1.0), num_envs=B, device="cpu")
    return env, 8


# (model, envs): the rodent CG 6 / 6 (both lane sets, the factor pair), the ant (single set, factor_lds), the humanoid
CASES = {"rodent_cg_6_6": (T.MODELS["rodent_cg_6_6"], 8), "ant_rodent_tracking": (_ant_as_rodent_tracking, 8),
         "humanoid": (T.MODELS["humanoid"], 4)}


def _rollout(library, real, make, B):
    dtype = torch.float64 if real == "double" else torch.float32
    with H.backend(library, dtype):
        env, nu = make(B)
    rng = np.random.default_rng(3)
    st = env.reset(5)
    snaps = [T._outputs(st)]
    for _ in range(STEPS):
        act = torch.from_numpy(np.clip(0.3 * rng.standard_normal((B, nu)), -1, 1)).to(dtype)
        st = env.step(st, act)
        snaps.append(T._outputs(st))
    return env, snaps


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(CASES))
def test_vector_memory_schedule_changes_no_bit(name, real):
    make, B = CASES[name]
    _, new = _rollout(H.hostsim_library(real), real, make, B)
    _, old = _rollout(_plain_library(real), real, make, B)
    moved = False
    for t, (a, b) in enumerate(zip(new, old)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k].numpy(), b[k].numpy(), equal_nan=True), (name, real, t, k)
        moved = moved or (t > 0 and not torch.equal(a["ps.qpos"], new[0]["ps.qpos"]))
    assert moved


def _schedule(par):
    """The factorisation schedule restated from the dof tree (csrc/vnl_lib.hip, build_dev_model): fac_match[a][t], bit k set
    where the pivot of step t in scratch line k lies strictly below row a."""
    nv = len(par)
    ftime, fslot, count = [0] * nv, [0] * nv, []
    for j in range(nv - 1, -1, -1):
        t = max([ftime[i] + 1 for i in range(j + 1, nv) if par[i] == j], default=0)
        while len(count) <= t:
            count.append(0)
        while count[t] >= FAC_LINES:
            t += 1
            if len(count) <= t:
                count.append(0)
        ftime[j], fslot[j] = t, count[t]
        count[t] += 1
    match = np.zeros((nv, len(count)), dtype=np.uint8)
    for j in range(nv):
        a = par[j]
        while a >= 0:
            match[a, ftime[j]] |= 1 << fslot[j]
            a = par[a]
    return match


def _schedule_words(env):
    """[nv][words] uint32: the table as factor_aba loads it (vnl_env_scratch "fac_match")."""
    ptr, cnt = C.c_void_p(), C.c_int32()
    _lib.check(env._L, env._L.vnl_env_scratch(env._env_h, b"fac_match", C.byref(ptr), C.byref(cnt)))
    nv = int(env.dims.nv)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(nv, cnt.value)).copy()


@pytest.mark.parametrize("name", ["rodent_cg_6_6", "humanoid", "ant_rodent_tracking"])
def test_packed_schedule_words_reproduce_fac_match(name):
    make, _ = CASES[name]
    with H.hostsim_backend("float"):
        env, _ = make(1)
    want = _schedule([int(p) for p in np.asarray(env.sys.dof_parentid)])
    nv, nsteps = want.shape
    words = _schedule_words(env)
    assert words.shape == (nv, (nsteps + 3) // 4)
    # the kernel's walk: step s is byte s & 3 of word s >> 2, taken by `& 0xff` and `>>= 8`
    got = np.stack([(words[:, s >> 2] >> (8 * (s & 3))) & 0xFF for s in range(nsteps)], axis=1).astype(np.uint8)
    assert np.array_equal(got, want)
    # .. which is the table byte for byte, and the padding of a row absorbs nothing
    raw = words.view(np.uint8).reshape(nv, -1)
    assert np.array_equal(raw[:, :nsteps], want) and not raw[:, nsteps:].any()
    assert want.any()


def test_cases_cover_a_schedule_that_is_no_multiple_of_four_steps():
    steps = {}
    for name in ("rodent_cg_6_6", "humanoid", "ant_rodent_tracking"):
        with H.hostsim_backend("float"):
            env, _ = CASES[name][0](1)
        steps[name] = _schedule([int(p) for p in np.asarray(env.sys.dof_parentid)]).shape[1]
    assert steps["rodent_cg_6_6"] == 36
    assert any(n % 4 for n in steps.values()), steps
