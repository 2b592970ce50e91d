"""The vector-memory accesses of a substep outside the solver loop, taken off the critical path (csrc/vnl_body.h): factor_aba
loads its schedule as 32-bit words (four steps each, one word ahead in registers) and stores 1/D2 once after its loop, euler()
reloads the second inverse factor four elements at a time with every load requested before the first LDS write, forward()
reads the warm start into LO(qacc) directly and skips the copy of LO(qacc) onto itself on the later substeps.  Pure data
movement: a build with the former accesses (-DVNL_VMEM_PLAIN, the `vmemplain` variant of csrc/build.py) must give the same bits
on every output.

What this file covers: the host simulation (one 'lane', 64 row sets), so the word walk, the deferred store, the padded rows of
fac_match / fac2 and the reload's bounds.  Lane-parallel behaviour is covered by tests/test_gpu_vmem_schedule.py."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import hostsim_cases as HC
from vnl_brax_imitation_amd import _lib

STEPS = 2
FAC_LINES = 6  # csrc/vnl_types.h: VNL_FAC_LINES

# (model, envs): the rodent CG 6 / 6 (both lane sets, the factor pair), the ant (single set, factor_lds), the humanoid
CASES = {"rodent_cg_6_6": (HC.MODELS["rodent_cg_6_6"], 8), "ant_rodent_tracking": (HC.ant_as_rodent_tracking, 8),
         "humanoid": (HC.MODELS["humanoid"], 4)}


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(CASES))
def test_vector_memory_schedule_changes_no_bit(name, real):
    make, B = CASES[name]
    _, new = HC.host_rollout(H.hostsim_library(real), real, make, B, STEPS)
    _, old = HC.host_rollout(H.hostsim_library(real, "vmemplain"), real, make, B, STEPS)
    HC.same_rollouts(new, old, (name, real), equal=HC.equal_with_nan)


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
