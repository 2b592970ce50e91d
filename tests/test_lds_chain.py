"""Serial LDS round trips taken out of a substep (csrc/vnl_body.h): blk_apply runs the trips of a product in phases (every
trip's index reads and the writers' operands, then every trip's gathers, then the sums, then the writes), factor_aba's pivot
block writes only the line its ancestors wait for and leaves V = U / D and 1/D1 to one pass after the step loop, its lane sets
request their lines before either absorbs, and the solver accumulates qg1 / qg2 and the Gauss term in the loops that produce
their operands.  The same operations on the same operands in another order of issue: a build with the former forms
(-DVNL_LDS_PLAIN, the `ldsplain` variant of csrc/build.py) must give the same bits on every output.

What this file covers: the host simulation (one 'lane', 64 row sets), so the phase form's two-trip windows on the one-, two-
and three-trip tables of the models, the `in != out` assertions of the products, the deferred V / 1/D1 pass, the Newton route's
product on the Hessian image and the solver scalars where grad / search / mv are visible (debug image).  Lane-parallel
behaviour is covered by tests/test_gpu_lds_chain.py."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import test_solver_tail as T
import test_vmem_schedule as V
from vnl_brax_imitation_amd import _lib

STEPS = 2


@functools.lru_cache(maxsize=None)
def _plain_library(real):
    src = os.path.join(H.ROOT, "vnl-brax-imitation_amd", "csrc")
    out = os.path.join(H.ROOT, "tests", "hostsim", "_build", f"libvnl_hostsim_{real}_ldsplain.so")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(H.ROOT, "include", "vnl.h"), os.path.join(H.ROOT, "tests", "hostsim", "stub", "hip", "hip_runtime.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", f"-DVNL_REAL={real}", "-DVNL_LDS_PLAIN",
                               "-I" + os.path.join(H.ROOT, "tests", "hostsim", "stub"), "-x", "c++",
                               os.path.join(src, "vnl_lib.hip"), "-o", out])
    return _lib.load_library(out, env_only=True)


# (model, envs): the rodent CG 6 / 6 (both lane sets, the factor pair, two-trip tables), the ant under RodentTracking's glue
# (single set, factor_lds, euler's own factorisation), the humanoid, and the rodent Newton 1 / 4 (solve_inplace on the Hessian)
CASES = {"rodent_cg_6_6": (T.MODELS["rodent_cg_6_6"], 8), "ant_rodent_tracking": (V._ant_as_rodent_tracking, 8),
         "humanoid": (T.MODELS["humanoid"], 4), "rodent_newton_1_4": (T.MODELS["rodent_newton_1_4"], 4)}


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
def test_lds_round_trips_taken_out_change_no_bit(name, real):
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


@pytest.mark.parametrize("real", ["float", "double"])
def test_debug_image_is_the_same_with_the_solver_scalars_in_their_producing_loops(real):
    """With the debug image on the solver runs every iteration in full and records its line searches: the trace and the
    solver's vectors (grad / Mgrad / search / mv: what qg1, qg2 and the Gauss term are made of) must be the same bits."""
    dtype = torch.float64 if real == "double" else torch.float32
    imgs = []
    for lib in (H.hostsim_library(real), _plain_library(real)):
        with H.backend(lib, dtype):
            env, _ = T.MODELS["rodent_cg_6_6"](2)
        env.debug(True)
        env.reset(5)
        img = {k: env.scratch(k).clone() for k in ("grad", "Mgrad", "search", "mv", "Ma", "qacc", "qfrc_constraint")}
        img["solver_trace"] = env.solver_trace().clone()
        imgs.append(img)
    for k in imgs[0]:
        assert torch.equal(imgs[0][k], imgs[1][k]), k
    assert imgs[0]["search"].abs().sum() > 0 and int(imgs[0]["solver_trace"][:, 0, 1].min()) >= 1  # (iterations ran)
