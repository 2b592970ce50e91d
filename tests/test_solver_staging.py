"""What the solver loop looks up per lane no longer comes from global memory (csrc/vnl_body.h): the contact / limit-row index
tables and this substep's friction are staged in LDS (EnvWaveT::load_tables, make_constraint), the block descriptors of the
M^-1 products and dof_limrow sit in registers (EnvWaveT::with_solve_regs).  The values are the same, so a build with the
former reads (-DVNL_SOLVER_PLAIN, the `plain` variant of csrc/build.py) must give the same bits on every output.

What this file covers: the LDS tables and the staged friction only.  The register part is device code (VNL_SOLVE_REGS is 0 in a
host build, which reads blk_tab and dof_limrow where they are): `with_solve_regs`, `limrow_of` and the `sr.blk` path of
`blk_apply` are covered by tests/test_gpu_solver_staging.py alone."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import domain_cases as D
import helpers as H
import test_solver_tail as T
from vnl_brax_imitation_amd import _lib

STEPS = 4
B = 4


@functools.lru_cache(maxsize=None)
def _plain_library(real):
    src = os.path.join(H.ROOT, "vnl-brax-imitation_amd", "csrc")
    out = os.path.join(H.ROOT, "tests", "hostsim", "_build", f"libvnl_hostsim_{real}_plain.so")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(H.ROOT, "include", "vnl.h"), os.path.join(H.ROOT, "tests", "hostsim", "stub", "hip", "hip_runtime.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", f"-DVNL_REAL={real}", "-DVNL_SOLVER_PLAIN",
                               "-I" + os.path.join(H.ROOT, "tests", "hostsim", "stub"), "-x", "c++",
                               os.path.join(src, "vnl_lib.hip"), "-o", out])
    return _lib.load_library(out, env_only=True)


def _rodent_friction(n):
    """A rodent whose envs each have their own friction (the randomised instantiation: friction staged per env)."""
    env, nu = T.MODELS["rodent_cg_6_6"](n)
    dom = D.random_domain(env.sys, n, 21)
    return env.with_domain({"cg_friction": dom["cg_friction"]}), nu


MODELS = dict(T.MODELS, rodent_friction_domain=_rodent_friction)


def _rollout(library, real, make):
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
@pytest.mark.parametrize("name", list(MODELS))
def test_staged_solver_constants_change_no_bit(name, real):
    _, staged = _rollout(H.hostsim_library(real), real, MODELS[name])
    _, plain = _rollout(_plain_library(real), real, MODELS[name])
    moved = False
    for t, (a, b) in enumerate(zip(staged, plain)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (name, real, t, k)
        moved = moved or (t > 0 and not torch.equal(a["ps.qpos"], staged[0]["ps.qpos"]))
    assert moved


def test_rodent_layout_keeps_eight_workgroups_per_cu():
    """160 KB of LDS per CU / 8 workgroups = 20,480 B per env (float32)."""
    env = H.hostsim_env(1)
    assert int(env.dims.workspace_floats_per_env) * 4 <= 20480, int(env.dims.workspace_floats_per_env)


def test_staged_sections_are_readable_by_name():
    """The new LDS sections through env.scratch, against the model they were filled from."""
    env = H.hostsim_env(2)
    env.debug(True)
    env.reset(5)
    m = env.sys
    ncon, ncg, nlimit = (int(m.scalars[k]) for k in ("ncon", "ncg", "nlimit"))

    def raw(name, dtype):
        return np.ascontiguousarray(env.scratch(name).numpy()).view(dtype)

    mu = env.scratch("con_mu").numpy()
    assert mu.shape == (2, ncg)
    assert np.array_equal(mu[0], np.asarray(m.cg_friction)[:, 0].astype(np.float32)) and np.array_equal(mu[0], mu[1])
    con = raw("tab_con", np.uint8)[0, :2 * ncon].reshape(ncon, 2)
    conadr, cn = np.asarray(m.cg_conadr), np.asarray(m.cg_ncon)
    geom = np.concatenate([np.full(cn[g], g) for g in np.argsort(conadr, kind="stable")])
    assert np.array_equal(con[:, 0], geom)                      # the geom of every contact ..
    # .. and the contacts in the order of their DYNAMIC bodies (a welded body rides on its nearest jointed ancestor)
    parent, jntnum = np.asarray(m.body_parentid), np.asarray(m.body_jntnum)

    def dyn(b):
        while b > 0 and jntnum[b] == 0:
            b = parent[b]
        return int(b)

    cbody = np.array([dyn(int(np.asarray(m.cg_bodyid)[g])) for g in geom])
    assert np.array_equal(con[:, 1], np.argsort(cbody, kind="stable"))
    lim = raw("tab_lim", np.uint8)[0, :nlimit]
    hinge_limited = [j for j in range(int(m.scalars["njnt"])) if m.jnt_limited[j] and m.jnt_type[j] == 3]
    assert np.array_equal(lim, np.asarray(m.jnt_dofadr)[hinge_limited])
    # the runs of consecutive dofs on the path root -> body of every contact: begin | end << 8, unused runs 0
    dofadr, dofnum, dpar = np.asarray(m.body_dofadr), np.asarray(m.body_dofnum), np.asarray(m.dof_parentid)
    want = []
    for b in cbody:
        path, d = [], (int(dofadr[b] + dofnum[b] - 1) if dofnum[b] > 0 else -1)
        while d >= 0:
            path.append(d)
            d = int(dpar[d])
        path.sort()
        runs, k = [], 0
        while k < len(path):
            j = k
            while j + 1 < len(path) and path[j + 1] == path[j] + 1:
                j += 1
            runs.append(path[k] | ((path[j] + 1) << 8))
            k = j + 1
        want.append(runs)
    nruns = max(len(r) for r in want)
    want = np.array([r + [0] * (nruns - len(r)) for r in want], dtype=np.uint16)
    assert np.array_equal(raw("tab_path", np.uint16)[0, :ncon * nruns].reshape(ncon, nruns), want)
