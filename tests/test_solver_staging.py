"""What the solver loop looks up per lane no longer comes from global memory (csrc/vnl_body.h): the contact / limit-row index
tables and this substep's friction are staged in LDS (EnvWaveT::load_tables, make_constraint), the block descriptors of the
M^-1 products and dof_limrow sit in registers (EnvWaveT::with_solve_regs).  The values are the same, so a build with the
former reads (-DVNL_SOLVER_PLAIN, the `plain` variant of csrc/build.py) must give the same bits on every output.

What this file covers: the LDS tables and the staged friction only.  The register part is device code (VNL_SOLVE_REGS is 0 in a
host build, which reads blk_tab and dof_limrow where they are): `with_solve_regs`, `limrow_of` and the `sr.blk` path of
`blk_apply` are covered by tests/test_gpu_solver_staging.py alone."""
import numpy as np
import pytest

import helpers as H
import hostsim_cases as HC

STEPS = 4
B = 4
MODELS = dict(HC.MODELS, rodent_friction_domain=HC.rodent_friction)


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(MODELS))
def test_staged_solver_constants_change_no_bit(name, real):
    # (env and rollout inside the backend: the friction case's with_domain must bind to the same library)
    _, staged = HC.host_rollout(H.hostsim_library(real), real, MODELS[name], B, STEPS, step_in_backend=True)
    _, plain = HC.host_rollout(H.hostsim_library(real, "plain"), real, MODELS[name], B, STEPS, step_in_backend=True)
    HC.same_rollouts(staged, plain, (name, real))


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
