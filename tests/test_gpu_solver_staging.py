"""The staged solver constants on the device (csrc/vnl_body.h: EnvWaveT::load_tables / with_solve_regs): the product library
against the regression build that reads them from global memory as before (csrc/build.py --plain).  Same values from another
place: every output bit for bit."""
import numpy as np
import pytest

import model_cases as M
import variant_cases as V

pytestmark = pytest.mark.gpu
B = 256
STEPS = 3


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_staged_constants_change_no_bit_on_the_device(solver):
    """Rodent CG 6 / 6 (specialised kernels) and Newton 1 / 4 (generic kernels), reset + three control steps."""
    kw = {"model": M.newton_model(1, 4)} if solver == "newton" else {}
    outs = []
    for lib in (None, V.variant("plain")):
        env = V.rodent(B, lib, **kw)
        assert int(env.dims.kernel_specialised) == (1 if solver == "cg" else 0)
        outs.append(V.rollout(env, B, STEPS))
    V.same(outs[0], outs[1], solver, STEPS, finite=False)


def test_staged_friction_of_a_randomised_env_changes_no_bit():
    """Per-env friction (the randomised instantiation): what make_constraint stages is this env's own value."""
    n = 64
    outs = [V.rollout(V.rodent(n, lib, V.friction), n, STEPS) for lib in (None, V.variant("plain"))]
    V.same(outs[0], outs[1], "friction domain", STEPS, finite=False)


def test_inputs_cover_the_one_row_per_lane_line_search_routes():
    """The inputs above reach both routes of the one-row-per-lane line search at every step: at least 200 of the 256 envs have at
    most 16 live constraint rows (all in one DPP row), at least 5 have 17 .. 64, none more than 64 (the float32 host build
    gives 232-243 and 13-24).  Read from a debug-enabled env of the product library."""
    env = V.rodent(B, None)
    env.debug(2)
    ncon = int(env.sys.scalars["ncon"])
    counts = []

    def live(e):
        raw = np.ascontiguousarray(e.scratch("act_list").cpu().numpy()).view(np.int32)
        counts.append(raw[:, (ncon + 3) // 4 + 1].copy())

    V.rollout(env, B, STEPS, each=live)
    assert len(counts) == 4
    for t, nl in enumerate(counts):
        few, mid, many = int((nl <= 16).sum()), int(((nl > 16) & (nl <= 64)).sum()), int((nl > 64).sum())
        print(f"step {t}: <= 16 rows {few}, 17..64 {mid}, > 64 {many}")
        assert few >= 200 and mid >= 5 and many == 0, (t, few, mid, many)


def test_rodent_keeps_eight_workgroups_per_cu():
    env = V.rodent(8, None)
    assert int(env.dims.workspace_floats_per_env) * 4 <= 20480
    assert int(env.dims.workgroups_per_cu) == 8
