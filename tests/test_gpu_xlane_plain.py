"""Cross-lane glue of the step kernel in fewer issue slots (csrc/vnl_body.h, vnl_rows_join / VNL_WAVE_SUMS / VNL_SCAN6: each
row_bcast step of a wave sum or scan one masked v_add_f32_dpp, several values through that stage together; dof_prefix: the last
trip of at most 16 dofs as two in-row scans): the product library against the regression build with the former forms
(csrc/build.py --xlaneplain).  The same adds on the same operands in the same order: every output bit for bit."""
import functools

import numpy as np
import pytest

import variant_cases as V

pytestmark = pytest.mark.gpu
STEPS = 3
N = 128  # 128 envs: the rodent's 73 dofs take both trips of every carried scan, the second one in the tail form
TRACE_ROWS = 8 + 64 * 8  # csrc/vnl_types.h VNL_TRACE_ROWS: then 16 ints, bit r set = constraint row r exists (D != 0)
FEW = 16  # the line search's short path: at most this many existing rows, one per lane of a DPP row


def _old():
    return V.variant("xlaneplain")


def _existing_rows(env):
    """(envs, solver calls of the last reset / step): number of existing constraint rows, from the debug trace's row bits."""
    bits = env.solver_trace()[..., TRACE_ROWS:TRACE_ROWS + 16].numpy().astype(np.uint32)
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=-1).sum(-1)


@functools.lru_cache(maxsize=None)
def _rows_of_the_rodent_inputs():
    """Existing rows per env and solver call over the rollout the tests below compare, from a debug run of the regression
    build (of the reset's trace, the one solver call it makes)."""
    env = V.rodent(N, _old())
    env.debug(True)
    rows = []
    V.rollout(env, N, STEPS, each=lambda e: rows.append(_existing_rows(e)))
    return np.concatenate([rows[0][:, :1]] + rows[1:], axis=1)


def test_the_inputs_take_both_line_search_paths():
    """The short path (at most 16 existing rows: the in-row butterfly alone) and the long one (more: the nine sums through
    vnl_rows_join) are both taken by the solver calls of the rollout the tests below compare."""
    rows = _rows_of_the_rodent_inputs()
    print(f"existing rows per env and solver call: min {rows.min()} max {rows.max()}; envs with a call of <= {FEW}: "
          f"{int((rows <= FEW).any(1).sum())}, of more: {int((rows > FEW).any(1).sum())}")
    assert ((rows <= FEW) & (rows > 0)).any(1).sum() >= 1 and (rows > FEW).any(1).sum() >= 1


@pytest.mark.parametrize("domain", [None, V.damping_armature], ids=["plain", "with_domain"])
def test_cross_lane_forms_change_no_bit_on_the_rodent(domain):
    """128 envs, the specialised kernels (CG 6 / 6) and their randomised instantiation (VnlSpecDom): both trips of every
    carried scan, the tail form as a compile-time fact."""
    new, old = V.rodent(N, None, domain), V.rodent(N, _old(), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(new, N, STEPS), V.rollout(old, N, STEPS), "plain" if domain is None else "with_domain", STEPS)


def test_generic_kernels_with_the_new_forms_equal_the_former_specialised_ones():
    """The shipped `nospec` library has the new forms (only -DVNL_XLANE_PLAIN switches them off): the generic kernels, where the
    tail form of dof_prefix is a wave-uniform branch at run time, against the former forms in the specialised kernel."""
    gen, old = V.rodent(N, V.variant("nospec")), V.rodent(N, _old())
    assert int(gen.dims.kernel_specialised) == 0 and int(old.dims.kernel_specialised) == 1
    V.same(V.rollout(gen, N, STEPS), V.rollout(old, N, STEPS), "nospec", STEPS)


def test_cross_lane_forms_change_no_bit_on_the_humanoid():
    """64 envs, nv = 27: a single trip of every scan and no tail form -- the one-instruction row_bcast steps alone."""
    n = 64
    V.same(V.humanoid_rollout(None, n, STEPS), V.humanoid_rollout(_old(), n, STEPS), "humanoid", STEPS)


def test_graphed_unroll_equals_the_eager_unroll_of_the_regression_build():
    """One 20-step replay of a captured unroll with the product library, 128 envs (the step kernel inside a graph, resets
    included), against the eager fused unroll of the regression build."""
    V.same_unroll(V.small_unroll(None, N, graphed=True), V.small_unroll(_old(), N, graphed=False), tail=True)
