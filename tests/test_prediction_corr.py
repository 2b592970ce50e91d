"""metrics["prediction_corr"] at every minibatch size, CPU tier: the torch backend computes it beyond the sizes the
one-workgroup HIP kernel holds in LDS, and vnl_prediction_corr_plan (which needs no device) states the route rule."""
import ctypes as C

import numpy as np
import pytest

import prediction_corr_cases as PC
from vnl_brax_imitation_amd import _lib


@pytest.mark.parametrize("T,B", [(20, 420), (20, 1024)])
def test_torch_backend_computes_the_metric_at_large_sizes(T, B):
    assert not PC.fits_one_workgroup(T, B)
    nets, flat, data, norm, noise = PC.make_update_case(T, B)
    m, vs = PC.loss_float64(nets, flat, data, norm, noise)
    got = float(m["prediction_corr"])
    assert np.isfinite(got)
    x = np.concatenate([vs.numpy(), data.reward.double().numpy() * PC.HP["reward_scaling"]], axis=0)
    ref = float(np.clip(np.corrcoef(x), -1.0, 1.0).mean())
    assert abs(got - ref) <= 1e-9, (got, ref)


def _plan(lib, T, B, route=0):
    p = _lib.CorrPlan()
    rc = lib.vnl_prediction_corr_plan(T, B, route, C.byref(p))
    return rc, p


def test_plan_states_the_route_rule_without_a_device():
    lib = _lib.load_library()
    for T, B in [(1, 2), (5, 9), (20, 128), (20, 383), (20, 384), (20, 420), (20, 1024), (33, 300), (3, 2559), (3, 2560),
                 (1, 7679), (1, 7680), (7680, 2), (100, 77)]:
        rc, p = _plan(lib, T, B)
        assert rc == 0, (T, B, lib.vnl_last_error())
        assert p.route == (1 if PC.fits_one_workgroup(T, B) else 2), (T, B, p.route)
        if p.route == 1:
            assert (p.chunks, p.chunk_cols, p.row_tiles, p.workspace_floats) == (0, 0, 0, 0)
        rc, p = _plan(lib, T, B, 2)  # the tiled route can be forced at every size
        R = 2 * T
        assert rc == 0 and p.route == 2
        assert 1 <= p.chunks <= 32 and p.chunk_cols >= 1 and p.chunks * p.chunk_cols >= B > (p.chunks - 1) * p.chunk_cols
        assert p.row_tiles == (R + 63) // 64
        assert p.workspace_floats >= p.chunks * R * R + R
        rc, p = _plan(lib, T, B, 1)
        if PC.fits_one_workgroup(T, B):
            assert rc == 0 and p.route == 1
        else:
            assert rc == -1 and b"fit" in lib.vnl_last_error()
    # the workspace at the reference's proportions (unroll_length 20, 1024 trajectories per minibatch) stays small
    rc, p = _plan(lib, 20, 1024)
    assert rc == 0 and p.route == 2 and p.workspace_floats * 4 <= 256 * 1024


def test_plan_and_call_reject_bad_arguments():
    lib = _lib.load_library()
    for T, B, route in [(0, 8, 0), (-1, 8, 0), (4, 1, 0), (4, 0, 2), (4, 8, 3), (4, 8, -1)]:
        rc, _ = _plan(lib, T, B, route)
        assert rc == -1 and b"prediction_corr" in lib.vnl_last_error(), (T, B, route)
    assert lib.vnl_prediction_corr_plan(4, 8, 0, None) == -1 and b"null" in lib.vnl_last_error()
    # nothing is launched (and no device is touched) when an argument is bad; the pointers are never dereferenced
    p8 = C.c_void_p(8)
    assert lib.vnl_prediction_corr(None, p8, 1.0, 4, 8, 0, None, 0, p8, None) == -1 and b"null" in lib.vnl_last_error()
    assert lib.vnl_prediction_corr(p8, None, 1.0, 4, 8, 0, None, 0, p8, None) == -1
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 4, 8, 0, None, 0, None, None) == -1
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 0, 8, 0, None, 0, p8, None) == -1
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 4, 1, 0, None, 0, p8, None) == -1
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 20, 1024, 1, None, 0, p8, None) == -1 and b"fit" in lib.vnl_last_error()
    rc, p = _plan(lib, 20, 1024, 2)
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 20, 1024, 2, None, 0, p8, None) == -1 and b"workspace" in lib.vnl_last_error()
    assert lib.vnl_prediction_corr(p8, p8, 1.0, 20, 1024, 2, p8, p.workspace_floats - 1, p8, None) == -1
    assert b"workspace" in lib.vnl_last_error()
