"""The factorisation routes each model takes (vnl_dims.factor_route): chosen once by the host at env creation
(csrc/vnl_lib.hip: choose_routes), read by the kernels' dispatchers (EnvWaveT::factor, invert_factor, newton_factor,
factor_both).  A route is a choice of arithmetic, so the packaged and test models are pinned to theirs (DESIGN.md, section 3,
"Factorisation routes")."""
import pytest

import helpers as H
import model_cases as M

LDS, ROWS16, ROWS36, ROWS36X2 = 1, 2, 3, 4  # csrc/vnl_types.h: VNL_ROUTE_*


def route(factor, inverse, hessian=0, pair=0):
    """qM's factor and inverse, the Newton Hessian's factor (0: CG), the lane sets of the articulated-body pair (0: none)."""
    return factor | inverse << 4 | hessian << 8 | pair << 12


# (the rodent's qM factor route is the one factor() takes in the diagnostic stage knobs: its forward pass takes the pair)
MODELS = {
    "rodent_cg": (lambda: H.hostsim_env(1), route(ROWS36X2, ROWS36X2, pair=2)),
    "rodent_newton": (lambda: M.rodent_env(1, M.newton_model(1, 4), real="float"), route(ROWS36X2, ROWS36X2, ROWS36X2, pair=2)),
    "ant_cg": (lambda: M.ant_env(1), route(LDS, ROWS16)),
    "ant_newton": (lambda: M.ant_env(1, params=M.NEWTON), route(LDS, ROWS16, ROWS16)),
    "ant_as_rodent": (lambda: M.ant_as_rodent_env(1, "float"), route(LDS, ROWS16)),  # eulerdamp on, nv 14: too small for the pair
    "humanoid_cg": (lambda: M.humanoid_env(1), route(LDS, ROWS16)),
    "humanoid_newton": (lambda: M.humanoid_newton_env(1, "float"), route(LDS, ROWS16, ROWS16)),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_takes_its_recorded_factor_route(name):
    make, want = MODELS[name]
    d = make().dims
    assert int(d.factor_route) == want, (name, hex(int(d.factor_route)), hex(want))
