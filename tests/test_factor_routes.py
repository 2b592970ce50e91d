"""The factorisation routes each model takes (vnl_dims.factor_route): chosen once by the host at env creation
(csrc/vnl_lib.hip: choose_routes), read by the kernels' dispatchers (EnvWaveT::factor, invert_factor, newton_factor,
factor_both).  A route is a choice of arithmetic, so the packaged and test models are pinned to theirs (DESIGN.md, section 3,
"Factorisation routes")."""
import pytest

import helpers as H
import test_ant_env as TA
import test_generic_model as TG
import test_humanoid as TH
import test_newton_sparse as TN

LDS, ROWS16, ROWS36, ROWS36X2 = 1, 2, 3, 4  # csrc/vnl_types.h: VNL_ROUTE_*


def route(factor, inverse, hessian=0, pair=0):
    """qM's factor and inverse, the Newton Hessian's factor (0: CG), the lane sets of the articulated-body pair (0: none)."""
    return factor | inverse << 4 | hessian << 8 | pair << 12


def _humanoid_newton():
    from vnl_brax_imitation_amd.envs.humanoid import HumanoidTracking

    m = TN.newton_model(1, 4, base=TH._model())
    with H.hostsim_backend("float"):
        return HumanoidTracking(dict(solver="newton", iterations=1, ls_iterations=4), clip_length=60, episode_length=20,
                                reference_clip=TH._clip(m), model=m, num_envs=1, device="cpu")


# (the rodent's qM factor route is the one factor() takes in the diagnostic stage knobs: its forward pass takes the pair)
MODELS = {
    "rodent_cg": (lambda: H.hostsim_env(1), route(ROWS36X2, ROWS36X2, pair=2)),
    "rodent_newton": (lambda: TN._rodent(1, TN.newton_model(1, 4), real="float"), route(ROWS36X2, ROWS36X2, ROWS36X2, pair=2)),
    "ant_cg": (lambda: TA._env(1), route(LDS, ROWS16)),
    "ant_newton": (lambda: TA._env(1, params=TA.NEWTON), route(LDS, ROWS16, ROWS16)),
    "ant_as_rodent": (lambda: TG._ant_env(1, "float"), route(LDS, ROWS16)),  # eulerdamp on, nv 14: too small for the pair
    "humanoid_cg": (lambda: TH._env(1), route(LDS, ROWS16)),
    "humanoid_newton": (_humanoid_newton, route(LDS, ROWS16, ROWS16)),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_model_takes_its_recorded_factor_route(name):
    make, want = MODELS[name]
    d = make().dims
    assert int(d.factor_route) == want, (name, hex(int(d.factor_route)), hex(want))
