"""The solver's last permitted iteration stops after constraint_force() (EnvWave::solve, csrc/vnl_body.h): its Gauss term,
cost, gradient, M^-1 grad (Newton: Hessian assembly + factorisation + inversion) and search update feed nothing -- the loop
cannot run again, and what follows reads only qacc and qfrc_constraint.  A host build of the same sources with the tail
forced back in (-DVNL_SOLVER_TAIL, the `tail` variant of csrc/build.py) must give the same bits on every output."""
import pytest
import torch

import helpers as H
import model_cases as M
import variant_cases as V
from hostsim_cases import MODELS, host_rollout, same_rollouts

STEPS = 4  # control steps (the issue asks for at least 3), each of several substeps = several full-length solves


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(MODELS))
def test_skipped_tail_of_the_last_solver_iteration_changes_no_bit(name, real):
    B = 4
    env, skip = host_rollout(H.hostsim_library(real), real, MODELS[name], B, STEPS)
    _, full = host_rollout(H.hostsim_library(real, "tail"), real, MODELS[name], B, STEPS)
    # the case is only a test if solves do run to the iteration count (where the tail is skipped): all four do
    assert int(env.sys.scalars["iterations"]) >= 1
    same_rollouts(skip, full, (name, real))


def test_debug_image_keeps_the_full_last_iteration():
    """With the debug image on, the solver runs its last iteration in full: the sections grad / Mgrad / search of the image are
    those of the build with the tail forced in, bit for bit (and are not left over from the iteration before)."""
    real = "double"
    imgs = []
    for lib in (H.hostsim_library(real), H.hostsim_library(real, "tail")):
        with H.backend(lib, torch.float64):
            env, _ = MODELS["rodent_cg_6_6"](1)
        env.debug(True)
        env.reset(5)
        imgs.append({k: env.scratch(k).clone() for k in ("grad", "Mgrad", "search", "mv", "Ma", "qacc", "qfrc_constraint")})
    for k in imgs[0]:
        assert torch.equal(imgs[0][k], imgs[1][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_skipped_tail_changes_no_bit_on_the_device(solver):
    """The product library against the regression build with the tail forced in (csrc/build.py --tail), 1024 envs, reset + three
    control steps, rodent CG 6 / 6 (specialised kernels) and Newton 1 / 4 (generic kernels): every output bit for bit."""
    B = 1024
    kw = {"model": M.newton_model(1, 4)} if solver == "newton" else {}
    outs = [V.rollout(V.rodent(B, lib, **kw), B, 3) for lib in (None, V.variant("tail"))]
    V.same(outs[0], outs[1], solver, 3, finite=False)
