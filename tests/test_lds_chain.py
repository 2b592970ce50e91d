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
import pytest
import torch

import helpers as H
import hostsim_cases as HC

STEPS = 2

# (model, envs): the rodent CG 6 / 6 (both lane sets, the factor pair, two-trip tables), the ant under RodentTracking's glue
# (single set, factor_lds, euler's own factorisation), the humanoid, and the rodent Newton 1 / 4 (solve_inplace on the Hessian)
CASES = {"rodent_cg_6_6": (HC.MODELS["rodent_cg_6_6"], 8), "ant_rodent_tracking": (HC.ant_as_rodent_tracking, 8),
         "humanoid": (HC.MODELS["humanoid"], 4), "rodent_newton_1_4": (HC.MODELS["rodent_newton_1_4"], 4)}


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("name", list(CASES))
def test_lds_round_trips_taken_out_change_no_bit(name, real):
    make, B = CASES[name]
    _, new = HC.host_rollout(H.hostsim_library(real), real, make, B, STEPS)
    _, old = HC.host_rollout(H.hostsim_library(real, "ldsplain"), real, make, B, STEPS)
    HC.same_rollouts(new, old, (name, real), equal=HC.equal_with_nan)


@pytest.mark.parametrize("real", ["float", "double"])
def test_debug_image_is_the_same_with_the_solver_scalars_in_their_producing_loops(real):
    """With the debug image on the solver runs every iteration in full and records its line searches: the trace and the
    solver's vectors (grad / Mgrad / search / mv: what qg1, qg2 and the Gauss term are made of) must be the same bits."""
    dtype = torch.float64 if real == "double" else torch.float32
    imgs = []
    for lib in (H.hostsim_library(real), H.hostsim_library(real, "ldsplain")):
        with H.backend(lib, dtype):
            env, _ = HC.MODELS["rodent_cg_6_6"](2)
        env.debug(True)
        env.reset(5)
        img = {k: env.scratch(k).clone() for k in ("grad", "Mgrad", "search", "mv", "Ma", "qacc", "qfrc_constraint")}
        img["solver_trace"] = env.solver_trace().clone()
        imgs.append(img)
    for k in imgs[0]:
        assert torch.equal(imgs[0][k], imgs[1][k]), k
    assert imgs[0]["search"].abs().sum() > 0 and int(imgs[0]["solver_trace"][:, 0, 1].min()) >= 1  # (iterations ran)
