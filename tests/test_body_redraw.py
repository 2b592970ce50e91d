"""The body-domain redraw at fresh resets (vnl_env_set_body_domain_ranges, the body part of vnl_env_redraw_domain and of the
redraw inside vnl_env_reset_done; RodentTracking.with_body_domain_ranges) on the host builds of the product source:
tests/body_redraw_cases.py on the rodent (the specialised randomised kernels) and the ant (the generic ones) at 8 envs, the
float64 build against the oracle of each env's drawn model, and the restatement ppo_imitation/philox.py body_domain_draws on
its own."""
import os

import numpy as np
import pytest
import torch

import body_domain_cases as BD
import body_redraw_cases as R
import domain_cases as D
import fresh_reset_cases as F
import helpers as H
from vnl_brax_imitation_amd.model import mjcf

B = 8
CPU = torch.device("cpu")


def _rodent(num_envs=B, real="float"):
    return H.hostsim_env(num_envs, real, reference_clip=F.three_clips())


def _ant(num_envs=B, real="float"):
    from vnl_brax_imitation_amd import envs

    m = mjcf.CompiledModel.load(os.path.join(H.ROOT, "vnl-brax-imitation_amd", "data", "ant.npz"))
    with H.hostsim_backend(real):
        return envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(m),
                                    model=m, num_envs=num_envs, device="cpu")


MAKERS = {"rodent": _rodent, "ant": _ant}
both = pytest.mark.parametrize("model", ["rodent", "ant"])


@both
def test_draw_is_the_restatement_and_the_tables_are_with_body_domain(model):
    """Case 1: independent, shared-mass and moments-with-mass ranges, a mask of half the envs, initial against later draws."""
    base = MAKERS[model]()
    assert (int(base.dims.nbody), int(base.dims.nbody_dynamic)) == ((66, 53) if model == "rodent" else (14, 10))
    R.check_draw_is_the_restatement(base)


@both
def test_draw_and_fold_in_the_double_build(model):
    """Case 1 where the tables hold the float64 values themselves: no cast hides a last-bit difference of draw or fold."""
    R.check_draw_is_the_restatement(MAKERS[model](B, "double"))


@both
def test_redrawn_env_is_the_env_set_by_hand(model):
    """Case 2: tables and reset + two control steps, bit for bit."""
    R.check_redrawn_env_is_the_env_set_by_hand(MAKERS[model]())


@both
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_redraw_inside_reset_done_is_the_separate_launch(model, weighted):
    """Case 3."""
    R.check_fused_is_separate(MAKERS[model](), weighted)


@both
def test_both_range_sets_together(model):
    """Case 4."""
    R.check_both_range_sets_together(MAKERS[model]())


@both
def test_sharding_does_not_change_the_bodies_or_the_reset(model):
    """Case 5: one env of 8 at offset 0 == two envs of 4 at offsets 0 and 4."""
    R.check_sharding(MAKERS[model])


@both
def test_degenerate_and_absent_ranges(model):
    """Case 6."""
    R.check_degenerate_and_absent_ranges(MAKERS[model]())


@both
def test_errors_launch_nothing(model):
    """Case 7."""
    R.check_errors_launch_nothing(MAKERS[model](4))


def test_eager_wrapper_equals_fused_unroll_with_body_ranges():
    """Case 8 on the host build (no graph there)."""
    R.check_wrapper_paths(_rodent, CPU, graphed=False)


@both
def test_unfinished_envs_keep_their_first_bodies(model):
    R.check_unfinished_envs_keep_their_first_bodies(MAKERS[model], CPU)


def test_float64_build_follows_the_oracle_of_each_envs_drawn_model():
    """Case 9: 4 rodent envs after a redraw, each against the float64 oracle of ITS model over a reset and one control step,
    with the bounds tests/test_body_domain.py holds its float64 build to (1e-11 after the reset, 1e-8 after a control step)."""
    n = 4
    base = H.hostsim_env(n, "double")
    env = base.with_body_domain_ranges(R.ranges_for(base.sys))
    R.redraw(env)
    dom = {k: v.numpy() for k, v in R.drawn(env).items()}
    sf, noise, acts = D.inputs(n, seed=3)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    osts = []
    for i in range(n):
        one = H.hostsim_env(1, "double", model=BD.model_with(base.sys, dom, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(sf[i:i + 1], noise[i:i + 1])
        e = D.row_err(st, ost, i)
        print(f"[body redraw oracle] env {i} reset max err {max(e.values()):.3e}")
        assert max(e.values()) < 1e-11, (i, e)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(acts[0]))
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, acts[0][i:i + 1])
        e = D.row_err(st, ost, i)
        print(f"[body redraw oracle] env {i} step max err {max(e.values()):.3e}")
        assert max(e.values()) < 1e-8, (i, e)
        assert np.array_equal(st.done[i:i + 1].numpy(), ost["done"])


def test_restatement_alone():
    """Case 10: no library."""
    R.check_restatement_alone()


def test_body_domain_ranges_scaled_builds_absolute_bounds():
    from vnl_brax_imitation_amd.envs.rodent import body_domain_ranges_scaled

    m = H.model()
    c = BD.compiled(m)
    rg = body_domain_ranges_scaled(m)
    assert set(rg) == {"body_mass", "body_inertia"}  # inertia=None: the mass multiples
    assert np.array_equal(rg["body_mass"][0], 0.7 * c["body_mass"]) and np.array_equal(rg["body_inertia"][1], 1.3 * c["body_inertia"])
    rg = body_domain_ranges_scaled(m, mass=(0.8, 1.2), inertia=(0.5, 2.0), ipos=(-0.1, 0.3))
    r = np.linalg.norm(c["body_ipos"], axis=1, keepdims=True)
    assert np.array_equal(rg["body_inertia"][0], 0.5 * c["body_inertia"]) and np.array_equal(rg["body_ipos"][1], c["body_ipos"] + 0.3 * r)
    for lo, hi in rg.values():
        assert bool((lo <= hi).all())
    env = _rodent(2).with_body_domain_ranges(rg, inertia_with_mass=True)
    got = env.body_domain_ranges
    assert torch.equal(got["body_mass"][1][1:], torch.from_numpy(rg["body_mass"][1][1:])) and got["inertia_with_mass"]
