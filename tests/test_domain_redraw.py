"""The domain redraw at fresh resets (vnl_env_set_domain_ranges, vnl_env_redraw_domain, the redraw inside vnl_env_reset_done;
RodentTracking.with_domain_ranges) on the host builds of the product source: tests/domain_redraw_cases.py on the rodent (the
specialised randomised kernels) and the ant (the generic ones) at 8 envs, the float64 build against the oracle of each env's
drawn model, and the restatement ppo_imitation/philox.py domain_draws on its own."""
import os

import numpy as np
import pytest
import torch

import domain_cases as D
import domain_redraw_cases as R
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
def test_draw_is_the_restatement_bit_for_bit(model):
    """Case 1: independent and shared ranges, a mask of half the envs, initial against later draws."""
    R.check_draw_is_the_restatement(MAKERS[model]())


def test_draw_is_the_restatement_in_the_double_build():
    """Case 1 where the tables hold the float64 values themselves: no cast hides a last-bit difference of the draw."""
    R.check_draw_is_the_restatement(_rodent(B, "double"))


@both
def test_redraw_is_set_domain_of_the_same_values(model):
    """Case 2: tables and reset + two control steps, bit for bit."""
    R.check_redraw_is_set_domain_of_the_same_values(MAKERS[model]())


@both
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_redraw_inside_reset_done_is_the_separate_launch(model, weighted):
    """Case 3."""
    R.check_fused_is_separate(MAKERS[model](), weighted)


@both
def test_sharding_does_not_change_the_domain_or_the_reset(model):
    """Case 4: one env of 8 at offset 0 == two envs of 4 at offsets 0 and 4."""
    R.check_sharding(MAKERS[model])


@both
def test_degenerate_and_absent_ranges(model):
    """Case 5."""
    R.check_degenerate_and_absent_ranges(MAKERS[model]())


@both
def test_errors_launch_nothing(model):
    """Case 6."""
    R.check_errors_launch_nothing(MAKERS[model](4))


def test_eager_wrapper_equals_fused_unroll_with_ranges():
    """Case 7 on the host build (no graph there)."""
    R.check_wrapper_paths(_rodent, CPU, graphed=False)


@both
def test_unfinished_envs_keep_their_first_domain(model):
    R.check_unfinished_envs_keep_their_first_domain(MAKERS[model], CPU)


def test_float64_build_follows_the_oracle_of_each_envs_drawn_model():
    """Case 8: 4 rodent envs after a redraw, each against the float64 oracle of ITS model over a reset and one control step
    (the bounds of tests/test_domain_randomization.py: the kernels read what was drawn)."""
    n = 4
    base = H.hostsim_env(n, "double")
    rg = R.ranges_for(base.sys, 8)
    env = base.with_domain_ranges(rg, shared=("cg_friction",))
    R.redraw(env)
    dom = {k: v.numpy() for k, v in R.drawn(env, rg, shared=("cg_friction",)).items()}
    assert np.array_equal(env.domain_table("dom_damp").numpy(), dom["dof_damping"])
    sf, noise, acts = D.inputs(n, seed=3)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    osts = []
    for i in range(n):
        one = H.hostsim_env(1, "double", model=D.model_with(base.sys, dom, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(sf[i:i + 1], noise[i:i + 1])
        e = D.row_err(st, ost, i)
        assert max(e.values()) < 1e-11, (i, e)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(acts[0]))
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, acts[0][i:i + 1])
        e = D.row_err(st, ost, i)
        assert max(e.values()) < 1e-8, (i, e)
        assert np.array_equal(st.done[i:i + 1].numpy(), ost["done"])


def test_restatement_alone():
    """Case 9: no library."""
    R.check_restatement_alone()


def test_domain_ranges_scaled_builds_absolute_bounds():
    from vnl_brax_imitation_amd.envs.rodent import domain_ranges_scaled

    m = H.model()
    rg = domain_ranges_scaled(m, gain=(0.7, 1.3), damping=(0.5, 2.0))
    assert set(rg) == {"cg_friction", "act_gain", "dof_damping"}
    c = D.compiled(m)
    assert np.array_equal(rg["cg_friction"][0], 0.5 * c["cg_friction"]) and np.array_equal(rg["cg_friction"][1], 1.5 * c["cg_friction"])
    for lo, hi in rg.values():
        assert bool((lo <= hi).all())
    env = _rodent(2).with_domain_ranges(rg)
    assert torch.equal(env.domain_ranges["act_gain"][1], torch.from_numpy(rg["act_gain"][1]))
