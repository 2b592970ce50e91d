"""Domain randomisation (RodentTracking.with_domain, include/vnl.h: vnl_env_set_domain) on the host builds of the kernels.

Per-env friction, actuator gain, damping and armature, MJX semantics: env i of a randomised batch runs what an unrandomised
env runs on a model whose four raw fields hold env i's values (derived constants as compiled, the contact rows' inverse
weight re-derived from friction).  The float64 build is held to the dense oracle of each env's own model, the float build
to the unrandomised kernels bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import domain_cases as D
import helpers as H
from domain_cases import inputs as _inputs
from domain_cases import row_err as _row_err
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.model import mjcf
from vnl_brax_imitation_amd.ppo_imitation import acting
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

def _outputs(st) -> dict:
    ps = st.pipeline_state
    out = {k: getattr(ps, k).clone() for k in ("qpos", "qvel", "qacc_warmstart")}
    out.update(obs=st.obs.clone(), reward=st.reward.clone(), done=st.done.clone(), metrics=st.info["_raw"]["metrics"].clone())
    return out


def _rodent_against_oracle(model=None, seed=1):
    """Float64 host build, rodent, 6 envs of a random domain: reset + one control step, every env against the float64
    oracle of an unrandomised env on that env's model (the bounds of test_hostsim_parity's float64 gate)."""
    B = 6
    kw = {} if model is None else dict(model=model)
    base = H.hostsim_env(B, "double", **kw)
    dom = D.random_domain(base.sys, B, seed)
    env = base.with_domain(dom)
    sf, noise, acts = _inputs(B, seed=seed)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    osts = []
    for i in range(B):
        one = H.hostsim_env(1, "double", model=D.model_with(base.sys, dom, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(sf[i:i + 1], noise[i:i + 1])
        e = _row_err(st, ost, i)
        assert max(e.values()) < 1e-11, (i, e)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(acts[0]))
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, acts[0][i:i + 1])
        e = _row_err(st, ost, i)
        assert max(e.values()) < 1e-8, (i, e)
        assert np.array_equal(st.done[i:i + 1].numpy(), ost["done"])
        m = np.stack([st.metrics[k][i:i + 1].numpy() for k in st.metrics], 1)
        assert np.abs(m - ost["metrics"]).max() < 1e-10
    # the domain did change the dynamics: the envs differ from an unrandomised batch
    plain = base.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    plain = base.step(plain, torch.from_numpy(acts[0]))
    assert not torch.equal(plain.pipeline_state.qvel, st.pipeline_state.qvel)


def test_float64_rodent_domain_matches_oracle_of_each_envs_model():
    _rodent_against_oracle()


def test_float64_rodent_newton_domain_matches_oracle_of_each_envs_model():
    """The tree-sparse Newton route (solver_newton in the model scalars, as tools/newton_bench.py model_for sets it): damping
    and armature also enter the Hessian's qM there."""
    m = copy.deepcopy(H.model())
    m.scalars.update(solver_newton=1)
    _rodent_against_oracle(m, seed=2)


def _ant(B, model, real="double"):
    from vnl_brax_imitation_amd import envs

    with H.hostsim_backend(real):
        return envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(model),
                                    model=model, num_envs=B, device="cpu")


def test_float64_ant_domain_matches_oracle_of_each_envs_model():
    """The generic (run-time dims) instantiation: the ant."""
    import os

    B = 6
    base = _ant(B, mjcf.CompiledModel.load(os.path.join(H.ROOT, "vnl-brax-imitation_amd", "data", "ant.npz")))
    assert int(base.dims.kernel_specialised) == 0
    dom = D.random_domain(base.sys, B, 3)
    env = base.with_domain(dom)
    st = env.reset()
    rng = np.random.default_rng(4)
    act = np.clip(0.5 * rng.standard_normal((B, 8)), -1, 1)
    osts = []
    for i in range(B):
        one = _ant(1, D.model_with(base.sys, dom, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(np.zeros(1, np.int32), np.zeros((1, 15)))
        for k in ("qpos", "qvel", "xpos", "qacc_warmstart"):
            assert H.scaled_err(getattr(st.pipeline_state, k).reshape(B, -1)[i:i + 1].numpy(), ost[k]) < 1e-10, (i, k)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(act))
    ps = st.pipeline_state
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, act[i:i + 1])
        assert H.scaled_err(ps.qpos[i:i + 1].numpy(), ost["qpos"]) < 1e-9, i
        assert H.scaled_err(ps.qvel[i:i + 1].numpy(), ost["qvel"]) < 1e-8, i
        assert np.abs(st.reward[i:i + 1].numpy() - ost["reward"]).max() < 1e-7 and np.array_equal(st.done[i:i + 1].numpy(), ost["done"])


def test_identity_domain_is_bitwise_the_unrandomised_env():
    """Float build: a domain equal to the compiled values gives the unrandomised env's outputs bit for bit (reset + 3 steps)."""
    B = 4
    base = H.hostsim_env(B)
    env = base.with_domain(D.identity(base.sys, B))
    sf, noise, acts = _inputs(B, seed=5)
    outs = []
    for e in (base, env):
        st = e.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
        for a in acts:
            st = e.step(st, torch.from_numpy(a))
        outs.append(_outputs(st))
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    # the derived tables are the upload's, bit for bit
    m = base.sys
    assert torch.equal(env.domain_table("dom_mu"), torch.tensor(D.identity(m, B)["cg_friction"], dtype=torch.float32))
    assert torch.equal(env.domain_table("dom_gain"), torch.tensor(D.identity(m, B)["act_gain"], dtype=torch.float32))


def test_randomised_env_i_is_bitwise_env_0_of_its_model():
    """Float build: env i of a randomised batch equals env 0 of an unrandomised env on model i, bit for bit."""
    B = 3
    base = H.hostsim_env(B)
    dom = D.random_domain(base.sys, B, 6)
    env = base.with_domain(dom)
    sf, noise, acts = _inputs(B, seed=7)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    for a in acts[:2]:
        st = env.step(st, torch.from_numpy(a))
    got = _outputs(st)
    for i in range(B):
        one = H.hostsim_env(1, model=D.model_with(base.sys, dom, i))
        s1 = one.reset(start_frame=torch.from_numpy(sf[i:i + 1]), noise=torch.from_numpy(noise[i:i + 1]))
        for a in acts[:2]:
            s1 = one.step(s1, torch.from_numpy(a[i:i + 1]))
        for k, v in _outputs(s1).items():
            assert torch.equal(got[k][i:i + 1], v), (i, k)


def test_wrap_binds_a_domain_without_touching_the_callers_env():
    B = 4
    base = H.hostsim_env(B)
    seen = []

    def fn(sys):
        seen.append(sys)
        return D.random_domain(sys, B, 8)

    wrapped = W.wrap(base, episode_length=10, randomization_fn=fn)
    assert seen == [base.sys] and base.domain is None
    inner = wrapped.env.env
    assert inner is not base and inner.sys is base.sys and inner.num_envs == B
    assert sorted(inner.domain) == sorted(D.FIELDS)
    assert acting._fusable(wrapped) is not None  # the fused rollout (and GraphedUnroll) accept the randomised env
    # the model is not mutated, and with_num_envs carries no domain
    for k, v in D.compiled(H.model()).items():
        assert np.array_equal(D.compiled(base.sys)[k], v), k
    assert inner.with_num_envs(2).domain is None
    st = wrapped.reset(torch.Generator().manual_seed(0))
    st = wrapped.step(st, torch.zeros(B, 30))
    assert torch.isfinite(st.obs).all()


def test_bad_domains_raise():
    B = 2
    base = H.hostsim_env(B)
    dom = D.identity(base.sys, B)
    with pytest.raises(ValueError, match="unknown domain field"):
        base.with_domain({"body_mass": np.ones((B, 66))})
    with pytest.raises(ValueError, match="shape"):
        base.with_domain({"act_gain": dom["act_gain"][:1]})
    with pytest.raises(ValueError, match="shape"):
        base.with_domain({"dof_damping": dom["dof_damping"][:, :-1]})
    bad = [("cg_friction", 0.0), ("cg_friction", -1.0), ("dof_damping", -1e-3), ("dof_armature", -1.0), ("act_gain", np.nan),
           ("dof_armature", np.inf)]
    for k, v in bad:
        d = {k: dom[k].copy()}
        d[k][1, 3] = v
        with pytest.raises(ValueError):
            base.with_domain(d)
    # zero damping / armature are allowed, as is a partial domain
    d = {"dof_damping": np.zeros_like(dom["dof_damping"])}
    assert sorted(base.with_domain(d).domain) == ["dof_damping"]
    # the C-ABI validates on its own
    lib = base._L
    fr = np.ascontiguousarray(dom["cg_friction"])
    fr[0, 0] = 0.0
    desc = _lib.Domain(cg_friction=C.c_void_p(fr.ctypes.data))
    assert lib.vnl_env_set_domain(base._env_h, C.byref(desc), None) == -1
    assert b"cg_friction" in lib.vnl_last_error()
    fr[0, 0] = np.nan
    assert lib.vnl_env_set_domain(base._env_h, C.byref(desc), None) == -1


def test_train_binding_is_the_same_on_every_rank():
    """train.bind_randomization: the training env's generator is seeded from `seed` alone (reference train.py:200: all
    devices get the same randomisation rng), so rank 0 and rank 1 build identical tables."""
    m = H.model()

    def fn(sys, num_envs, rng):
        u = torch.rand((num_envs, len(sys.act_gain)), generator=rng, dtype=torch.float64)
        return {"act_gain": torch.as_tensor(sys.act_gain) * (0.7 + 0.6 * u)}

    tabs = []
    for rank in (0, 1):
        bound = ppo.bind_randomization(fn, 4, seed=11)
        tabs.append(bound(m)["act_gain"])
    assert torch.equal(tabs[0], tabs[1])
    assert not torch.equal(ppo.bind_randomization(fn, 4, seed=12)(m)["act_gain"], tabs[0])
    assert ppo.bind_randomization(None, 4, 0) is None


def test_derived_inverse_weight_is_the_float64_formula():
    """vnl_env_scratch "dom_invw": (t + mu^2 t) 2 mu^2 / impratio per env, t = invweight0 of the world + that of the geom's body
    (the upload's expression, float64 build), and the raw tables are what was given."""
    B = 3
    base = H.hostsim_env(B, "double")
    m = base.sys
    dom = D.random_domain(m, B, 9)
    env = base.with_domain(dom)
    iw0 = np.asarray(m.body_invweight0, np.float64).reshape(-1)
    t = iw0[0] + iw0[2 * np.asarray(m.cg_bodyid)]
    mu = dom["cg_friction"]
    want = (t + mu * mu * t) * 2 * mu * mu / float(m.scalars["impratio"])
    assert np.array_equal(env.domain_table("dom_invw").numpy(), want)
    assert np.array_equal(env.domain_table("dom_mu").numpy(), mu)
    assert np.array_equal(env.domain_table("dom_gain").numpy(), dom["act_gain"])
    assert np.array_equal(env.domain_table("dom_damp").numpy(), dom["dof_damping"])
    assert np.array_equal(env.domain_table("dom_arm").numpy(), dom["dof_armature"])
    with pytest.raises(_lib.VnlError, match="no domain"):
        base.domain_table("dom_mu")
