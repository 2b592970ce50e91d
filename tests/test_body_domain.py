"""Body-domain randomisation (RodentTracking.with_body_domain, include/vnl.h: vnl_env_set_body_domain) on the host builds
of the kernels.

Per-env body_mass / body_inertia / body_ipos over the bodies of the model as given, MJX semantics: env i of a randomised
batch runs what an unrandomised env runs on a model whose three arrays hold env i's values (invweight0, meaninertia as
compiled; the fold of the welded bodies, the packed inertia and 1 / total mass derived per env).  The float64 build is held
to the dense oracle of each env's own model, the float build to the unrandomised kernels bit for bit."""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import body_domain_cases as BD
import domain_cases as D
import helpers as H
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.ppo_imitation import ppo_networks
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

OUT_KEYS = ("qpos", "qvel", "act", "qacc_warmstart", "xpos", "qfrc_actuator", "subtree_com1")
TABLES = ("dom_mass", "dom_ipos", "dom_inertia6", "dom_tminv")


def _inputs(B, nq=74, nu=30, seed=0):
    rng = np.random.default_rng(seed)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = 1e-3 * rng.standard_normal((B, nq))
    acts = np.clip(0.3 * rng.standard_normal((3, B, nu)), -1, 1)
    return sf, noise, acts


def _row_err(st, ost, i):
    ps = st.pipeline_state
    okey = {"subtree_com1": "com1"}  # (the oracle's name of data.subtree_com[1])
    out = {k: H.scaled_err(ps.raw(k).reshape(st.obs.shape[0], -1)[i:i + 1].numpy(), np.asarray(ost[okey.get(k, k)]).reshape(1, -1))
           for k in OUT_KEYS}
    out["obs"] = H.scaled_err(st.info["_raw"]["obs"][i:i + 1].numpy(), ost["obs"])  # (the kernel's buffer: AntTracking presents [traj | obs])
    out["traj"] = H.scaled_err(st.info["traj"][i:i + 1].numpy(), ost["traj"])
    return out


def _outputs(st) -> dict:
    ps = st.pipeline_state
    out = {k: ps.raw(k).clone() for k in ps._FIELDS}
    out.update(obs=st.obs.clone(), reward=st.reward.clone(), done=st.done.clone(), metrics=st.info["_raw"]["metrics"].clone(),
               traj=st.info["traj"].clone())
    return out


def _run(env, sf, noise, acts, real="float"):
    dt = torch.float64 if real == "double" else torch.float32
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    for a in acts:
        st = env.step(st, torch.from_numpy(a).to(dt))
    return _outputs(st)


def _model_of(base_sys, dom4, body, i):
    m = base_sys if dom4 is None else D.model_with(base_sys, dom4, i)
    return BD.model_with(m, body, i)


def _rodent_against_oracle(model=None, seed=1, four=None):
    """Float64 host build, rodent, 6 envs of a random body domain (four: also a random four-field domain, applied "first" or
    "last"): reset + one control step, every env against the float64 oracle on that env's model, with the bounds of
    test_domain_randomization / test_hostsim_parity's float64 gate (1e-11 after reset, 1e-8 after a control step, scaled;
    metrics 1e-10)."""
    B = 6
    kw = {} if model is None else dict(model=model)
    base = H.hostsim_env(B, "double", **kw)
    body = BD.random_body_domain(base.sys, B, seed)
    dom4 = D.random_domain(base.sys, B, 1) if four else None
    if four == "first":
        env = base.with_domain(dom4).with_body_domain(body)
    elif four == "last":
        env = base.with_body_domain(body).with_domain(dom4)
    else:
        env = base.with_body_domain(body)
    assert sorted(env.domain) == sorted(BD.FIELDS + (D.FIELDS if four else ()))
    sf, noise, acts = _inputs(B, seed=seed)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    osts = []
    for i in range(B):
        one = H.hostsim_env(1, "double", model=_model_of(base.sys, dom4, body, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(sf[i:i + 1], noise[i:i + 1])
        e = _row_err(st, ost, i)
        print(f"[reset, env {i}] " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) < 1e-11, (i, e)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(acts[0]))
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, acts[0][i:i + 1])
        e = _row_err(st, ost, i)
        print(f"[step, env {i}] " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) < 1e-8, (i, e)
        assert np.array_equal(st.done[i:i + 1].numpy(), ost["done"])
        m = np.stack([st.metrics[k][i:i + 1].numpy() for k in st.metrics], 1)
        assert np.abs(m - ost["metrics"]).max() < 1e-10
    plain = base.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    plain = base.step(plain, torch.from_numpy(acts[0]))
    assert not torch.equal(plain.pipeline_state.qvel, st.pipeline_state.qvel)
    assert not torch.equal(plain.pipeline_state.raw("subtree_com1"), st.pipeline_state.raw("subtree_com1"))


def test_numpy_inertia_recomputation_reproduces_the_packaged_models():
    """What the per-env reference models rest on (it involves no new product code: the issue asks for it as a guard of the
    tests' own recomputation of body_inertia_full)."""
    assert BD.check_recomputation()


def test_float64_rodent_body_domain_matches_oracle_of_each_envs_model():
    """The specialised rodent kernel (13 welded bodies folded per env), CG."""
    assert len(BD.welded_bodies(H.model())) == 13
    _rodent_against_oracle()


def test_float64_rodent_newton_body_domain_matches_oracle_of_each_envs_model():
    m = copy.deepcopy(H.model())
    m.scalars.update(solver_newton=1)
    _rodent_against_oracle(m, seed=2)


@pytest.mark.parametrize("order", ["first", "last"])
def test_float64_four_field_and_body_domain_together(order):
    """Both parts on one env, the four-field domain applied before / after the body domain.

    The four-field draw is that of seed 1, the draw test_domain_randomization holds to these bounds on its own; the body draw
    is seed 3 at the issue's full spread.  Finding behind that choice: with the four-field draw of seed 103 the bound after
    reset is missed in env 2 (qacc_warmstart 5.3e-10 against 1e-11), and so it is by the UNRANDOMISED float64 build on that
    env's model against the same oracle, while the randomised and the unrandomised build agree to 1.1e-15: the miss belongs
    to that model's CG solve, not to the per-env tables.  Either draw alone holds 1e-11 on that env, so shrinking the body
    spread is not what removes it; the bounds are unchanged."""
    _rodent_against_oracle(seed=3, four=order)


def _ant(B, model, real="double"):
    """(the clip -- its centre-of-mass track included -- is always that of the packaged ant: a randomised batch shares one clip)"""
    from vnl_brax_imitation_amd import envs

    with H.hostsim_backend(real):
        return envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(BD.packaged("ant")),
                                    model=model, num_envs=B, device="cpu")


def test_float64_ant_body_domain_matches_oracle_of_each_envs_model():
    """The generic (run-time dims) instantiation: the ant (14 bodies, 4 of them welded)."""
    B = 6
    base = _ant(B, BD.packaged("ant"))
    assert int(base.dims.kernel_specialised) == 0 and (int(base.dims.nbody_dynamic), int(base.dims.nbody)) == (10, 14)
    body = BD.random_body_domain(base.sys, B, 3)
    env = base.with_body_domain(body)
    st = env.reset()
    rng = np.random.default_rng(4)
    act = np.clip(0.5 * rng.standard_normal((B, 8)), -1, 1)
    osts = []
    for i in range(B):
        one = _ant(1, BD.model_with(base.sys, body, i))
        o = H.make_oracle(one, "f64")
        ost = o.env_reset(np.zeros(1, np.int32), np.zeros((1, 15)))
        e = _row_err(st, ost, i)
        print(f"[ant reset, env {i}] " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) < 1e-11, (i, e)
        osts.append((o, ost))
    st = env.step(st, torch.from_numpy(act))
    ps = st.pipeline_state
    for i, (o, ost) in enumerate(osts):
        o.env_step(ost, act[i:i + 1])
        e = _row_err(st, ost, i)
        print(f"[ant step, env {i}] " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
        assert max(e.values()) < 1e-8, (i, e)
        assert np.array_equal(st.done[i:i + 1].numpy(), ost["done"])
        assert np.abs(st.info["_raw"]["metrics"][i:i + 1].numpy() - ost["metrics"]).max() < 1e-10
    plain = base.step(base.reset(), torch.from_numpy(act))
    assert not torch.equal(plain.pipeline_state.qvel, ps.qvel)


def test_a_welded_bodys_mass_alone_changes_its_env():
    """The per-env fold: one welded body's mass doubled in env 1 only.  Env 1's fused tables and state change, env 0 keeps
    the unrandomised env's bits."""
    B = 2
    base = H.hostsim_env(B)
    m = base.sys
    wb = int(BD.welded_bodies(m)[-1])
    assert np.asarray(m.arrays["body_jntnum"])[wb] == 0 and np.asarray(m.arrays["body_mass"])[wb] > 0
    mass = BD.identity(m, B)["body_mass"]
    mass[1, wb] *= 2.0
    env = base.with_body_domain({"body_mass": mass})
    assert sorted(env.domain) == ["body_mass"]
    tm, ti, tv = env.domain_table("dom_mass"), env.domain_table("dom_ipos"), env.domain_table("dom_tminv")
    assert torch.equal(tm[0], tm[1]) is False and int((tm[0] != tm[1]).sum()) == 1  # the one dynamic body it rides on
    assert not torch.equal(ti[0], ti[1]) and float(tv[1]) < float(tv[0])
    sf, noise, acts = _inputs(B, seed=5)
    sf[:], noise[:] = sf[0], noise[0]
    acts[:, 1] = acts[:, 0]
    a, b = _run(base, sf, noise, acts[:1]), _run(env, sf, noise, acts[:1])
    for k in a:
        assert torch.equal(a[k][0], b[k][0]), k
    assert not torch.equal(b["qvel"][0], b["qvel"][1]) and not torch.equal(b["subtree_com1"][0], b["subtree_com1"][1])


def _fused_compiled_tables(env):
    """The vreal cast of the fused compiled inertial tables: an unrandomised env has no "dom_*" tables, so they are read
    from an env whose body part was set and cleared again (the four-field part keeps the tables alive)."""
    e = env.with_domain(D.identity(env.sys, env.num_envs))
    return {k: e.domain_table(k) for k in TABLES}


@pytest.mark.parametrize("which", ["rodent", "ant"])
def test_identity_body_domain_is_bitwise_the_unrandomised_env(which):
    """Float build: the compiled arrays tiled give the unrandomised env's outputs bit for bit (reset + 3 steps), and the
    tables are the upload's."""
    B = 4
    if which == "rodent":
        base = H.hostsim_env(B)
        sf, noise, acts = _inputs(B, seed=5)
    else:
        base = _ant(B, BD.packaged("ant"), "float")
        sf, noise, acts = _inputs(B, nq=15, nu=8, seed=6)
        sf, noise = np.zeros_like(sf), noise * 0
    env = base.with_body_domain(BD.identity(base.sys, B))
    f32 = lambda x: x.astype(np.float32)  # noqa: E731
    a, b = _run(base, sf, f32(noise), f32(acts)), _run(env, sf, f32(noise), f32(acts))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    mass = np.asarray(base.sys.arrays["body_mass"], np.float64)
    assert torch.equal(env.domain_table("dom_tminv"), torch.full((B, 1), 1.0 / mass.sum(), dtype=torch.float64).to(torch.float32))
    tm = env.domain_table("dom_mass")
    assert tm.shape == (B, int(base.dims.nbody_dynamic)) and abs(float(tm[0].double().sum()) - mass.sum()) < 1e-5 * mass.sum()
    for k, v in _fused_compiled_tables(base).items():
        assert torch.equal(env.domain_table(k), v), k
    # ... and an independent NumPy fold of the compiled arrays gives them to float32 rounding (the moments' sums carry the
    # parallel-axis terms of the welded bodies: a few roundings of the largest term)
    for k, v in BD.numpy_fold(base.sys).items():
        got = env.domain_table(k)[0].double().numpy()
        assert np.abs(got - v).max() <= 4e-7 * np.abs(v).max(), (k, np.abs(got - v).max(), np.abs(v).max())


def test_float64_tables_of_a_random_body_domain_are_an_independent_numpy_fold():
    """Float64 build: the per-env tables of a random body domain against a fold written independently in NumPy (sums about
    the fused centre of mass instead of the library's accumulate-about-the-origin-and-shift), 1e-12 of each table's scale."""
    B = 3
    for base in (H.hostsim_env(B, "double"), _ant(B, BD.packaged("ant"))):
        m = base.sys
        dom = BD.random_body_domain(m, B, 21)
        env = base.with_body_domain(dom)
        for i in range(B):
            full = BD.inertia_full(np.asarray(m.arrays["body_iquat"]).reshape(-1, 4), dom["body_inertia"][i])
            for k, v in BD.numpy_fold(m, dom["body_mass"][i], full, dom["body_ipos"][i]).items():
                got = env.domain_table(k)[i].numpy()
                assert np.abs(got - v).max() <= 1e-12 * np.abs(v).max(), (i, k, np.abs(got - v).max())


def test_body_randomised_groups_are_bitwise_unrandomised_envs_on_their_models():
    """Float build: 16 envs in 4 groups (mass and ipos varied), each env bit for bit an unrandomised env created on its
    group's model: the per-env fold is the upload's fold."""
    B, G = 16, 4
    base = H.hostsim_env(B)
    sets = BD.group_domain(base.sys, G, 7)
    grp = np.arange(B) // (B // G)
    dom = {k: v[grp] for k, v in sets.items()}
    sf, noise, acts = _inputs(B, seed=8)
    noise, acts = noise.astype(np.float32), acts.astype(np.float32)
    env = base.with_body_domain(dom)
    got = _run(env, sf, noise, acts[:2])
    for g in range(G):
        rows = np.nonzero(grp == g)[0]
        one = H.hostsim_env(len(rows), model=BD.model_with(base.sys, sets, g))
        want = _run(one, sf[rows], noise[rows], acts[:2, rows])
        for k, v in want.items():
            assert torch.equal(got[k][rows], v), (g, k)
    assert not torch.equal(got["qvel"][0], _run(base, sf, noise, acts[:2])["qvel"][0])


def test_permuting_the_rows_of_a_body_domain_permutes_the_outputs():
    B = 5
    base = H.hostsim_env(B)
    dom = BD.random_body_domain(base.sys, B, 9)
    perm = np.array([3, 0, 4, 1, 2])
    sf, noise, acts = _inputs(B, seed=10)
    noise, acts = noise.astype(np.float32), acts.astype(np.float32)
    a = _run(base.with_body_domain(dom), sf, noise, acts[:2])
    b = _run(base.with_body_domain({k: v[perm] for k, v in dom.items()}), sf[perm], noise[perm], acts[:2, perm])
    for k in a:
        assert torch.equal(a[k][perm], b[k]), k


def test_bad_body_domains_raise():
    B = 2
    base = H.hostsim_env(B)
    m = base.sys
    ident = BD.identity(m, B)
    with pytest.raises(ValueError, match="unknown domain field"):
        base.with_domain({"body_mass": np.ones((B, 66))})
    with pytest.raises(ValueError, match="unknown body domain field"):
        base.with_body_domain({"body_iquat": np.ones((B, 66, 4))})
    with pytest.raises(ValueError, match="shape"):
        base.with_body_domain({"body_mass": ident["body_mass"][:1]})
    with pytest.raises(ValueError, match="shape"):
        base.with_body_domain({"body_mass": np.ones((B, int(base.dims.nbody_dynamic)))})
    with pytest.raises(ValueError, match="shape"):
        base.with_body_domain({"body_ipos": ident["body_ipos"].reshape(B, -1)})
    for k, v in [("body_mass", np.nan), ("body_mass", -1e-3), ("body_inertia", -1e-9), ("body_inertia", np.inf), ("body_ipos", np.nan),
                 ("body_ipos", np.inf)]:
        d = {k: ident[k].copy()}
        d[k][1, 5] = v
        with pytest.raises(ValueError, match=k):
            base.with_body_domain(d)
    # a jointed body left without mass once welded bodies are folded in: only the per-env fold can tell
    jn = np.asarray(m.arrays["body_jntnum"])
    welded = set(BD.welded_bodies(m).tolist())
    parents = {int(np.asarray(m.arrays["body_parentid"])[w]) for w in welded}
    lone = next(b for b in range(2, jn.size) if jn[b] > 0 and b not in parents and ident["body_mass"][0, b] > 0)
    d = {"body_mass": ident["body_mass"].copy()}
    d["body_mass"][1, lone] = 0.0
    with pytest.raises(ValueError, match="body_mass"):
        base.with_body_domain(d)
    d = {"body_inertia": ident["body_inertia"].copy()}
    d["body_inertia"][0, lone] = 0.0
    with pytest.raises(ValueError, match="body_inertia"):
        base.with_body_domain(d)
    # ... while a welded body may be massless (its parent carries the dofs), and a partial domain is accepted
    w = int(BD.welded_bodies(m)[0])
    d = {"body_mass": ident["body_mass"].copy()}
    d["body_mass"][:, w] = 0.0
    assert sorted(base.with_body_domain(d).domain) == ["body_mass"]
    # row 0 (the world body) is not read
    d["body_mass"][:, 0] = 123.0
    assert torch.equal(base.with_body_domain(d).domain_table("dom_mass")[:, 0], torch.zeros(B))
    # the C-ABI validates on its own
    lib = base._L
    for field, bad, idx in (("body_mass", np.nan, (0, 3)), ("body_mass", -1.0, (1, 4)), ("body_inertia", -1.0, (0, 7, 1)),
                            ("body_ipos", np.inf, (1, 2, 0)), ("body_mass", 0.0, (1, lone))):
        arr = np.ascontiguousarray(ident[field].copy())
        arr[idx] = bad
        desc = _lib.BodyDomain(**{field: C.c_void_p(arr.ctypes.data)})
        assert lib.vnl_env_set_body_domain(base._env_h, C.byref(desc), None) == -1, (field, bad)
        assert field.encode() in lib.vnl_last_error(), lib.vnl_last_error()
    zero = np.zeros_like(ident["body_mass"])
    desc = _lib.BodyDomain(body_mass=C.c_void_p(zero.ctypes.data))
    assert lib.vnl_env_set_body_domain(base._env_h, C.byref(desc), None) == -1 and b"body_mass" in lib.vnl_last_error()
    assert lib.vnl_env_set_body_domain(None, C.byref(desc), None) == -1
    with pytest.raises(_lib.VnlError, match="no domain"):
        base.domain_table("dom_mass")


def test_clearing_a_part_returns_it_to_the_compiled_values():
    """Raw calls: a null descriptor clears one part; the other part stays, and with both cleared the env is the
    unrandomised one bit for bit."""
    B = 3
    base = H.hostsim_env(B)
    env = H.hostsim_env(B)
    body, dom4 = BD.random_body_domain(base.sys, B, 11), D.random_domain(base.sys, B, 12)
    sf, noise, acts = _inputs(B, seed=13)
    noise, acts = noise.astype(np.float32), acts.astype(np.float32)
    keep = [np.ascontiguousarray(v) for v in list(body.values()) + list(dom4.values())]
    bdesc = _lib.BodyDomain(**{k: C.c_void_p(a.ctypes.data) for k, a in zip(body, keep[:3])})
    fdesc = _lib.Domain(**{k: C.c_void_p(a.ctypes.data) for k, a in zip(dom4, keep[3:])})
    lib = env._L
    assert lib.vnl_env_set_body_domain(env._env_h, C.byref(bdesc), None) == 0
    assert lib.vnl_env_set_domain(env._env_h, C.byref(fdesc), None) == 0
    both = _run(env, sf, noise, acts[:1])
    ref = _run(base.with_domain(dom4).with_body_domain(body), sf, noise, acts[:1])
    for k in ref:
        assert torch.equal(both[k], ref[k]), k
    assert lib.vnl_env_set_body_domain(env._env_h, None, None) == 0  # the four-field part stays
    four = _run(env, sf, noise, acts[:1])
    ref = _run(base.with_domain(dom4), sf, noise, acts[:1])
    for k in ref:
        assert torch.equal(four[k], ref[k]), k
    assert lib.vnl_env_set_body_domain(env._env_h, C.byref(bdesc), None) == 0
    assert lib.vnl_env_set_domain(env._env_h, None, None) == 0  # the body part stays
    only_body = _run(env, sf, noise, acts[:1])
    ref = _run(base.with_body_domain(body), sf, noise, acts[:1])
    for k in ref:
        assert torch.equal(only_body[k], ref[k]), k
    assert lib.vnl_env_set_body_domain(env._env_h, None, None) == 0
    plain, cleared = _run(base, sf, noise, acts), _run(env, sf, noise, acts)
    for k in plain:
        assert torch.equal(plain[k], cleared[k]), k
    with pytest.raises(_lib.VnlError, match="no domain"):
        env.domain_table("dom_mass")


@pytest.mark.parametrize("first", ["four", "body"])
def test_a_cleared_part_reads_as_compiled_when_the_other_part_is_set_later(first):
    """Raw calls: set one part to random values, clear it, then set the OTHER part to its identity: every table holds the
    compiled values and the env is the unrandomised one bit for bit."""
    B = 3
    base, env = H.hostsim_env(B), H.hostsim_env(B)
    lib = env._L
    rand = {"four": D.random_domain(base.sys, B, 14), "body": BD.random_body_domain(base.sys, B, 15)}
    ident = {"four": D.identity(base.sys, B), "body": BD.identity(base.sys, B)}
    other = "body" if first == "four" else "four"

    def call(part, dom):
        if dom is None:
            return (lib.vnl_env_set_domain if part == "four" else lib.vnl_env_set_body_domain)(env._env_h, None, None)
        keep = {k: np.ascontiguousarray(v) for k, v in dom.items()}
        ptrs = {k: C.c_void_p(a.ctypes.data) for k, a in keep.items()}
        if part == "four":
            return lib.vnl_env_set_domain(env._env_h, C.byref(_lib.Domain(**ptrs)), None)
        return lib.vnl_env_set_body_domain(env._env_h, C.byref(_lib.BodyDomain(**ptrs)), None)

    assert call(first, rand[first]) == 0 and call(first, None) == 0 and call(other, ident[other]) == 0
    want = base.with_domain(ident["four"])
    for k in ("dom_mu", "dom_invw", "dom_gain", "dom_damp", "dom_arm") + TABLES:
        assert torch.equal(env.domain_table(k), want.domain_table(k)), k
    assert torch.equal(env.domain_table("dom_mu"), torch.tensor(ident["four"]["cg_friction"], dtype=torch.float32))
    sf, noise, acts = _inputs(B, seed=16)
    noise, acts = noise.astype(np.float32), acts.astype(np.float32)
    a, b = _run(base, sf, noise, acts[:2]), _run(env, sf, noise, acts[:2])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _fn(sys, num_envs, rng):
    """A randomization_fn returning body keys and cg_friction together."""
    u = lambda *s: torch.rand((num_envs,) + s, generator=rng, dtype=torch.float64)  # noqa: E731
    nb = len(sys.arrays["body_mass"])
    return {"body_mass": torch.as_tensor(np.asarray(sys.arrays["body_mass"], np.float64)) * (0.7 + 0.6 * u(nb)),
            "body_ipos": torch.as_tensor(np.asarray(sys.arrays["body_ipos"], np.float64).reshape(nb, 3)) * (0.9 + 0.2 * u(nb, 3)),
            "cg_friction": torch.as_tensor(np.asarray(sys.cg_friction)[:, 0]) * (0.4 + 1.2 * u(sys.cg_friction.shape[0]))}


def _tables_are(inner, d):
    """The tables the kernels read equal what fn returned: friction directly, the body tables through an unrandomised
    model of env 0's values (the library's own fold) and the sum of the masses."""
    assert sorted(inner.domain) == ["body_ipos", "body_mass", "cg_friction"]
    assert torch.equal(inner.domain_table("dom_mu"), d["cg_friction"].to(torch.float32))
    for k in ("body_mass", "body_ipos", "cg_friction"):
        assert torch.equal(inner.domain[k], d[k]), k
    tv = inner.domain_table("dom_tminv")[:, 0]
    mass = d["body_mass"].clone()
    mass[:, 0] = 0.0
    assert torch.allclose(tv.double(), 1.0 / mass.sum(1), rtol=1e-6, atol=0)
    sets = {k: d[k].numpy() for k in ("body_mass", "body_ipos")}
    one = H.hostsim_env(1, model=BD.model_with(inner.sys, sets, 0))
    ref = one.with_domain(D.identity(one.sys, 1))
    for k in TABLES:
        assert torch.equal(inner.domain_table(k)[:1], ref.domain_table(k)), k


def test_wrap_splits_the_domain_by_key():
    B = 4
    base = H.hostsim_env(B)
    returned = []

    def fn(sys):
        returned.append(_fn(sys, B, torch.Generator().manual_seed(3)))
        return returned[-1]

    wrapped = W.wrap(base, episode_length=10, randomization_fn=fn)
    inner = wrapped.env.env
    assert base.domain is None and inner is not base and inner.sys is base.sys and inner.num_envs == B
    _tables_are(inner, returned[0])
    assert inner.with_num_envs(2).domain is None
    for k, v in BD.compiled(H.model()).items():
        assert np.array_equal(BD.compiled(base.sys)[k], v), k
    st = wrapped.reset(torch.Generator().manual_seed(0))
    st = wrapped.step(st, torch.zeros(B, 30))
    assert torch.isfinite(st.obs).all()
    with pytest.raises(ValueError, match="unknown domain field"):
        W.wrap(base, randomization_fn=lambda sys: {"body_mass": returned[0]["body_mass"], "body_quat": 1.0})


def test_train_binds_a_body_domain(monkeypatch):
    """A short train(..., randomization_fn=fn) on the host build: the training and the eval env read what fn returned."""
    returned, wrapped = [], []

    def fn(sys, num_envs, rng):
        returned.append(_fn(sys, num_envs, rng))
        return returned[-1]

    real_wrap = W.wrap

    def recording_wrap(*a, **k):
        w = real_wrap(*a, **k)
        wrapped.append(w)
        return w

    monkeypatch.setattr(W, "wrap", recording_wrap)
    env = H.hostsim_env(8)
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=16, encoder_layer_sizes=(32,),
                           decoder_layer_sizes=(32,), value_hidden_layer_sizes=(32,))
    _, _, metrics = ppo.train(environment=env, num_timesteps=8 * 5, episode_length=20, num_envs=8, learning_rate=1e-3, entropy_cost=1e-3,
                              discounting=0.95, unroll_length=5, batch_size=2, num_minibatches=4, num_updates_per_batch=1, num_evals=1,
                              normalize_observations=True, network_factory=nf, num_eval_envs=4, seed=1, randomization_fn=fn)
    assert np.isfinite(float(metrics["eval/episode_reward"]))
    assert env.domain is None and len(returned) == 2 and len(wrapped) == 2
    for d, w, n in zip(returned, wrapped, (8, 4)):
        assert w.env.env.num_envs == n
        _tables_are(w.env.env, d)


def test_train_binding_of_a_body_domain_is_the_same_on_every_rank():
    """train.bind_randomization seeds the generator from `seed` alone: two ranks wrapping their env read back identical
    body tables, another seed different ones."""
    tabs = []
    for seed in (11, 11, 12):
        w = W.wrap(H.hostsim_env(4), episode_length=10, randomization_fn=ppo.bind_randomization(_fn, 4, seed=seed))
        tabs.append({k: w.env.env.domain_table(k) for k in TABLES + ("dom_mu",)})
    for k in tabs[0]:
        assert torch.equal(tabs[0][k], tabs[1][k]), k
    assert not torch.equal(tabs[0]["dom_mass"], tabs[2]["dom_mass"])


def _san(name):
    p = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_san("libasan.so") is None or _san("libubsan.so") is None, reason="sanitizer runtimes not installed")
def test_body_domain_host_build_is_clean_under_asan_and_ubsan():
    """Host code only, as tests/test_sanitizers.py drives it: the setters, the per-env fold and the randomised kernels'
    table reads (rodent CG, rodent with both parts, ant)."""
    src = os.path.join(H.ROOT, "vnl-brax-imitation_amd", "csrc", "vnl_lib.hip")
    out = os.path.join(H.ROOT, "tests", "hostsim", "_build", "libvnl_hostsim_float_asan_body.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-fPIC", "-shared", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-DVNL_REAL=float", "-I" + os.path.join(H.ROOT, "tests", "hostsim", "stub"),
                           "-x", "c++", src, "-o", out])
    env = dict(os.environ, LD_PRELOAD=f"{_san('libasan.so')} {_san('libubsan.so')}",
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "hostsim", "body_domain_sanitizer_driver.py"), out], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert "rodent ok" in p.stdout and "both ok" in p.stdout and "ant ok" in p.stdout and "bad ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
