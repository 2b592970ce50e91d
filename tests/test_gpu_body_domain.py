"""Body-domain randomisation on the device (vnl_env_set_body_domain; the randomised instantiations of csrc/vnl_domain.hip).

The randomised kernels are the unrandomised ones with the inertial tables of body_inertias read per env: on the compiled
values they must give the same bits, and env i of a randomised batch the bits of an unrandomised env on env i's model."""
import copy

import numpy as np
import pytest
import torch

import body_domain_cases as BD
import domain_cases as D
import helpers as H
import parity as P
from oracle.oracle import Oracle
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.envs.rodent import RodentTracking
from vnl_brax_imitation_amd.model import blob
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rodent(B, model=None):
    kw = H.env_kwargs() if model is None else dict(H.env_kwargs(), model=model)
    return RodentTracking(H.reference_clip(), num_envs=B, device=DEV, **kw)


def _inputs(B, nq=74, nu=30, seed=0, steps=3):
    rng = np.random.default_rng(seed)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((B, nq))).astype(np.float32)
    acts = np.clip(0.3 * rng.standard_normal((steps, B, nu)), -1, 1).astype(np.float32)
    return sf, noise, acts


def _run(env, sf, noise, acts) -> dict:
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    for a in acts:
        st = env.step(st, torch.from_numpy(a))
    ps = st.pipeline_state
    out = {k: ps.raw(k).cpu().clone() for k in ps._FIELDS}
    out.update(obs=st.obs.cpu().clone(), reward=st.reward.cpu().clone(), done=st.done.cpu().clone(),
               metrics=st.info["_raw"]["metrics"].cpu().clone(), traj=st.info["traj"].cpu().clone())
    return out


def _assert_identity(base, sf, noise, acts):
    env = base.with_body_domain(BD.identity(base.sys, base.num_envs))
    a, b = _run(base, sf, noise, acts), _run(env, sf, noise, acts)
    same = {k: torch.equal(a[k], b[k]) for k in a}
    assert all(same.values()), same
    assert torch.isfinite(b["qvel"]).all()
    mass = np.asarray(base.sys.arrays["body_mass"], np.float64)
    want = torch.full((base.num_envs, 1), 1.0 / mass.sum(), dtype=torch.float64).to(torch.float32)
    assert torch.equal(env.domain_table("dom_tminv"), want)


def test_identity_body_domain_specialised_rodent_kernel_4096_envs():
    B = 4096
    base = _rodent(B)
    assert int(base.dims.kernel_specialised) == 1
    _assert_identity(base, *_inputs(B, seed=1))


def test_identity_body_domain_generic_kernel_ant_and_newton_rodent_4096_envs():
    from vnl_brax_imitation_amd import envs

    m = BD.packaged("ant")
    ant = envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(m),
                               model=m, num_envs=4096, device=DEV)
    assert int(ant.dims.kernel_specialised) == 0
    sf, noise, acts = _inputs(4096, nq=15, nu=8, seed=2)
    _assert_identity(ant, np.zeros_like(sf), noise * 0, acts)
    mn = copy.deepcopy(H.model())
    mn.scalars.update(solver_newton=1)
    _assert_identity(_rodent(4096, mn), *_inputs(4096, seed=3))


def test_body_randomised_groups_equal_unrandomised_envs_on_their_models():
    """256 envs, 8 parameter sets (mass and ipos) in groups of 32: each group bit for bit an unrandomised env on its own model."""
    B, G = 256, 8
    base = _rodent(B)
    sets = BD.group_domain(base.sys, G, 10)
    grp = np.arange(B) // (B // G)
    dom = {k: v[grp] for k, v in sets.items()}
    sf, noise, acts = _inputs(B, seed=4)
    got = _run(base.with_body_domain(dom), sf, noise, acts)
    for g in range(G):
        rows = np.nonzero(grp == g)[0]
        one = _rodent(len(rows), BD.model_with(base.sys, sets, g))
        want = _run(one, sf[rows], noise[rows], acts[:, rows])
        for k, v in want.items():
            assert torch.equal(got[k][rows], v), (g, k)
    assert not torch.equal(got["qvel"], _run(base, sf, noise, acts)["qvel"])


def test_four_field_and_body_domain_compose_on_the_device():
    """Both parts in either order give the same bits, and equal an unrandomised env on the model of both (one group)."""
    B = 64
    base = _rodent(B)
    sets, four = BD.group_domain(base.sys, 1, 11), D.random_domain(base.sys, 1, 12)
    body = {k: np.repeat(v, B, 0) for k, v in sets.items()}
    dom4 = {k: np.repeat(v, B, 0) for k, v in four.items()}
    sf, noise, acts = _inputs(B, seed=5, steps=2)
    a = _run(base.with_domain(dom4).with_body_domain(body), sf, noise, acts)
    b = _run(base.with_body_domain(body).with_domain(dom4), sf, noise, acts)
    c = _run(_rodent(B, BD.model_with(D.model_with(base.sys, four, 0), sets, 0)), sf, noise, acts)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


class RowOracles:
    """One oracle per env row behind the batch interface parity.follow_compare drives (new_state, env_step_follow,
    env_step): row i of every call goes to oracle i, the oracle of env i's own model."""

    def __init__(self, oracles):
        self.o = list(oracles)
        self.real = self.o[0].real

    def new_state(self, B):
        assert B == len(self.o)
        return self.o[0].new_state(B)

    def _each(self, st, call):
        extra = []
        for i, o in enumerate(self.o):
            row = {k: np.ascontiguousarray(v[i:i + 1]) for k, v in st.items()}
            res = call(o, row, i)
            row, rest = (res[0], res[1:]) if isinstance(res, tuple) else (res, ())
            for k, v in st.items():
                v[i:i + 1] = row[k]
            extra.append(rest)
        return st, [np.concatenate(x) for x in zip(*extra)]

    def env_step_follow(self, st, action, follow):
        st, (tr, rep) = self._each(st, lambda o, row, i: o.env_step_follow(row, action[i:i + 1], follow[i:i + 1]))
        return st, tr, rep

    def env_step(self, st, action):
        return self._each(st, lambda o, row, i: o.env_step(row, action[i:i + 1]))[0]


def test_random_body_domain_follows_the_oracle_of_each_envs_model():
    """256 envs of a random body domain (mass, moments and ipos of every body of every env drawn on their own), one control
    step of the RANDOMISED kernels against the float64 oracle of each env's own model following the product's decisions
    (parity.control_step_follow / check_control_step, per-env bounds as they are; one oracle per env row, each on a deep copy
    of the model with env i's three arrays and body_inertia_full recomputed in NumPy).  The share of envs allowed to show a
    later flipped decision is the suite's allowance for models other than the compiled rodent, B / 8."""
    B = 256
    base = _rodent(B)
    m = base.sys
    body = BD.random_body_domain(m, B, 13)
    env = base.with_body_domain(body)
    dims = [int(m.scalars[k]) for k in ("nbody", "nq", "nv", "nu")]

    def oracles(precision):
        out = []
        for i in range(B):
            o = Oracle(blob.to_blob(BD.model_with(m, body, i)), precision)
            o.bind_env(base.env_spec(), base.clip_arrays(0), *dims)
            out.append(o)
        return RowOracles(out)

    o64, o32 = oracles("f64"), oracles("f32")
    sf, noise, acts = _inputs(B, seed=6, steps=1)
    st, err, dev, rep, ost = P.control_step_follow(env, o64, o32, sf, noise, acts[0])
    print("\n[random body domain, control step] " + ", ".join(f"{k} max {v.max():.2e}" for k, v in err.items()))
    flipped = P.check_control_step(err, dev, rep, max_flipped=B // 8)
    print(f"[random body domain] envs with a flipped later decision: {flipped} of {B}")
    # the domain did change the batch: env 0 run unrandomised ends elsewhere
    plain = base.step(base.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise)), torch.from_numpy(acts[0]))
    assert not torch.equal(plain.pipeline_state.qvel.cpu(), st.pipeline_state.qvel.cpu())


def test_graphed_unroll_of_a_body_randomised_env_equals_the_eager_unroll():
    B, T = 130, 6
    out = []
    for graphed in (False, True):
        base = _rodent(B)
        env = W.AutoResetWrapper(W.EpisodeWrapper(base.with_body_domain(BD.random_body_domain(base.sys, B, 12)), episode_length=4,
                                                  action_repeat=1))
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=16, encoder_layer_sizes=(32,),
                                                        decoder_layer_sizes=(32,))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(DEV)
        policy = ppo_networks.make_inference_fn(nets)((running_statistics.init_state(base.observation_size, device=DEV), flat))
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        key = torch.Generator(device=DEV).manual_seed(11)
        g = acting.GraphedUnroll(env, state, policy, key, T, extra_fields=("truncation",)) if graphed else None
        datas = []
        for _ in range(3):
            if graphed:
                state, data = g()
            else:
                state, data = acting.generate_unroll(env, state, policy, key, T, extra_fields=("truncation",), fused=True)
            datas.append([x.clone() for x in acting._leaves(data)])
        out.append((state, datas))
    (s0, d0), (s1, d1) = out
    for a_, b_ in zip(d0, d1):
        for a, b in zip(a_, b_):
            assert torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n
