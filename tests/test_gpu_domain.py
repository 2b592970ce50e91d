"""Domain randomisation on the device (vnl_env_set_domain; the randomised instantiations of csrc/vnl_domain.hip).

The randomised kernels are the unrandomised ones with five model tables read per env: on the same parameters they must
give the same bits, and env i of a randomised batch the bits of an unrandomised env on env i's model."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import domain_cases as D
import helpers as H
import parity as P
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.envs.rodent import RodentTracking
from vnl_brax_imitation_amd.model import mjcf
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

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
    out = {k: getattr(ps, k).cpu().clone() for k in ("qpos", "qvel", "qacc_warmstart")}
    out.update(obs=st.obs.cpu().clone(), reward=st.reward.cpu().clone(), done=st.done.cpu().clone(),
               metrics=st.info["_raw"]["metrics"].cpu().clone())
    return out


def _assert_identity(base, sf, noise, acts):
    env = base.with_domain(D.identity(base.sys, base.num_envs))
    a, b = _run(base, sf, noise, acts), _run(env, sf, noise, acts)
    same = {k: torch.equal(a[k], b[k]) for k in a}
    assert all(same.values()), same
    assert torch.isfinite(b["qvel"]).all()


def test_identity_domain_specialised_rodent_kernel_4096_envs():
    B = 4096
    base = _rodent(B)
    assert int(base.dims.kernel_specialised) == 1
    _assert_identity(base, *_inputs(B, seed=1))


def test_identity_domain_generic_kernel_ant_and_newton_rodent():
    from vnl_brax_imitation_amd import envs

    m = mjcf.CompiledModel.load(os.path.join(H.ROOT, "vnl-brax-imitation_amd", "data", "ant.npz"))
    ant = envs.get_environment("ant", params=D.ANT_PARAMS, clip_length=60, episode_length=20, reference_clip=D.ant_clip(m),
                               model=m, num_envs=512, device=DEV)
    assert int(ant.dims.kernel_specialised) == 0
    sf, noise, acts = _inputs(512, nq=15, nu=8, seed=2)
    _assert_identity(ant, np.zeros_like(sf), noise * 0, acts)
    mn = copy.deepcopy(H.model())
    mn.scalars.update(solver_newton=1)
    newton = _rodent(1024, mn)
    _assert_identity(newton, *_inputs(1024, seed=3))


def test_randomised_groups_equal_unrandomised_envs_on_their_models():
    """256 envs, 8 parameter sets in groups of 32: each group bit for bit an unrandomised env on its own model."""
    B, G = 256, 8
    base = _rodent(B)
    sets = D.random_domain(base.sys, G, 10)
    grp = np.arange(B) // (B // G)
    dom = {k: v[grp] for k, v in sets.items()}
    sf, noise, acts = _inputs(B, seed=4)
    got = _run(base.with_domain(dom), sf, noise, acts)
    for g in range(G):
        rows = np.nonzero(grp == g)[0]
        one = _rodent(len(rows), D.model_with(base.sys, sets, g))
        want = _run(one, sf[rows], noise[rows], acts[:, rows])
        for k, v in want.items():
            assert torch.equal(got[k][rows], v), (g, k)


@pytest.mark.parametrize("scale", [dict(cg_friction=0.4), dict(act_gain=1.3)], ids=["friction0.6", "gain1.3x"])
def test_unrandomised_kernels_follow_the_oracle_on_modified_models(scale):
    """parity.control_step_follow against the float64 oracle on parameters the repository never ran before (friction 0.6,
    gain 1.3x): the existing error bounds hold."""
    B = 256
    m = D.model_with(H.model(), D.scaled_domain(H.model(), 1, **scale), 0)
    env = _rodent(B, m)
    o64, o32 = H.make_oracle(env, "f64"), H.make_oracle(env, "f32")
    sf, noise, acts = _inputs(B, seed=5, steps=1)
    st, err, dev, rep, ost = P.control_step_follow(env, o64, o32, sf, noise, acts[0])
    print(f"\n[{scale}, control step] " + ", ".join(f"{k} max {v.max():.2e}" for k, v in err.items()))
    # the flipped-decision allowance of every model other than the compiled rodent (tests/test_generic_model.py,
    # test_ant_env.py, test_newton_sparse.py): at friction 0.6 more contacts sit on their cone's switching point, and 6 of
    # these 256 envs show a later decision flipped against the oracle's drifted state (2.3 %, over the compiled rodent's 1 %);
    # the error bounds of check_control_step hold for every env, flipped or not
    P.check_control_step(err, dev, rep, max_flipped=B // 8)


def test_graphed_unroll_of_a_randomised_env_equals_the_eager_unroll():
    B, T = 130, 6
    out = []
    for graphed in (False, True):
        base = _rodent(B)
        env = W.AutoResetWrapper(W.EpisodeWrapper(base.with_domain(D.random_domain(base.sys, B, 12)), episode_length=4,
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


def test_training_with_a_randomization_fn(monkeypatch):
    """A short train(..., randomization_fn=fn): finite losses, and the tables the kernels read (vnl_env_scratch dom_*) are
    what fn returned, for the training env (per-rank batch) and the eval env (num_eval_envs)."""
    returned, wrapped = [], []

    def fn(sys, num_envs, rng):
        u = lambda n: torch.rand((num_envs, n), generator=rng, dtype=torch.float64)  # noqa: E731
        d = {"cg_friction": torch.as_tensor(sys.cg_friction[:, 0]) * (0.4 + 1.2 * u(sys.cg_friction.shape[0])),
             "act_gain": torch.as_tensor(sys.act_gain) * (0.7 + 0.6 * u(len(sys.act_gain)))}
        returned.append(d)
        return d

    real_wrap = W.wrap

    def recording_wrap(*a, **k):
        w = real_wrap(*a, **k)
        wrapped.append(w)
        return w

    monkeypatch.setattr(W, "wrap", recording_wrap)
    env = _rodent(64)
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=60,
                           encoder_layer_sizes=(128, 128), decoder_layer_sizes=(128, 128))
    _, _, metrics = ppo.train(
        environment=env, num_timesteps=2 * 64 * 5, episode_length=20, num_envs=64, learning_rate=1e-3, entropy_cost=1e-2,
        discounting=0.95, unroll_length=5, batch_size=16, num_minibatches=4, num_updates_per_batch=2, num_evals=2,
        normalize_observations=True, network_factory=nf, num_eval_envs=32, seed=1, randomization_fn=fn)
    for k in ("training/total_loss", "training/policy_loss", "training/v_loss", "eval/episode_reward"):
        assert k in metrics and np.isfinite(float(metrics[k])), k
    assert env.domain is None and len(returned) == 2 and len(wrapped) == 2
    for d, w, n in zip(returned, wrapped, (64, 32)):
        inner = w.env.env
        assert inner.num_envs == n
        assert torch.equal(inner.domain_table("dom_mu"), d["cg_friction"].to(torch.float32))
        assert torch.equal(inner.domain_table("dom_gain"), d["act_gain"].to(torch.float32))
