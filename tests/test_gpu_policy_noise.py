"""The acting kernel drawing its own noise (vnl_policy_forward_noise, MODE 3 of csrc/vnl_policy.hip): the emitted draws against
the torch restatement of Philox4x32-10 (ppo_imitation/philox.py), the same function as vnl_policy_forward on those draws,
independence of batch size / row / how the step is split, and the unroll, graph and trainer paths built on it."""
import ctypes as C
import functools

import pytest
import torch

import helpers as H
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.ppo_imitation import acting, checkpoint, ppo_networks, running_statistics
from vnl_brax_imitation_amd.ppo_imitation import train as ppo

pytestmark = pytest.mark.gpu

NETS = {  # traj, obs, act, latent, encoder, decoder
    "reference": (795, 232, 30, 64, (256, 128), (128, 256)),
    "small-odd": (45, 19, 5, 6, (40, 24), (24, 40)),  # act and latent are no multiples of 4
}
B = 33  # two full 16-env tiles and a one-row tile
SEED, STEP, OFFSET = 0x123456789ABCDEF, 5, 1000  # (the seed's high word and a non-zero env offset reach the kernel)
OUTS = ("action", "raw_action", "log_prob", "rand_log_prob", "logits", "latent_mean", "latent_logvar")


class Case:
    def __init__(self, name):
        from vnl_brax_imitation_amd.ppo_imitation.hip_policy import HipIntentionPolicy

        self.dev = dev = torch.device("cuda:0")
        self.traj_size, self.obs_size, self.act, self.latent, enc, dec = NETS[name]
        n = ppo_networks.make_intention_ppo_networks(self.traj_size, self.obs_size, self.act,
                                                     preprocess_observations_fn=running_statistics.normalize,
                                                     intention_latent_size=self.latent, encoder_layer_sizes=enc,
                                                     decoder_layer_sizes=dec)
        g = torch.Generator().manual_seed(1)
        flat = n.policy_network.init(g)
        flat += 0.05 * torch.randn(flat.shape, generator=g)
        st = running_statistics.update(running_statistics.init_state(self.obs_size),
                                       torch.randn((64, self.obs_size), generator=g) * 2 + 0.3)
        self.flat, self.mean, self.std = flat.to(dev), st.mean.to(dev), st.std.to(dev)
        self.traj = (torch.randn((48, self.traj_size), generator=g) * 0.2).to(dev)
        self.obs = torch.randn((48, self.obs_size), generator=g).to(dev)
        self.hp = HipIntentionPolicy(n.policy_module, self.act, 48, dev)

    def noise(self, rows=slice(0, B), counter=STEP, step_offset=0, env_offset=OFFSET, deterministic=False, record=True):
        """one vnl_policy_forward_noise call -> (outputs incl. action, recorded draws, the counter tensor)"""
        nb = self.traj[rows].shape[0]
        ctr = torch.tensor([counter], dtype=torch.int64, device=self.dev)
        rec = None
        if record:
            rec = {"eps_latent": torch.full((nb, self.latent), 9.0, device=self.dev),
                   "eps_action": torch.full((nb, self.act), 9.0, device=self.dev),
                   "rand_action": torch.full((self.act,), 9.0, device=self.dev)}
        a, ex = self.hp.forward_noise(self.flat, self.mean, self.std, self.traj[rows], self.obs[rows], ctr,
                                      step_offset=step_offset, seed=SEED, env_offset=env_offset, deterministic=deterministic,
                                      eps_out=rec)
        return {"action": a, **ex}, rec, ctr


@pytest.fixture(scope="module", params=list(NETS))
def case(request):
    c = Case(request.param)
    c.out, c.rec, _ = c.noise()  # the stochastic call every test compares against: computed once, left unchanged
    return c


def test_emitted_draws_match_the_restatement(case):
    """<= 1e-5 absolute: |x| <= 5.9 and logf, sqrtf, sinf, cosf each within ~2 ulp is under ~8 ulp of 5.9 = 5.6e-6; a wrong
    Philox bit misses by O(1)."""
    from vnl_brax_imitation_amd.ppo_imitation import philox

    env = OFFSET + torch.arange(B)
    for name, n, stream in (("eps_latent", case.latent, 0), ("eps_action", case.act, 1)):
        ref = philox.normal(SEED, STEP, env, n, stream)
        err = float((case.rec[name].cpu().double() - ref.double()).abs().max())
        print(f"{name}: max |kernel - restatement| = {err:.2e}")
        assert err <= 1e-5, (name, err)
    r = case.rec["rand_action"].cpu()
    err = float((r.double() - philox.shared_uniform(SEED, STEP, case.act).double()).abs().max())
    print(f"rand_action: max |kernel - restatement| = {err:.2e}")
    assert err <= 1e-5 and float(r.abs().max()) < 1


@pytest.mark.parametrize("deterministic", [False, True])
def test_same_function_as_the_caller_supplied_noise_kernel(case, deterministic):
    """vnl_policy_forward fed the recorded draws returns the noise call's bits, on every output."""
    out, rec = (case.out, case.rec) if not deterministic else case.noise(deterministic=True)[:2]
    sl = slice(0, B)
    a, ex = case.hp.forward(case.flat, case.mean, case.std, case.traj[sl], case.obs[sl], rec["eps_latent"],
                            None if deterministic else rec["eps_action"], deterministic,
                            rand_action=None if deterministic else rec["rand_action"])
    ref = {"action": a, **ex}
    keys = ("action", "latent_mean", "latent_logvar") if deterministic else OUTS
    assert set(keys) <= set(out) and set(keys) <= set(ref)
    for k in keys:
        assert torch.equal(out[k], ref[k]), (k, float((out[k] - ref[k]).abs().max()))
    if deterministic:  # stream 0 only: the other records are left alone, the latent draw is the stochastic call's
        assert torch.equal(rec["eps_latent"], case.rec["eps_latent"])
        assert float(rec["eps_action"].min()) == 9.0 and float(rec["rand_action"].min()) == 9.0
    # the optional records null: the other outputs are unchanged
    bare = case.noise(deterministic=deterministic, record=False)[0]
    for k in keys:
        assert torch.equal(out[k], bare[k]), k


def test_independent_of_batch_size_row_and_step_split(case):
    big = case.noise(rows=slice(0, 48), env_offset=0)[0]
    part, _, ctr = case.noise(rows=slice(32, 48), env_offset=32)
    for k in OUTS:
        assert torch.equal(big[k][32:48], part[k]), k
    assert not torch.equal(big["action"][:16], part["action"])
    a, _, ctr_a = case.noise(counter=7, step_offset=3)
    b, _, ctr_b = case.noise(counter=10, step_offset=0)
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k
    assert int(ctr_a) == 7 and int(ctr_b) == 10 and int(ctr) == STEP  # the kernel leaves the counter unwritten
    assert not torch.equal(a["action"], case.out["action"])  # another step, other draws


def test_abi_errors(case):
    lib, hp = case.hp.lib, case.hp
    f32 = lambda *s: torch.zeros(s, device=case.dev)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    ctr = torch.zeros(1, dtype=torch.int64, device=case.dev)
    action = torch.full((B, case.act), 7.0, device=case.dev)
    bufs = (f32(B, case.act), f32(B), f32(B, 2 * case.act), f32(B, case.latent), f32(B, case.latent), f32(B))

    def call(step_base, step_offset=0, env_offset=0):
        nz = _lib.PolicyNoise()
        nz.seed, nz.step_base, nz.step_offset, nz.env_offset = 1, p(step_base), step_offset, env_offset
        return lib.vnl_policy_forward_noise(hp.h, p(case.flat), p(case.mean), p(case.std), p(case.traj), p(case.obs),
                                            C.byref(nz), B, 0, p(action), *[p(t) for t in bufs], C.c_void_p(0))

    for kw, word in ((dict(step_base=None), "step_base"), (dict(step_base=ctr, step_offset=-1), "negative"),
                     (dict(step_base=ctr, env_offset=-1), "negative"),
                     (dict(step_base=ctr, env_offset=2 ** 32 - 1 - B), "2^32")):
        rc = call(**kw)
        msg = lib.vnl_last_error().decode()
        assert rc == -1 and word in msg, (kw, rc, msg)  # VNL_ERR_ARG
    torch.cuda.synchronize()
    assert float(action.min()) == 7.0  # nothing was launched
    assert call(ctr, env_offset=2 ** 32 - 2 - B) == 0  # the largest env index allowed
    torch.cuda.synchronize()
    assert float(action.abs().max()) <= 1.0
    with pytest.raises(_lib.VnlError):
        case.noise(env_offset=-1)


# ---- the unroll ----------------------------------------------------------------------------------------------------------
def _rodent_setup(B, seed=9):
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper

    dev = torch.device("cuda:0")
    base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=4, action_repeat=1))
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    policy = ppo_networks.make_inference_fn(nets)((norm, flat), noise="device", seed=seed)
    return env, policy, env.reset(torch.Generator().manual_seed(5))


def _state_leaves(s):
    return [s.obs, s.done, s.reward] + [s.info[k] for k in ("steps", "truncation", "traj", "cur_frame", "sub_clip_frame")] + \
        [s.pipeline_state.raw(n) for n in s.pipeline_state._FIELDS]


def test_graphed_unroll_and_direct_logging(monkeypatch):
    """64 rodent envs, unroll length 5 (odd), AutoReset(Episode): two replays of GraphedUnroll == two eager fused unrolls,
    bit for bit, in every Transition leaf and the env state; the counter ends at 10; the policy writing the unroll's log rows
    itself == the same unroll logging through vnl_rollout_post."""
    T, extra = 5, ("truncation", "traj")
    runs = {}
    for mode in ("eager", "graphed", "eager-post"):
        monkeypatch.setattr(acting, "_DIRECT_LOG", mode != "eager-post")
        env, policy, state = _rodent_setup(64)
        g = acting.GraphedUnroll(env, state, policy, None, T, extra_fields=extra) if mode == "graphed" else None
        assert int(policy.counter) == 0  # building the graph consumes no noise
        datas = []
        for _ in range(2):
            state, data = g() if g else acting.generate_unroll(env, state, policy, None, T, extra_fields=extra, fused=True)
            datas.append([x.clone() for x in acting._leaves(data)])
        assert int(policy.counter) == 10
        runs[mode] = (datas, [x.clone() for x in _state_leaves(state)])
    d0, s0 = runs["eager"]
    i_trunc = [i for i, x in enumerate(acting._leaves(data)) if x is data.extras["state_extras"]["truncation"]][0]
    assert float(d0[0][i_trunc].sum()) > 0  # episodes of 4 steps did end inside the unroll
    assert not torch.equal(d0[0][1], d0[1][1])  # the second unroll drew other actions
    for other in ("graphed", "eager-post"):
        d1, s1 = runs[other]
        for a_, b_ in zip(d0, d1):
            for a, b in zip(a_, b_):
                assert a.shape == b.shape and torch.equal(a, b), other
        for a, b in zip(s0, s1):
            assert torch.equal(a, b), other


# ---- the trainer ---------------------------------------------------------------------------------------------------------
def _train(tmp=None, restore=None, steps=2):
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    dev = torch.device("cuda:0")
    env = RodentTracking(H.reference_clip(), num_envs=64, device=dev, **H.env_kwargs())
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=60,
                           encoder_layer_sizes=(128, 128), decoder_layer_sizes=(128, 128))
    log = []
    _, (norm, flat), _ = ppo.train(
        environment=env, num_timesteps=steps * 64 * 5, episode_length=150, num_envs=64, learning_rate=1e-3,
        entropy_cost=1e-2, discounting=0.95, unroll_length=5, batch_size=16, num_minibatches=4,
        num_updates_per_batch=2, num_evals=1, normalize_observations=True, network_factory=nf, num_eval_envs=0,
        eval_env=None, seed=3, policy_noise="device", restore_from=restore, progress_fn=lambda s, m: log.append(m))
    return flat, log[-1], ppo.train.last_training_state, ppo.train.last_ppo_network


def test_trainer_with_device_noise_is_reproducible_and_resumes(tmp_path):
    f0, m0, ts0, net = _train()
    f1, m1, ts1, _ = _train()
    assert torch.equal(f0, f1)
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in m0.values())
    assert int(ts0.policy_counter) == 2 * 5  # two training steps of one 5-step unroll each
    n_pol = net.policy_network.layout.size
    path = checkpoint.save_params(str(tmp_path / "ck"), (ts0.normalizer_params, ts0.params[:n_pol]), net,
                                  value_params=ts0.params[n_pol:], optimizer_state=ts0.optimizer_state,
                                  env_steps=ts0.env_steps, policy_counter=ts0.policy_counter)
    assert int(checkpoint.load_params(path, net)["policy_counter"]) == 10
    _, m2, ts2, _ = _train(restore=path, steps=1)
    assert int(ts2.policy_counter) == 10 + 5  # continued from the restored counter, not from 0
