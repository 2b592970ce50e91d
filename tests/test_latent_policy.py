"""Latent-driven acting on the CPU: the decoder policy of ppo_networks.make_decoder_inference_fn on the torch backend -- the
same torch ops as IntentionNetwork.apply from the latent on, the prior draw on stream 0 of the counter-based noise, the call
conventions of the device-noise policy, and a generic unroll on the host simulation of the env kernels.  The HIP kernel is
held to the same function in tests/test_gpu_latent_policy.py."""
import pytest
import torch

import latent_policy_cases as LC
from vnl_brax_imitation_amd.ppo_imitation import philox, ppo_networks, running_statistics

LOGGED = {"log_prob", "rand_log_prob", "raw_action", "logits"}


@pytest.fixture(scope="module")
def net():
    return LC.Net("small-odd")


def _mk(net, **kw):
    return ppo_networks.make_decoder_inference_fn(net.nets)((net.norm, net.flat), backend="torch", **kw)


def _same(a, b):
    (act_a, ex_a), (act_b, ex_b) = a, b
    return torch.equal(act_a, act_b) and set(ex_a) == set(ex_b) and all(torch.equal(ex_a[k], ex_b[k]) for k in ex_a)


def test_given_latent_is_the_full_networks_function(net):
    """z of IntentionNetwork.apply fed to the decoder policy: apply's logits, bit for bit (the same torch ops)"""
    mod = net.nets.policy_module
    eps = torch.randn((LC.ROWS, net.latent), generator=torch.Generator().manual_seed(3))
    logits, mean, logvar = net.nets.policy_network.apply(net.norm, net.flat, net.traj, net.obs, eps)
    z = mean + eps * torch.exp(0.5 * logvar)
    m2, lv2 = mod.encode(net.flat, net.traj)
    assert torch.equal(m2, mean) and torch.equal(lv2, logvar)
    a, ex = _mk(net, latent=z, seed=5)(net.traj, net.obs)
    assert set(ex) == LOGGED and torch.equal(ex["logits"], logits)
    # the tail: streams 1 and 2 at (seed, step 0, row), as the device-noise policy of the full network draws them
    dist = net.nets.parametric_action_distribution
    env = torch.arange(LC.ROWS)
    raw = dist.sample_no_postprocessing(logits, philox.normal(5, 0, env, net.act, philox.STREAM_ACTION))
    assert torch.equal(ex["raw_action"], raw) and torch.equal(a, dist.postprocess(raw))
    assert torch.equal(ex["log_prob"], dist.log_prob(logits, raw))
    r = philox.shared_uniform(5, 0, net.act)
    assert torch.equal(ex["rand_log_prob"], dist.log_prob(logits, r.expand(LC.ROWS, net.act)))
    # a callable latent receives (traj, obs) and runs in front of the decoder
    seen = []

    def controller(traj, obs):
        seen.append((traj, obs))
        return z

    assert _same((a, ex), _mk(net, latent=controller, seed=5)(net.traj, net.obs))
    assert len(seen) == 1 and seen[0][0] is net.traj and seen[0][1] is net.obs
    # a tensor latent is read live
    live = z.clone()
    pol = _mk(net, latent=live, seed=5)
    first = pol(net.traj, net.obs, advance=False)
    live.mul_(-1.0)
    second = pol(net.traj, net.obs, advance=False)
    assert _same((a, ex), first) and not torch.equal(first[0], second[0])


def test_prior_draw_counter_and_outputs(net):
    t, o = net.traj, net.obs
    zo = torch.full((LC.ROWS, net.latent), 9.0)
    pol = _mk(net, seed=LC.SEED, env_offset=LC.OFFSET, latent_out=zo, counter=torch.tensor([LC.STEP]))
    assert pol.noise == "device" and pol.deterministic is False
    a, ex = pol(t, o, step_offset=2, advance=False)
    assert int(pol.counter) == LC.STEP and pol.counter.dtype == torch.int64 and pol.counter.shape == (1,)
    env = LC.OFFSET + torch.arange(LC.ROWS)
    z = philox.normal(LC.SEED, LC.STEP + 2, env, net.latent, philox.STREAM_LATENT)
    assert torch.equal(zo, z)  # latent_out holds the z used: stream 0 at (seed, counter + step_offset, env_offset + row)
    assert _same((a, ex), _mk(net, latent=z, seed=LC.SEED, env_offset=LC.OFFSET, counter=torch.tensor([LC.STEP + 2]))(t, o))
    # the same step reached through the counter alone; advance adds one
    q = _mk(net, seed=LC.SEED, env_offset=LC.OFFSET, counter=torch.tensor([LC.STEP + 2]))
    assert _same((a, ex), q(t, o)) and int(q.counter) == LC.STEP + 3
    assert not torch.equal(q(t, o)[0], a)
    # rows 32..47 of the batch == a batch of 16 at env_offset + 32; the key argument is ignored
    part = _mk(net, seed=LC.SEED, env_offset=LC.OFFSET + 32, counter=torch.tensor([LC.STEP + 2]))
    ap, ep = part(t[32:], o[32:], torch.Generator().manual_seed(1))
    assert torch.equal(ap, a[32:]) and all(torch.equal(ep[k], ex[k][32:]) for k in ex)
    # latent_out with a given latent holds that latent
    zo.fill_(9.0)
    _mk(net, latent=net.z, latent_out=zo)(t, o)
    assert torch.equal(zo, net.z)
    # deterministic: no extras, the mode; preallocated outputs are written in place
    dist = net.nets.parametric_action_distribution
    det = _mk(net, seed=LC.SEED, env_offset=LC.OFFSET, counter=torch.tensor([LC.STEP + 2]), deterministic=True)
    ad, ed = det(t, o)
    assert ed == {} and det.deterministic is True and torch.equal(ad, dist.mode(ex["logits"]))
    out = {"action": torch.empty(LC.ROWS, net.act), "log_prob": torch.empty(LC.ROWS), "rand_log_prob": torch.empty(LC.ROWS),
           "raw_action": torch.empty(LC.ROWS, net.act), "logits": torch.empty(LC.ROWS, 2 * net.act)}
    ao, eo = _mk(net, seed=LC.SEED, env_offset=LC.OFFSET, counter=torch.tensor([LC.STEP + 2]))(t, o, out=out)
    assert ao is out["action"] and eo["logits"] is out["logits"] and _same((a, ex), (ao, eo))


def test_argument_validation(net):
    with pytest.raises(ValueError, match="shape"):
        _mk(net, latent=torch.zeros(LC.ROWS, net.latent + 1))
    with pytest.raises(ValueError, match="shape"):
        _mk(net, latent=torch.zeros(LC.ROWS - 1, net.latent))(net.traj, net.obs)  # (the batch is known at the call)
    with pytest.raises(ValueError, match="float32"):
        _mk(net, latent=torch.zeros(LC.ROWS, net.latent, dtype=torch.float64))
    with pytest.raises(ValueError, match="prior"):
        _mk(net, latent="posterior")
    with pytest.raises(ValueError, match="negative"):
        _mk(net, env_offset=-1)
    with pytest.raises(ValueError, match="shape"):
        _mk(net, latent=lambda traj, obs: torch.zeros(obs.shape[0], net.latent + 2))(net.traj, net.obs)
    with pytest.raises(ValueError, match="backend"):
        ppo_networks.make_decoder_inference_fn(net.nets)((net.norm, net.flat), backend="triton")
    with pytest.raises(ValueError, match="counter"):
        _mk(net, counter=torch.zeros(1, dtype=torch.int32))
    other = ppo_networks.make_intention_ppo_networks(45, 19, 5, preprocess_observations_fn=lambda o, p: o * 2)
    with pytest.raises(ValueError, match="preprocessor"):
        ppo_networks.make_decoder_inference_fn(other)


def test_generic_unroll_on_the_host_simulation():
    """three steps of acting.generate_unroll (the actor_step loop) at 4 envs of the float host build, decoder policy in prior
    mode: the four policy extras are logged, the counter advances by one per step, the recorded z is that of the last step"""
    import helpers as H
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import acting

    base = H.hostsim_env(4, "float")
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=3, action_repeat=1))
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,), decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0))
    norm = running_statistics.init_state(base.observation_size)
    zo = torch.zeros(4, 16)
    policy = ppo_networks.make_decoder_inference_fn(nets)((norm, flat), backend="torch", seed=4, latent_out=zo)
    state = env.reset(torch.Generator().manual_seed(5))
    state, data = acting.generate_unroll(env, state, policy, None, 3, extra_fields=("truncation",), fused=False)
    assert int(policy.counter) == 3
    px = data.extras["policy_extras"]
    assert set(px) == LOGGED
    na = base.action_size
    assert px["logits"].shape == (3, 4, 2 * na) and px["raw_action"].shape == (3, 4, na) and px["log_prob"].shape == (3, 4)
    assert data.action.shape == (3, 4, na) and float(data.action.abs().max()) <= 1.0
    assert all(bool(torch.isfinite(v).all()) for v in px.values())
    assert torch.equal(zo, philox.normal(4, 2, torch.arange(4), 16, philox.STREAM_LATENT))
    # step t of the unroll is the policy called at counter t on the logged observation
    again = ppo_networks.make_decoder_inference_fn(nets)((norm, flat), backend="torch", seed=4, counter=torch.tensor([1]))
    a1, e1 = again(None, data.observation[1])
    assert torch.equal(a1, data.action[1]) and torch.equal(e1["logits"], px["logits"][1])
