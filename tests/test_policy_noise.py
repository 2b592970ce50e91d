"""Counter-based policy noise on the CPU: the torch restatement of Philox4x32-10 (ppo_imitation/philox.py) against the
Random123 known-answer vectors, its statistics, and the torch-backend policy with noise="device" (an env's draws depend on
(seed, step, global env index) alone).  The HIP kernel's draws are held to the restatement in tests/test_gpu_policy_noise.py."""
import math

import pytest
import torch

from vnl_brax_imitation_amd.ppo_imitation import ppo_networks, running_statistics


def _philox():
    from vnl_brax_imitation_amd.ppo_imitation import philox

    return philox


KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def test_philox_known_answer_vectors():
    philox = _philox()
    ctr = torch.tensor([c for c, _, _ in KAT], dtype=torch.int64)
    for i, (c, k, want) in enumerate(KAT):
        assert philox.philox4x32(torch.tensor(c, dtype=torch.int64), tuple(k)).tolist() == want
        # batched, with tensor keys
        got = philox.philox4x32(ctr, (torch.tensor(k[0]), torch.tensor(k[1])))
        assert got[i].tolist() == want


@pytest.mark.parametrize("stream,n,mean_lim,var_lim", [(0, 64, 0.0078, 0.0111), (1, 30, 0.0114, 0.0161)])
def test_restatement_statistics(stream, n, mean_lim, var_lim):
    """seed 0, step 0, envs 0..4095: limits 4 / sqrt(N) and 4 sqrt(2 / N) of the N = 4096 n values."""
    philox = _philox()
    env = torch.arange(4096)
    x = philox.normal(0, 0, env, n, stream)
    assert x.shape == (4096, n) and x.dtype == torch.float32
    N = x.numel()
    assert mean_lim <= 4 / math.sqrt(N) * 1.01 and var_lim <= 4 * math.sqrt(2 / N) * 1.01
    xd = x.double()
    print(f"stream {stream}: mean {xd.mean():.5f} var {xd.var(unbiased=False):.5f} max |x| {xd.abs().max():.3f}")
    assert abs(float(xd.mean())) < mean_lim
    assert abs(float(xd.var(unbiased=False)) - 1) < var_lim
    assert len(torch.unique(x, dim=0)) == 4096  # all rows distinct
    assert float(x.abs().max()) <= 5.9  # sqrt(-2 ln 2^-25) = 5.887: the largest value u = 2^-25 can produce
    y = philox.normal(0, 1, env, n, stream).double()
    corr = float(((xd - xd.mean()) * (y - y.mean())).mean() / (xd.std(unbiased=False) * y.std(unbiased=False)))
    print(f"stream {stream}: correlation of step 0 with step 1 {corr:.5f}")
    assert abs(corr) < 0.01
    # a row is a prefix-stable sequence of blocks: a shorter row is the longer one's head
    assert torch.equal(philox.normal(0, 0, env[:8], n - 3, stream), x[:8, :n - 3])


def test_shared_uniform_and_streams():
    philox = _philox()
    r = philox.shared_uniform(0, 0, 30)
    assert r.shape == (30,) and float(r.abs().max()) < 1 and len(torch.unique(r)) == 30
    assert torch.equal(philox.shared_uniform(0, 0, 5), r[:5])
    assert not torch.equal(philox.shared_uniform(0, 1, 30), r)
    env = torch.arange(4)
    a, b = philox.normal(7, 3, env, 8, 0), philox.normal(7, 3, env, 8, 1)
    assert not torch.equal(a, b)
    # the high step bits and the 64-bit seed reach the counter / key
    assert not torch.equal(philox.normal(7, 3 + (1 << 32), env, 8, 0), a)
    assert not torch.equal(philox.normal(7 + (1 << 32), 3, env, 8, 0), a)
    # a step held in a tensor (the policy's counter) is the same step
    assert torch.equal(philox.normal(7, torch.tensor([3]), env, 8, 0), a)


def _policy_setup():
    traj, obs, act = 45, 19, 5
    nets = ppo_networks.make_intention_ppo_networks(traj, obs, act, preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=6, encoder_layer_sizes=(40, 24),
                                                    decoder_layer_sizes=(24, 40))
    g = torch.Generator().manual_seed(0)
    flat = nets.policy_network.init(g)
    norm = running_statistics.init_state(obs)
    t, o = torch.randn(64, traj, generator=g), torch.randn(64, obs, generator=g)
    return ppo_networks.make_inference_fn(nets), (norm, flat), t, o


def _same(a, b):
    (act_a, ex_a), (act_b, ex_b) = a, b
    return torch.equal(act_a, act_b) and all(torch.equal(ex_a[k], ex_b[k]) for k in ex_a)


def test_torch_policy_with_device_noise():
    make_policy, params, t, o = _policy_setup()
    mk = lambda **kw: make_policy(params, backend="torch", noise="device", **kw)  # noqa: E731
    full = mk(seed=5)
    a64, e64 = full(t, o)
    assert set(e64) == {"log_prob", "rand_log_prob", "raw_action", "logits"}
    assert int(full.counter) == 1 and full.counter.dtype == torch.int64 and full.counter.shape == (1,)
    # rows 32..63 of a batch of 64 == a batch of 32 at env_offset 32, bit for bit
    a32, e32 = mk(seed=5, env_offset=32)(t[32:], o[32:])
    assert torch.equal(a64[32:], a32)
    for k in e64:
        assert torch.equal(e64[k][32:], e32[k]), k
    assert not torch.equal(a64[:32], a32)
    # the same (seed, step) twice; the key is ignored
    again = mk(seed=5)(t, o, torch.Generator().manual_seed(99))
    assert _same((a64, e64), again)
    # another step, another seed
    assert not torch.equal(full(t, o)[0], a64) and int(full.counter) == 2
    assert not torch.equal(mk(seed=6)(t, o)[0], a64)
    # step = counter + step_offset; an unroll advances the counter itself
    p = mk(seed=5)
    p.counter.fill_(7)
    x = p(t, o, step_offset=3, advance=False)
    assert int(p.counter) == 7
    q = mk(seed=5, counter=torch.tensor([10]))
    assert _same(x, q(t, o)) and int(q.counter) == 11
    # rand_log_prob: ONE draw shared by all rows -- it is the log-prob of philox.shared_uniform under every row's logits
    philox = _philox()
    dist = ppo_networks.distribution.NormalTanhDistribution(event_size=5)
    r = philox.shared_uniform(5, 0, 5)
    assert torch.equal(e64["rand_log_prob"], dist.log_prob(e64["logits"], r.expand(64, 5)))
    # deterministic: stream 0 only, no extras; preallocated outputs are written in place
    det = mk(seed=5, deterministic=True)
    ad, ed = det(t, o)
    assert ed == {} and torch.equal(ad, dist.mode(e64["logits"]))
    out = {"action": torch.empty(64, 5), "log_prob": torch.empty(64), "rand_log_prob": torch.empty(64),
           "raw_action": torch.empty(64, 5), "logits": torch.empty(64, 10)}
    ao, eo = mk(seed=5)(t, o, out=out)
    assert ao is out["action"] and eo["logits"] is out["logits"] and _same((a64, e64), (ao, eo))


def test_default_noise_mode_is_the_generator_path():
    make_policy, params, t, o = _policy_setup()
    a = make_policy(params, backend="torch")(t, o, torch.Generator().manual_seed(3))
    b = make_policy(params, backend="torch", noise="generator")(t, o, torch.Generator().manual_seed(3))
    assert _same(a, b)
    with pytest.raises(ValueError):
        make_policy(params, backend="torch", noise="philox")


@pytest.mark.parametrize("deterministic", [False, True])
def test_unroll_with_device_noise_on_the_host_simulation(deterministic, monkeypatch):
    """The fused unroll with a device-noise policy (torch backend, host simulation of the env kernels): the policy writing the
    log rows itself == logging through vnl_rollout_post == the generic actor_step loop, and the counter advances by T."""
    import helpers as H
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import acting

    T, extra, runs = 5, ("truncation", "traj"), []
    for fused, direct in ((True, True), (True, False), (False, True)):
        monkeypatch.setattr(acting, "_DIRECT_LOG", direct)
        base = H.hostsim_env(6, "float")
        env = AutoResetWrapper(EpisodeWrapper(base, episode_length=3, action_repeat=1))
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=16, encoder_layer_sizes=(32,),
                                                        decoder_layer_sizes=(32,))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0))
        norm = running_statistics.init_state(base.observation_size)
        policy = ppo_networks.make_inference_fn(nets)((norm, flat), deterministic=deterministic, noise="device", seed=4)
        state = env.reset(torch.Generator().manual_seed(5))
        leaves = []
        for _ in range(2):
            state, data = acting.generate_unroll(env, state, policy, None, T, extra_fields=extra, fused=fused)
            leaves += [x.clone() for x in acting._leaves(data)]
        assert int(policy.counter) == 2 * T
        runs.append(leaves + [state.obs.clone(), state.done.clone()])
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert a.shape == b.shape and torch.equal(a, b)
