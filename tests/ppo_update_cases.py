"""The inputs of one PPO minibatch step -- networks, flat parameters, a Transition batch, normaliser state, noise -- and the
loss coefficients, shared by tests/test_gpu_ppo_update.py, tools/ppo_update_bench.py and the benchmark."""
import torch


def make(traj, obs, act, latent, enc, dec, val, T, B, seed=0):
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    nets = ppo_networks.make_intention_ppo_networks(traj, obs, act, preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=latent, encoder_layer_sizes=enc,
                                                    decoder_layer_sizes=dec, value_hidden_layer_sizes=val)
    g = torch.Generator().manual_seed(seed)
    flat = torch.cat([nets.policy_network.init(g), nets.value_network.init(g)])
    # LayerNorm scale / bias and the biases away from their trivial initial values, so that their gradients matter
    flat = flat + 0.05 * torch.randn(flat.shape, generator=g)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    data = acting.Transition(
        observation=2.0 * r(T, B, obs) + 0.5, action=torch.tanh(r(T, B, act)), reward=0.1 * r(T, B).abs(),
        discount=(torch.rand(T, B, generator=g) > 0.1).float(), next_observation=2.0 * r(T, B, obs) + 0.5,
        extras={"policy_extras": {"raw_action": 0.5 * r(T, B, act), "log_prob": -20.0 + r(T, B)},
                "state_extras": {"truncation": (torch.rand(T, B, generator=g) > 0.9).float(), "traj": 0.3 * r(T, B, traj)}})
    norm = running_statistics.init_state(obs)
    norm = running_statistics.update(norm, data.observation)
    noise = {"latent": r(T, B, latent), "entropy": r(T, B, act)}
    return nets, flat, data, norm, noise


HP = dict(entropy_cost=1e-3, discounting=0.99, reward_scaling=1.0, gae_lambda=0.95, clipping_epsilon=0.2,
          normalize_advantage=True, kl_weight=1e-4)
