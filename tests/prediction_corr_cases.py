"""Shared by tests/test_prediction_corr.py (CPU tier) and tests/test_gpu_prediction_corr.py: inputs and the float64
reference of metrics["prediction_corr"] (reference ppo_imitation/intention_losses.py:186-188)."""
import functools

import numpy as np
import torch

LDS_LIMIT = 60 * 1024  # bytes of LDS the one-workgroup kernel may request (csrc/vnl_ppo.hip)
SMALL_ODD = dict(traj=45, obs=19, act=5, latent=6, enc=(40, 24), dec=(24, 40), val=(72, 56))  # as tests/test_gpu_ppo_update.py
HP = dict(entropy_cost=1e-3, discounting=0.99, reward_scaling=1.0, gae_lambda=0.95, clipping_epsilon=0.2,
          normalize_advantage=True, kl_weight=1e-4)


def fits_one_workgroup(T: int, B: int) -> bool:
    return (2 * T * B + 2 * T) * 4 <= LDS_LIMIT


@functools.lru_cache(maxsize=None)
def rows(T: int, B: int, seed: int = 0):
    """Correlated rows with |mean| >> std on the `vs` side (mean / std = 50): row t of vs is 5 + 0.1 (0.7 z + 0.7 n_t), row
    t of reward 0.1 |m_t| + 0.02 z; z, n_t, m_t ~ N(0, 1) of length B.  float32 [T, B] arrays (read-only)."""
    rng = np.random.default_rng(1000 * T + B + seed)
    z = rng.standard_normal(B)
    vs = (5.0 + 0.1 * (0.7 * z[None] + 0.7 * rng.standard_normal((T, B)))).astype(np.float32)
    reward = (0.1 * np.abs(rng.standard_normal((T, B))) + 0.02 * z[None]).astype(np.float32)
    vs.setflags(write=False), reward.setflags(write=False)
    return vs, reward


def reference(vs: np.ndarray, reward: np.ndarray, scaling: float) -> float:
    """float64 np.corrcoef of the given (float32) inputs, clipped and averaged; the scaling is applied in float32, as the
    kernels and the loss do."""
    x = np.concatenate([vs, reward * np.float32(scaling)], axis=0).astype(np.float64)
    return float(np.clip(np.corrcoef(x), -1.0, 1.0).mean())


def make_update_case(T, B, seed=0, traj=45, obs=19, act=5, latent=6, enc=(40, 24), dec=(24, 40), val=(72, 56)):
    """A small network and a time-major minibatch (the construction of tests/test_gpu_ppo_update.py)."""
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    nets = ppo_networks.make_intention_ppo_networks(traj, obs, act, preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=latent, encoder_layer_sizes=enc,
                                                    decoder_layer_sizes=dec, value_hidden_layer_sizes=val)
    g = torch.Generator().manual_seed(seed)
    flat = torch.cat([nets.policy_network.init(g), nets.value_network.init(g)])
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


def loss_float64(nets, flat, data, norm, noise, hp=HP):
    """The op-by-op torch loss in float64 on the CPU: (metrics, vs) with vs recomputed from the same value network and GAE."""
    from vnl_brax_imitation_amd.ppo_imitation import intention_losses, running_statistics

    n_pol = nets.policy_network.layout.size
    p64 = flat.double()
    d64 = data.map(lambda x: x.double())
    n64 = running_statistics.RunningStatisticsState(norm.count.double(), norm.mean.double(), norm.summed_variance.double(),
                                                    norm.std.double())
    params = intention_losses.PPONetworkParams(policy=p64[:n_pol], value=p64[n_pol:])
    with torch.no_grad():
        _, m = intention_losses.compute_ppo_intention_loss(
            params, n64, d64, None, ppo_network=nets, noise={k: v.double() for k, v in noise.items()}, head="torch",
            time_major=True, **hp)
        values = nets.value_network.apply(n64, params.value, torch.cat([d64.observation, d64.next_observation[-1:]], dim=0))
        trunc = d64.extras["state_extras"]["truncation"]
        vs, _ = intention_losses.compute_gae(truncation=trunc, termination=(1 - d64.discount) * (1 - trunc),
                                             rewards=d64.reward * hp["reward_scaling"], values=values[:-1],
                                             bootstrap_value=values[-1], lambda_=hp["gae_lambda"], discount=hp["discounting"])
    return m, vs
