"""Case data of the latent-driven acting tests (tests/test_latent_policy.py, tests/test_gpu_latent_policy.py): the two
networks tests/test_gpu_policy_noise.py runs on the acting kernel, with the same parameter and normaliser construction, the
float64 restatement of the decoder, and the small rodent setup of the unroll tests."""
import numpy as np
import torch

from oracle import ppo_numpy as O
from vnl_brax_imitation_amd.ppo_imitation import ppo_networks, running_statistics

NETS = {  # traj, obs, act, latent, encoder, decoder
    "reference": (795, 232, 30, 64, (256, 128), (128, 256)),
    "small-odd": (45, 19, 5, 6, (40, 24), (24, 40)),  # act and latent are no multiples of 4
}
ROWS = 48
SEED, STEP, OFFSET = 0x123456789ABCDEF, 5, 1000  # (the seed's high word and a non-zero env offset reach the kernel)


class Net:
    """one network of NETS on the host: flat parameters, normaliser, 48 rows of inputs (float32 CPU tensors)"""

    def __init__(self, name):
        self.name = name
        self.traj_size, self.obs_size, self.act, self.latent, self.enc, self.dec = NETS[name]
        self.nets = n = ppo_networks.make_intention_ppo_networks(
            self.traj_size, self.obs_size, self.act, preprocess_observations_fn=running_statistics.normalize,
            intention_latent_size=self.latent, encoder_layer_sizes=self.enc, decoder_layer_sizes=self.dec)
        g = torch.Generator().manual_seed(1)
        flat = n.policy_network.init(g)
        flat += 0.05 * torch.randn(flat.shape, generator=g)
        self.norm = running_statistics.update(running_statistics.init_state(self.obs_size),
                                              torch.randn((64, self.obs_size), generator=g) * 2 + 0.3)
        self.flat = flat
        self.traj = torch.randn((ROWS, self.traj_size), generator=g) * 0.2
        self.obs = torch.randn((ROWS, self.obs_size), generator=g)
        # (drawn after the inputs of the acting kernel's test, so that those stay what they are there)
        self.z = torch.randn((ROWS, self.latent), generator=g)
        self.eps_action = torch.randn((ROWS, self.act), generator=g)
        self.rand_action = torch.rand((self.act,), generator=g) * 2 - 1

    def decoder_f64(self, z, obs):
        """float64 logits of the decoder on [z | (obs - mean) / std]: [Dense -> ReLU -> LayerNorm] x (n-1), last Dense linear"""
        P = {k: v.double().numpy() for k, v in self.nets.policy_network.layout.views(self.flat).items()}
        x = np.concatenate([np.asarray(z, dtype=np.float64),
                            (np.asarray(obs, dtype=np.float64) - self.norm.mean.double().numpy()) / self.norm.std.double().numpy()], -1)
        n = len(self.dec) + 1
        for i in range(n):
            x = x @ P[f"decoder/hidden_{i}/kernel"] + P[f"decoder/hidden_{i}/bias"]
            if i != n - 1:
                x = O.layer_norm(np.maximum(x, 0.0), P[f"decoder/LayerNorm_{i}/scale"], P[f"decoder/LayerNorm_{i}/bias"])
        return x

    @staticmethod
    def scale_f64(logits):
        """scale = softplus(s) + 1e-3 of float64 logits [loc | s]"""
        s = np.split(np.asarray(logits, dtype=np.float64), 2, axis=-1)[1]
        return O.softplus(s) + 1e-3


def rodent_setup(B, device, episode_length=4, backend="auto", latent="prior", seed=9, **kw):
    """AutoReset(Episode(RodentTracking)) with episodes of `episode_length` steps, a small intention network and its decoder
    policy -> (env, policy, state, nets, params)"""
    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper

    dev = torch.device(device)
    base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1))
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    policy = ppo_networks.make_decoder_inference_fn(nets)((norm, flat), latent=latent, backend=backend, seed=seed, **kw)
    return env, policy, env.reset(torch.Generator().manual_seed(5)), nets, (norm, flat)


def state_leaves(s):
    return [s.obs, s.done, s.reward] + [s.info[k] for k in ("steps", "truncation", "traj", "cur_frame", "sub_clip_frame")] + \
        [s.pipeline_state.raw(n) for n in s.pipeline_state._FIELDS]
