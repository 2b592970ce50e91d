"""PPO networks with the intention policy: counterpart of reference ppo_imitation/ppo_networks.py:27-124.

`make_intention_ppo_networks(traj_size, observation_size, action_size, preprocess_observations_fn=...)`
keeps the reference's factory signature (it is what ppo.train calls through `network_factory`,
reference ppo_imitation/train.py:225-230).  Parameters are flat float32 buffers (see
intention_policy_network.py); "params" tuples are (normalizer_params, flat_policy_params) exactly
like the reference's `(normalizer_params, params.policy)` (train.py:299-301).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Callable, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import distribution, philox, running_statistics
from . import intention_policy_network as ipn


def identity_observation_preprocessor(obs, params):
    return obs


@dataclasses.dataclass
class FeedForwardNetwork:
    init: Callable[[torch.Generator], torch.Tensor]
    apply: Callable[..., Any]
    layout: ipn.ParamLayout


class ValueMLP:
    """brax.training.networks.make_value_network [UPSTREAM]: MLP obs -> hidden... -> 1, swish, lecun_uniform,
    output squeezed (used at ppo_networks.py:114-118)."""

    def __init__(self, obs_size: int, hidden: Sequence[int]):
        self.sizes = list(hidden) + [1]
        L = ipn.ParamLayout()
        fan = obs_size
        for i, h in enumerate(self.sizes):
            L.add(f"hidden_{i}/kernel", (fan, h)), L.add(f"hidden_{i}/bias", (h,))
            fan = h
        self.layout = L

    def init(self, gen: torch.Generator) -> torch.Tensor:
        flat = torch.zeros(self.layout.size, dtype=torch.float32)
        for name, (off, shape) in self.layout.entries.items():
            if name.endswith("/kernel"):
                ipn.lecun_uniform_(self.layout.view(flat, name), shape[0], gen)
        return flat

    def apply(self, flat: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
        lead = obs.shape[:-1]
        x = obs.reshape(-1, obs.shape[-1])
        n = len(self.sizes)
        for i in range(n):  # addmm: bias fused into the GEMM epilogue
            x = torch.addmm(self.layout.view(flat, f"hidden_{i}/bias"), x, self.layout.view(flat, f"hidden_{i}/kernel"))
            if i != n - 1:
                x = F.silu(x)
        return x.reshape(*lead, -1).squeeze(-1)


@dataclasses.dataclass
class PPOImitationNetworks:
    policy_network: FeedForwardNetwork
    value_network: FeedForwardNetwork
    parametric_action_distribution: distribution.NormalTanhDistribution
    policy_module: ipn.IntentionNetwork = None
    value_module: ValueMLP = None
    normalizes: bool = False  # preprocess_observations_fn is running_statistics.normalize
    hip_ok: bool = False      # the fused HIP inference kernel computes the same function


def make_intention_ppo_networks(
    traj_size: int,
    observation_size: int,
    action_size: int,
    preprocess_observations_fn=identity_observation_preprocessor,
    intention_latent_size: int = 64,
    encoder_layer_sizes: Sequence[int] = (1024,) * 2,
    decoder_layer_sizes: Sequence[int] = (1024,) * 2,
    value_hidden_layer_sizes: Sequence[int] = (1024,) * 2,
) -> PPOImitationNetworks:
    """ppo_networks.py:91-124."""
    dist = distribution.NormalTanhDistribution(event_size=action_size)
    pol = ipn.make_intention_policy(dist.param_size, latent_size=intention_latent_size, traj_size=traj_size,
                                    obs_size=observation_size, encoder_layer_sizes=encoder_layer_sizes,
                                    decoder_layer_sizes=decoder_layer_sizes)
    val = ValueMLP(observation_size, value_hidden_layer_sizes)

    def policy_apply(processor_params, policy_params, traj, obs, eps_latent):
        obs = preprocess_observations_fn(obs, processor_params)  # traj is NOT normalised (ipn:125-127)
        return pol.apply(policy_params, traj, obs, eps_latent)

    def value_apply(processor_params, value_params, obs):
        return val.apply(value_params, preprocess_observations_fn(obs, processor_params))

    return PPOImitationNetworks(
        policy_network=FeedForwardNetwork(init=pol.init, apply=policy_apply, layout=pol.layout),
        value_network=FeedForwardNetwork(init=val.init, apply=value_apply, layout=val.layout),
        parametric_action_distribution=dist,
        policy_module=pol,
        value_module=val,
        normalizes=preprocess_observations_fn is running_statistics.normalize,
        hip_ok=preprocess_observations_fn in (running_statistics.normalize, identity_observation_preprocessor),
    )


def _randn(shape, key: Optional[torch.Generator], device) -> torch.Tensor:
    if key is not None and key.device.type != torch.device(device).type:
        return torch.randn(shape, generator=key, dtype=torch.float32).to(device)
    return torch.randn(shape, generator=key, dtype=torch.float32, device=device)


def _rand_action(n: int, key: Optional[torch.Generator], device) -> torch.Tensor:
    """One U(-1, 1) pre-tanh action shared by the whole batch (ppo_networks.py:67-69), drawn on the device the
    generator lives on (a host draw + copy would synchronise the rollout loop every step)."""
    if key is not None and key.device.type != torch.device(device).type:
        return torch.empty((n,), dtype=torch.float32).uniform_(-1.0, 1.0, generator=key).to(device)
    return torch.empty((n,), dtype=torch.float32, device=device).uniform_(-1.0, 1.0, generator=key)  # one launch, not three


_LOGGED = ("log_prob", "rand_log_prob", "raw_action", "logits")  # the policy extras of a stochastic call, in this order


class _DeviceNoisePolicy:
    """make_inference_fn(...)(params, noise="device"): the acting policy with counter-based noise (philox.py).

    `policy(traj, obs)` is the usual call.  An unroll that steps the counter itself passes `step_offset=t, advance=False`
    (and adds T to `policy.counter` once, afterwards) and may hand in `out`: preallocated contiguous tensors for "action" and
    the policy extras, which the call then writes instead of allocating its own."""

    noise = "device"

    def __init__(self, nets: PPOImitationNetworks, hip_cache: dict, params, deterministic: bool, use_hip: bool, seed: int,
                 env_offset: int, counter: Optional[torch.Tensor]):
        self.nets, self.hip_cache, self.params = nets, hip_cache, params
        self.deterministic, self.use_hip = bool(deterministic), use_hip
        self.seed, self.env_offset = int(seed), int(env_offset)
        if self.env_offset < 0:
            raise ValueError("env_offset must not be negative")
        dev = params[1].device
        if counter is None:
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
        if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != dev:
            raise ValueError("counter must be an int64 tensor of one element on the parameters' device")
        self.counter = counter

    @torch.no_grad()
    def __call__(self, trajectories: torch.Tensor, observations: torch.Tensor, key_sample=None, *, step_offset: int = 0,
                 advance: bool = True, out: Optional[dict] = None) -> Tuple[torch.Tensor, dict]:
        if observations.dim() != 2:
            raise ValueError("noise='device' keys the draws by the row: observations must be (batch, obs_size)")
        res = (self._hip if self.use_hip else self._torch)(trajectories, observations, int(step_offset), out)
        if advance:
            self.counter.add_(1)
        return res

    def _hip(self, trajectories, observations, step_offset, out):
        from .hip_policy import HipIntentionPolicy

        nets, dist = self.nets, self.nets.parametric_action_distribution
        normalizer_params, policy_params = self.params
        dev, B = observations.device, observations.shape[0]
        k = (dev, B)
        if k not in self.hip_cache:
            self.hip_cache[k] = HipIntentionPolicy(nets.policy_module, dist.event_size, B, dev)
        mean = std = None
        if nets.normalizes and normalizer_params is not None:
            mean, std = normalizer_params.mean, normalizer_params.std
        action, extras = self.hip_cache[k].forward_noise(
            policy_params.detach(), mean, std, trajectories, observations, self.counter, step_offset=step_offset,
            seed=self.seed, env_offset=self.env_offset, deterministic=self.deterministic, out=out)
        if self.deterministic:
            return action, {}
        return action, {k2: extras[k2] for k2 in _LOGGED}

    def _torch(self, trajectories, observations, step_offset, out):
        nets, dist = self.nets, self.nets.parametric_action_distribution
        normalizer_params, policy_params = self.params
        dev, B = observations.device, observations.shape[0]
        if self.env_offset + B >= philox.SHARED_ENV:
            raise ValueError("env_offset + batch must stay below 2^32 - 1")
        step = self.counter.to(dev) + step_offset
        env = self.env_offset + torch.arange(B, dtype=torch.int64, device=dev)
        eps_latent = philox.normal(self.seed, step, env, nets.policy_module.latents, philox.STREAM_LATENT)
        logits, _, _ = nets.policy_network.apply(normalizer_params, policy_params, trajectories, observations, eps_latent)
        if self.deterministic:
            res = {"action": dist.mode(logits)}
        else:
            eps_action = philox.normal(self.seed, step, env, dist.event_size, philox.STREAM_ACTION)
            raw_actions = dist.sample_no_postprocessing(logits, eps_action)
            random_actions = philox.shared_uniform(self.seed, step, dist.event_size, device=dev)
            res = {"action": dist.postprocess(raw_actions), "log_prob": dist.log_prob(logits, raw_actions),
                   "rand_log_prob": dist.log_prob(logits, random_actions.expand_as(raw_actions)),
                   "raw_action": raw_actions, "logits": logits}
        if out is not None:
            res = {k2: out[k2].copy_(v) for k2, v in res.items()}
        return res["action"], {k2: res[k2] for k2 in _LOGGED if k2 in res}


def make_inference_fn(ppo_networks: PPOImitationNetworks):
    """ppo_networks.py:35-87.  `key_sample` is a torch.Generator (or None for the global one);
    the JAX threefry stream is not reproduced, the sampling structure is:
      eps_latent ~ N(0,I) for the encoder's reparameterisation (ipn:96-101),
      eps_action ~ N(0,I) for sample_no_postprocessing (ppo_networks.py:60-62),
      one (action_size,) U(-1,1) draw broadcast over the batch for rand_log_prob (:67-73)."""

    hip_cache = {}

    def make_policy(params, deterministic: bool = False, backend: str = "auto", noise: str = "generator", seed: int = 0,
                    env_offset: int = 0, counter: Optional[torch.Tensor] = None):
        """backend: "hip" = fused MFMA inference kernel (vnl_policy_forward), "torch" = hipBLASLt ops,
        "auto" = hip on a HIP device when the observation preprocessor is the running-statistics
        normaliser or the identity.

        noise: "generator" = the three draws come from `key_sample`, batch-shaped (an env's noise depends on the batch size
        and on its row); "device" = counter-based streams keyed by (seed, step, env_offset + row) (philox.py): the HIP kernel
        draws its own noise (vnl_policy_forward_noise), the torch backend draws from the restatement, and `key_sample` is
        ignored.  The returned policy then holds `policy.counter`, an int64 [1] tensor beside the parameters: a call draws
        at step `counter`, then advances it by one (`counter`: continue an existing one instead of starting at 0;
        checkpoint it to resume a run).  `env_offset`: global index of row 0 (rank * num_envs of a sharded run)."""
        normalizer_params, policy_params = params
        dist = ppo_networks.parametric_action_distribution
        latent = ppo_networks.policy_module.latents
        use_hip = backend == "hip" or (backend == "auto" and policy_params.is_cuda and ppo_networks.hip_ok)
        if noise not in ("generator", "device"):
            raise ValueError(f"noise must be 'generator' or 'device', got {noise!r}")
        if noise == "device":
            return _DeviceNoisePolicy(ppo_networks, hip_cache, params, deterministic, use_hip, seed, env_offset, counter)

        @torch.no_grad()
        def policy_hip(trajectories, observations, key_sample=None):
            from .hip_policy import HipIntentionPolicy

            dev, B = observations.device, observations.shape[0]
            k = (dev, B)
            if k not in hip_cache:
                hip_cache[k] = HipIntentionPolicy(ppo_networks.policy_module, dist.event_size, B, dev)
            eps_latent = _randn((B, latent), key_sample, dev)
            eps_action = None if deterministic else _randn((B, dist.event_size), key_sample, dev)
            mean = std = None
            if ppo_networks.normalizes and normalizer_params is not None:
                mean, std = normalizer_params.mean, normalizer_params.std
            random_actions = None if deterministic else _rand_action(dist.event_size, key_sample, dev)
            action, extras = hip_cache[k].forward(policy_params.detach(), mean, std, trajectories, observations,
                                                  eps_latent, eps_action, deterministic, rand_action=random_actions)
            if deterministic:
                return action, {}
            return action, {k2: extras[k2] for k2 in ("log_prob", "rand_log_prob", "raw_action", "logits")}

        if use_hip:
            return policy_hip

        @torch.no_grad()
        def policy(trajectories: torch.Tensor, observations: torch.Tensor,
                   key_sample: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, dict]:
            dev = observations.device
            lead = observations.shape[:-1]
            eps_latent = _randn((*lead, latent), key_sample, dev)
            logits, _, _ = ppo_networks.policy_network.apply(normalizer_params, policy_params, trajectories,
                                                             observations, eps_latent)
            if deterministic:
                return dist.mode(logits), {}
            eps_action = _randn((*lead, dist.event_size), key_sample, dev)
            raw_actions = dist.sample_no_postprocessing(logits, eps_action)
            log_prob = dist.log_prob(logits, raw_actions)
            random_actions = _rand_action(dist.event_size, key_sample, dev)
            rand_log_prob = dist.log_prob(logits, random_actions.expand_as(raw_actions))
            return dist.postprocess(raw_actions), {
                "log_prob": log_prob,
                "rand_log_prob": rand_log_prob,
                "raw_action": raw_actions,
                "logits": logits,
            }

        return policy

    return make_policy


class _DecoderPolicy:
    """make_decoder_inference_fn(...)(params, latent=...): latent-driven acting, the motor decoder alone as a policy.

    Duck-types `_DeviceNoisePolicy` (noise == "device", `.counter`, `.deterministic`, the same call), so the unrolls, the
    graph captures and the evaluator of acting.py take it as they are.  `trajectories` is read only by a callable latent."""

    noise = "device"

    def __init__(self, nets: PPOImitationNetworks, hip_cache: dict, params, latent, deterministic: bool, use_hip: bool,
                 seed: int, env_offset: int, counter: Optional[torch.Tensor], latent_out: Optional[torch.Tensor]):
        self.nets, self.hip_cache, self.params = nets, hip_cache, params
        self.deterministic, self.use_hip = bool(deterministic), use_hip
        self.seed, self.env_offset = int(seed), int(env_offset)
        if self.env_offset < 0:
            raise ValueError("env_offset must not be negative")
        nl = nets.policy_module.latents
        if isinstance(latent, str):
            if latent != "prior":
                raise ValueError(f"latent must be 'prior', a float32 [B, {nl}] tensor or a callable (traj, obs) -> latent, got {latent!r}")
        elif isinstance(latent, torch.Tensor):
            self._check_latent(latent, None, "latent")
        elif not callable(latent):
            raise ValueError(f"latent must be 'prior', a float32 [B, {nl}] tensor or a callable (traj, obs) -> latent")
        if latent_out is not None:
            self._check_latent(latent_out, None, "latent_out")
        self.latent, self.latent_out = latent, latent_out
        dev = params[1].device
        if counter is None:
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
        if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != dev:
            raise ValueError("counter must be an int64 tensor of one element on the parameters' device")
        self.counter = counter

    def _check_latent(self, z, B, what):
        nl = self.nets.policy_module.latents
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[1] != nl or (B is not None and z.shape[0] != B):
            raise ValueError(f"{what} must have shape [{'B' if B is None else B}, {nl}], got "
                             f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__}")
        if z.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, got {z.dtype}")

    @torch.no_grad()
    def __call__(self, trajectories: torch.Tensor, observations: torch.Tensor, key_sample=None, *, step_offset: int = 0,
                 advance: bool = True, out: Optional[dict] = None) -> Tuple[torch.Tensor, dict]:
        if observations.dim() != 2:
            raise ValueError("the draws are keyed by the row: observations must be (batch, obs_size)")
        B = observations.shape[0]
        z = None  # the prior draw, made by the backend
        if callable(self.latent):  # a high-level controller of torch ops, in front of the decode launch
            z = self.latent(trajectories, observations)
            self._check_latent(z, B, "the latent callable's result")
        elif isinstance(self.latent, torch.Tensor):  # read live: the caller may rewrite it in place between calls
            z = self.latent
            self._check_latent(z, B, "latent")
        if self.latent_out is not None:
            self._check_latent(self.latent_out, B, "latent_out")
            if z is not None:
                self.latent_out.copy_(z)
        res = (self._hip if self.use_hip else self._torch)(z, observations, int(step_offset), out)
        if advance:
            self.counter.add_(1)
        return res

    def _hip(self, z, observations, step_offset, out):
        from .hip_policy import HipIntentionPolicy

        nets, dist = self.nets, self.nets.parametric_action_distribution
        normalizer_params, policy_params = self.params
        dev, B = observations.device, observations.shape[0]
        k = (dev, B)
        if k not in self.hip_cache:
            self.hip_cache[k] = HipIntentionPolicy(nets.policy_module, dist.event_size, B, dev)
        mean = std = None
        if nets.normalizes and normalizer_params is not None:
            mean, std = normalizer_params.mean, normalizer_params.std
        eps_out = None
        if z is None and self.latent_out is not None:  # the kernel writes the z it draws
            if not self.latent_out.is_contiguous() or self.latent_out.device != dev:
                raise ValueError("latent_out must be contiguous and on the inputs' device")
            eps_out = {"eps_latent": self.latent_out}
        action, extras = self.hip_cache[k].decode_noise(
            policy_params.detach(), mean, std, z, observations, self.counter, step_offset=step_offset, seed=self.seed,
            env_offset=self.env_offset, deterministic=self.deterministic, out=out, eps_out=eps_out)
        if self.deterministic:
            return action, {}
        return action, {k2: extras[k2] for k2 in _LOGGED}

    def _torch(self, z, observations, step_offset, out):
        nets, dist = self.nets, self.nets.parametric_action_distribution
        normalizer_params, policy_params = self.params
        dev, B = observations.device, observations.shape[0]
        if self.env_offset + B >= philox.SHARED_ENV:
            raise ValueError("env_offset + batch must stay below 2^32 - 1")
        step = self.counter.to(dev) + step_offset
        env = self.env_offset + torch.arange(B, dtype=torch.int64, device=dev)
        if z is None:  # the prior of the KL term, on the counters of the acting policy's eps_latent
            z = philox.normal(self.seed, step, env, nets.policy_module.latents, philox.STREAM_LATENT)
            if self.latent_out is not None:
                self.latent_out.copy_(z)
        obs = running_statistics.normalize(observations, normalizer_params) if nets.normalizes else observations
        logits = nets.policy_module.decode(policy_params, torch.cat([z, obs], dim=-1))
        if self.deterministic:
            res = {"action": dist.mode(logits)}
        else:
            eps_action = philox.normal(self.seed, step, env, dist.event_size, philox.STREAM_ACTION)
            raw_actions = dist.sample_no_postprocessing(logits, eps_action)
            random_actions = philox.shared_uniform(self.seed, step, dist.event_size, device=dev)
            res = {"action": dist.postprocess(raw_actions), "log_prob": dist.log_prob(logits, raw_actions),
                   "rand_log_prob": dist.log_prob(logits, random_actions.expand_as(raw_actions)),
                   "raw_action": raw_actions, "logits": logits}
        if out is not None:
            res = {k2: out[k2].copy_(v) for k2, v in res.items()}
        return res["action"], {k2: res[k2] for k2 in _LOGGED if k2 in res}


def make_decoder_inference_fn(ppo_networks: PPOImitationNetworks):
    """Latent-driven acting: the intention network's decoder alone, [z | normalised obs] -> action, as a policy (the
    encoder is not run and its parameters are not read).  Needs the running-statistics normaliser or the identity as the
    observation preprocessor."""
    if not ppo_networks.hip_ok:
        raise ValueError("the decoder policy needs running_statistics.normalize or the identity as the observation preprocessor")
    hip_cache = {}

    def make_decoder_policy(params, latent="prior", deterministic: bool = False, backend: str = "auto", seed: int = 0,
                            env_offset: int = 0, counter: Optional[torch.Tensor] = None,
                            latent_out: Optional[torch.Tensor] = None):
        """latent: "prior" = z ~ N(0, I) drawn per env and step, stream 0 of the counter-based noise (philox.py), keyed by
        (seed, step, env_offset + row); a float32 [B, latent] tensor, read live at every call (rewrite it in place between
        steps, also between replays of a captured graph); or a callable (traj, obs) -> [B, latent] of torch ops, which runs
        in front of the decode launch.  eps_action and the shared random action are streams 1 and 2, as with
        make_inference_fn(...)(params, noise="device"); `counter`, `seed`, `env_offset` and the returned policy's call are
        that policy's.  backend: "hip" = vnl_policy_decode_noise, "torch" = IntentionNetwork.decode on the restated draws,
        "auto" = hip when the parameters live on a HIP device.  latent_out: a float32 [B, latent] tensor that every call
        overwrites with the z it used (in prior mode on the hip backend the kernel writes it)."""
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be 'auto', 'hip' or 'torch', got {backend!r}")
        use_hip = backend == "hip" or (backend == "auto" and params[1].is_cuda and ppo_networks.hip_ok)
        return _DecoderPolicy(ppo_networks, hip_cache, params, latent, deterministic, use_hip, seed, env_offset, counter,
                              latent_out)

    return make_decoder_policy
