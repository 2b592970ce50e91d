"""Fused HIP inference kernel for the intention policy (C-ABI vnl_policy_*, csrc/vnl_policy.hip).

Used by `make_inference_fn` for acting on a HIP device; training (autograd) keeps the torch path,
which computes the same function (tests/test_gpu_policy.py compares the two)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib
from .intention_policy_network import IntentionNetwork


class HipIntentionPolicy:
    def __init__(self, net: IntentionNetwork, action_size: int, max_batch: int, device: torch.device):
        self.lib = _lib.load_library()
        self.net, self.action_size, self.device = net, action_size, torch.device(device)
        spec = _lib.PolicySpec()
        spec.traj_size, spec.obs_size, spec.action_size, spec.latent_size = net.traj_size, net.obs_size, action_size, net.latents
        spec.num_encoder_layers, spec.num_decoder_layers = len(net.encoder_layers), len(net.decoder_layers)
        for i, h in enumerate(net.encoder_layers):
            spec.encoder_layers[i] = h
        for i, h in enumerate(net.decoder_layers):
            spec.decoder_layers[i] = h
        self.h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib, self.lib.vnl_policy_create(C.byref(spec), int(max_batch), idx, C.byref(self.h)))
        n = self.lib.vnl_policy_num_params(self.h)
        if n != net.num_params:
            raise _lib.VnlError(f"parameter layout mismatch: kernel expects {n}, network has {net.num_params}")
        self.max_batch = int(max_batch)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.vnl_policy_destroy(self.h)
        except Exception:
            pass

    @torch.no_grad()
    def forward(self, params: torch.Tensor, obs_mean: Optional[torch.Tensor], obs_std: Optional[torch.Tensor],
                traj: torch.Tensor, obs: torch.Tensor, eps_latent: torch.Tensor, eps_action: Optional[torch.Tensor],
                deterministic: bool = False, rand_action: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, dict]:
        B, na, nl = obs.shape[0], self.action_size, self.net.latents
        f32 = dict(dtype=torch.float32, device=obs.device)
        c = lambda t: t.contiguous()  # noqa: E731
        traj, obs, eps_latent, params = c(traj), c(obs), c(eps_latent), c(params)
        action = torch.empty((B, na), **f32)
        logits = torch.empty((B, 2 * na), **f32)
        lat_mean, lat_logvar = torch.empty((B, nl), **f32), torch.empty((B, nl), **f32)
        raw = torch.empty((B, na), **f32) if not deterministic else None
        lp = torch.empty((B,), **f32) if not deterministic else None
        rlp = torch.empty((B,), **f32) if (rand_action is not None and not deterministic) else None
        if rlp is None:
            rand_action = None
        else:
            rand_action = c(rand_action)
        if not deterministic:
            eps_action = c(eps_action)
        if obs_mean is not None:
            obs_mean, obs_std = c(obs_mean), c(obs_std)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        _lib.check(self.lib, self.lib.vnl_policy_forward(
            self.h, p(params), p(obs_mean), p(obs_std), p(traj), p(obs), p(eps_latent), p(eps_action), B,
            int(deterministic), p(action), p(raw), p(lp), p(logits), p(lat_mean), p(lat_logvar), p(rand_action),
            p(rlp), stream))
        self._hold = (traj, obs, eps_latent, eps_action, params, obs_mean, obs_std, rand_action)
        extras = {} if deterministic else {"log_prob": lp, "raw_action": raw, "logits": logits}
        if rlp is not None:
            extras["rand_log_prob"] = rlp
        return action, {**extras, "latent_mean": lat_mean, "latent_logvar": lat_logvar}

    @torch.no_grad()
    def forward_noise(self, params: torch.Tensor, obs_mean: Optional[torch.Tensor], obs_std: Optional[torch.Tensor],
                      traj: torch.Tensor, obs: torch.Tensor, counter: torch.Tensor, step_offset: int = 0, seed: int = 0,
                      env_offset: int = 0, deterministic: bool = False, rand: bool = True, out: Optional[dict] = None,
                      eps_out: Optional[dict] = None) -> Tuple[torch.Tensor, dict]:
        """vnl_policy_forward_noise: the kernel draws eps_latent, eps_action and the shared random action itself, from
        streams keyed by (seed, *counter + step_offset, env_offset + row).  Nothing is owned here: `counter` is the caller's
        int64 [1] device tensor, which the kernel only reads (advance it after the calls that share it).
        `out`: optional preallocated contiguous float32 tensors "action", "raw_action", "log_prob", "rand_log_prob", "logits"
        (e.g. rows of an unroll's log buffers) written instead of fresh ones; `eps_out`: optional "eps_latent" [B, latent],
        "eps_action" [B, act], "rand_action" [act] that record the draws used.  `rand=False`: no rand_log_prob."""
        B, na, nl = obs.shape[0], self.action_size, self.net.latents
        f32 = dict(dtype=torch.float32, device=obs.device)
        c = lambda t: t.contiguous()  # noqa: E731
        traj, obs, params = c(traj), c(obs), c(params)
        if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != obs.device:
            raise ValueError("counter must be an int64 tensor of one element on the inputs' device")
        out, eps_out = out or {}, eps_out or {}

        def buf(name, shape, wanted=True):
            if not wanted:
                return None
            t = out.get(name)
            if t is None:
                return torch.empty(shape, **f32)
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != obs.device:
                raise ValueError(f"out[{name!r}] must be a contiguous float32 {shape} tensor on the inputs' device")
            return t

        stochastic = not deterministic
        action, logits = buf("action", (B, na)), buf("logits", (B, 2 * na))
        lat_mean, lat_logvar = torch.empty((B, nl), **f32), torch.empty((B, nl), **f32)
        raw, lp = buf("raw_action", (B, na), stochastic), buf("log_prob", (B,), stochastic)
        rlp = buf("rand_log_prob", (B,), stochastic and rand)
        rec = {k: eps_out.get(k) for k in ("eps_latent", "eps_action", "rand_action")}
        for k, shape in (("eps_latent", (B, nl)), ("eps_action", (B, na)), ("rand_action", (na,))):
            t = rec[k]
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"eps_out[{k!r}] must be a contiguous float32 {shape} tensor")
        if obs_mean is not None:
            obs_mean, obs_std = c(obs_mean), c(obs_std)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        nz = _lib.PolicyNoise()
        nz.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        nz.step_base, nz.step_offset, nz.env_offset = p(counter), int(step_offset), int(env_offset)
        nz.eps_latent_out, nz.eps_action_out, nz.rand_action_out = p(rec["eps_latent"]), p(rec["eps_action"]), p(rec["rand_action"])
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        _lib.check(self.lib, self.lib.vnl_policy_forward_noise(
            self.h, p(params), p(obs_mean), p(obs_std), p(traj), p(obs), C.byref(nz), B, int(deterministic), p(action), p(raw),
            p(lp), p(logits), p(lat_mean), p(lat_logvar), p(rlp), stream))
        self._hold = (traj, obs, params, obs_mean, obs_std, counter, rec)
        extras = {} if deterministic else {"log_prob": lp, "raw_action": raw, "logits": logits}
        if rlp is not None:
            extras["rand_log_prob"] = rlp
        return action, {**extras, "latent_mean": lat_mean, "latent_logvar": lat_logvar}

    @torch.no_grad()
    def decode(self, params: torch.Tensor, obs_mean: Optional[torch.Tensor], obs_std: Optional[torch.Tensor],
               latent: torch.Tensor, obs: torch.Tensor, eps_action: Optional[torch.Tensor], deterministic: bool = False,
               rand_action: Optional[torch.Tensor] = None, out: Optional[dict] = None) -> Tuple[torch.Tensor, dict]:
        """vnl_policy_decode: the decoder alone on a caller-supplied latent [B, latent] -- the arithmetic of `forward` from
        the decoder input [z | normalised obs] on.  `out` as in `forward_noise`."""
        B, na, nl = obs.shape[0], self.action_size, self.net.latents
        c = lambda t: t.contiguous()  # noqa: E731
        if latent is None:
            raise ValueError("decode needs a latent; decode_noise(latent=None) draws it from the prior")
        if tuple(latent.shape) != (B, nl) or latent.dtype != torch.float32 or latent.device != obs.device:
            raise ValueError(f"latent must be a float32 {(B, nl)} tensor on the inputs' device")
        latent, obs, params = c(latent), c(obs), c(params)
        stochastic = not deterministic
        buf = self._out_buffers(out, obs.device)
        action, logits = buf("action", (B, na)), buf("logits", (B, 2 * na))
        raw, lp = buf("raw_action", (B, na), stochastic), buf("log_prob", (B,), stochastic)
        rlp = buf("rand_log_prob", (B,), stochastic and rand_action is not None)
        rand_action = c(rand_action) if rlp is not None else None
        eps_action = c(eps_action) if stochastic else None
        if obs_mean is not None:
            obs_mean, obs_std = c(obs_mean), c(obs_std)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        _lib.check(self.lib, self.lib.vnl_policy_decode(
            self.h, p(params), p(obs_mean), p(obs_std), p(latent), p(obs), p(eps_action), B, int(deterministic), p(action),
            p(raw), p(lp), p(logits), p(rand_action), p(rlp), stream))
        self._hold = (latent, obs, eps_action, params, obs_mean, obs_std, rand_action)
        extras = {} if deterministic else {"log_prob": lp, "raw_action": raw}
        if rlp is not None:
            extras["rand_log_prob"] = rlp
        return action, {**extras, "logits": logits}

    @torch.no_grad()
    def decode_noise(self, params: torch.Tensor, obs_mean: Optional[torch.Tensor], obs_std: Optional[torch.Tensor],
                     latent: Optional[torch.Tensor], obs: torch.Tensor, counter: torch.Tensor, step_offset: int = 0,
                     seed: int = 0, env_offset: int = 0, deterministic: bool = False, rand: bool = True,
                     out: Optional[dict] = None, eps_out: Optional[dict] = None) -> Tuple[torch.Tensor, dict]:
        """vnl_policy_decode_noise: the decoder alone, eps_action and the shared random action drawn by the kernel from
        streams 1 and 2 keyed by (seed, *counter + step_offset, env_offset + row), as `forward_noise` draws them.
        `latent=None` selects the prior draw: z is stream 0's normal draw, recorded in eps_out["eps_latent"] when given (with
        a latent given, stream 0 is not drawn and that record is left alone).  `counter`, `out`, `eps_out`, `rand` as in
        `forward_noise`."""
        B, na, nl = obs.shape[0], self.action_size, self.net.latents
        c = lambda t: t.contiguous()  # noqa: E731
        obs, params = c(obs), c(params)
        if latent is not None:
            if tuple(latent.shape) != (B, nl) or latent.dtype != torch.float32 or latent.device != obs.device:
                raise ValueError(f"latent must be a float32 {(B, nl)} tensor on the inputs' device")
            latent = c(latent)
        if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != obs.device:
            raise ValueError("counter must be an int64 tensor of one element on the inputs' device")
        eps_out = eps_out or {}
        stochastic = not deterministic
        buf = self._out_buffers(out, obs.device)
        action, logits = buf("action", (B, na)), buf("logits", (B, 2 * na))
        raw, lp = buf("raw_action", (B, na), stochastic), buf("log_prob", (B,), stochastic)
        rlp = buf("rand_log_prob", (B,), stochastic and rand)
        rec = {k: eps_out.get(k) for k in ("eps_latent", "eps_action", "rand_action")}
        for k, shape in (("eps_latent", (B, nl)), ("eps_action", (B, na)), ("rand_action", (na,))):
            t = rec[k]
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"eps_out[{k!r}] must be a contiguous float32 {shape} tensor")
        if obs_mean is not None:
            obs_mean, obs_std = c(obs_mean), c(obs_std)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        nz = _lib.PolicyNoise()
        nz.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        nz.step_base, nz.step_offset, nz.env_offset = p(counter), int(step_offset), int(env_offset)
        nz.eps_latent_out, nz.eps_action_out, nz.rand_action_out = p(rec["eps_latent"]), p(rec["eps_action"]), p(rec["rand_action"])
        stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        _lib.check(self.lib, self.lib.vnl_policy_decode_noise(
            self.h, p(params), p(obs_mean), p(obs_std), p(latent), p(obs), C.byref(nz), B, int(deterministic), p(action), p(raw),
            p(lp), p(logits), p(rlp), stream))
        self._hold = (latent, obs, params, obs_mean, obs_std, counter, rec)
        extras = {} if deterministic else {"log_prob": lp, "raw_action": raw}
        if rlp is not None:
            extras["rand_log_prob"] = rlp
        return action, {**extras, "logits": logits}

    @staticmethod
    def _out_buffers(out: Optional[dict], device):
        """buf(name, shape, wanted=True): out[name] when given (checked), else a fresh float32 tensor; None if not wanted"""
        out = out or {}

        def buf(name, shape, wanted=True):
            if not wanted:
                return None
            t = out.get(name)
            if t is None:
                return torch.empty(shape, dtype=torch.float32, device=device)
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
                raise ValueError(f"out[{name!r}] must be a contiguous float32 {shape} tensor on the inputs' device")
            return t

        return buf
