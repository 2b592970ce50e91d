"""Training wrappers with brax.envs.wrappers.training semantics [UPSTREAM], as applied
by the reference at ppo_imitation/train.py:204-214 (wrap_for_training) and
ppo_imitation/acting.py:109 (EvalWrapper).  The Vmap wrapper is not needed: the
envs are natively batched.

State buffers are updated in place by the kernels, so the wrappers keep their own
copies where brax relies on immutability (first_pipeline_state / first_obs).
"""
from __future__ import annotations

import dataclasses
from typing import Dict

import torch

from .base import Env, State


class Wrapper(Env):
    def __init__(self, env: Env):
        self.env = env

    def __getattr__(self, name):
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self) -> Env:
        return self.env.unwrapped

    @property
    def observation_size(self) -> int:
        return self.env.observation_size

    @property
    def action_size(self) -> int:
        return self.env.action_size

    def reset(self, rng=None, **kw) -> State:
        return self.env.reset(rng, **kw)

    def step(self, state: State, action: torch.Tensor) -> State:
        return self.env.step(state, action)


class EpisodeWrapper(Wrapper):
    """Maintains episode step count and sets done at episode end (brax EpisodeWrapper)."""

    def __init__(self, env: Env, episode_length: int, action_repeat: int):
        super().__init__(env)
        self.episode_length = int(episode_length)
        self.action_repeat = int(action_repeat)

    def reset(self, rng=None, **kw) -> State:
        state = self.env.reset(rng, **kw)
        state.info["steps"] = torch.zeros_like(state.done)
        state.info["truncation"] = torch.zeros_like(state.done)
        return state

    def step(self, state: State, action: torch.Tensor) -> State:
        if self.action_repeat == 1:
            state = self.env.step(state, action)
        else:
            total = torch.zeros_like(state.reward)
            for _ in range(self.action_repeat):
                state = self.env.step(state, action)
                total += state.reward
            state.reward.copy_(total)
        steps = state.info["steps"]
        steps += self.action_repeat
        over = steps >= self.episode_length
        state.info["truncation"].copy_(torch.where(over, 1.0 - state.done, torch.zeros_like(state.done)))
        state.done.copy_(torch.where(over, torch.ones_like(state.done), state.done))
        return state


AUTO_RESET_MODES = ("first_state", "fresh")


class AutoResetWrapper(Wrapper):
    """Automatically resets done envs.

    mode="first_state" (default; brax AutoResetWrapper): to the cached first state.  As in brax, only `pipeline_state` and
    `obs` are restored; `info` (cur_frame, sub_clip_frame, traj) is NOT unless
    reset_info_on_autoreset=True.

    mode="fresh": to a NEW episode -- start frame, clip and reset noise drawn on the device per env and episode
    (`env.reset_done`, vnl_env_reset_done), keyed by (seed, info["reset_step"], env_offset + env index): no first state is
    cached, and the whole of `info` follows the reset.  `info["reset_step"]` is an int64[1] device counter that advances by
    one per step.  reward / done / metrics of the terminal step are kept, as under brax's auto-reset.
    With `start_priority` (envs/start_priority.py StartPriority; mode="fresh" only) start frame and clip are drawn from its
    table and the episodes that end are counted into its counters -- not those an EpisodeWrapper below truncated.  The
    caller runs its `update()` (between unrolls).
    An env with domain ranges (`with_domain_ranges`, `with_body_domain_ranges`; mode="fresh" only has a use for them) gets a new physical domain with
    every fresh reset -- the reset kernel reads the ranges from the env, no argument here -- and `reset` draws the domain of
    every env's FIRST episode (`redraw_domain(initial=True)` at this wrapper's seed, the counter's value and env_offset).
    """

    def __init__(self, env: Env, reset_info_on_autoreset: bool = False, mode: str = "first_state", seed: int = 0,
                 env_offset: int = 0, start_priority=None):
        super().__init__(env)
        if mode not in AUTO_RESET_MODES:
            raise ValueError(f"unknown auto-reset mode {mode!r}: expected one of {AUTO_RESET_MODES}")
        if mode == "fresh" and reset_info_on_autoreset:
            raise ValueError("reset_info_on_autoreset has no meaning with mode='fresh': a fresh reset rewrites the info")
        if mode == "fresh" and not hasattr(env.unwrapped, "reset_done"):
            raise ValueError(f"{type(env.unwrapped).__name__} has no reset_done: mode='fresh' needs a tracking env of this library")
        if start_priority is not None and mode != "fresh":
            raise ValueError("start_priority needs mode='fresh': the cached first state has one start frame")
        self.reset_info, self.start_priority = reset_info_on_autoreset, start_priority
        self.mode, self.seed, self.env_offset = mode, int(seed), int(env_offset)
        self.before_reset = None  # EvalWrapper's scoring, for the length of its step: sees a finished episode before the fresh reset

    def reset(self, rng=None, *, reset_step=None, **kw) -> State:
        """`reset_step` (mode="fresh"): the value the counter starts from, an int or int64 [1] tensor -- a resumed run's;
        default 0."""
        if self.mode == "fresh":
            base = self.env.unwrapped
            counter = torch.zeros(1, dtype=torch.int64, device=base.device)
            if reset_step is not None:
                counter.copy_(torch.as_tensor(reset_step, dtype=torch.int64).reshape(1))
            if (getattr(base, "domain_ranges", None) is not None or
                    getattr(base, "body_domain_ranges", None) is not None):  # the first episodes are randomised too: before their reset
                base.redraw_domain(seed=self.seed, step_base=counter, env_offset=self.env_offset, initial=True)
            state = self.env.reset(rng, **kw)
            state.info["reset_step"] = counter
            return state
        if reset_step is not None:
            raise ValueError("reset_step has no meaning without mode='fresh'")
        state = self.env.reset(rng, **kw)
        state.info["first_pipeline_state"] = state.pipeline_state.clone()
        state.info["first_obs"] = state.obs.clone()
        if self.reset_info:
            state.info["first_info"] = {k: state.info[k].clone() for k in ("cur_frame", "sub_clip_frame", "traj")}
        return state

    def priority_args(self, state: State) -> dict:
        """the `priority` / `truncation` arguments of `reset_done` (none without a priority object)"""
        if self.start_priority is None:
            return {}
        return {"priority": self.start_priority, "truncation": state.info.get("truncation")}

    def step(self, state: State, action: torch.Tensor) -> State:
        if "steps" in state.info:
            steps = state.info["steps"]
            steps.copy_(torch.where(state.done.bool(), torch.zeros_like(steps), steps))
        state.done.zero_()
        state = self.env.step(state, action)
        if self.mode == "fresh":
            counter = state.info["reset_step"]
            if self.before_reset is not None:
                self.before_reset(state)
            self.env.unwrapped.reset_done(state, state.done, seed=self.seed, step_base=counter, env_offset=self.env_offset,
                                          **self.priority_args(state))
            counter.add_(1)
            return state
        done = state.done.bool()
        state.pipeline_state.copy_(state.info["first_pipeline_state"], mask=done)
        state.obs.copy_(torch.where(done[:, None], state.info["first_obs"], state.obs))
        if self.reset_info:
            for k, v in state.info["first_info"].items():
                cur = state.info[k]
                cur.copy_(torch.where(done[:, None] if cur.dim() == 2 else done, v, cur))
        return state


@dataclasses.dataclass
class EvalMetrics:
    """brax.envs.wrappers.training.EvalMetrics."""

    episode_metrics: Dict[str, torch.Tensor]
    active_episodes: torch.Tensor
    episode_steps: torch.Tensor


class EvalWrapper(Wrapper):
    """Accumulates per-episode metrics of the first episode of every env (brax EvalWrapper): info["eval_metrics"].

    Beside it, the scored episodes of include/vnl.h vnl_eval_desc in torch ops (the restatement the device's records are
    compared with, bit for bit): each env scores its first `episodes_per_env` episodes.  info["eval_run"] (B, 8) float32 are
    the running sums of the seven metrics and the reward, info["eval_count"] (B,) int32 the episodes completed,
    info["eval_records"] (B, K, 12) float32 one row per completed episode: start frame, clip, steps, truncation, the eight
    sums (`_lib.EVAL_COLUMNS`).  A tracking env of this library sums the seven columns of its metrics buffer, as the kernel
    does, whichever of them its `State.metrics` names (`columns`: name -> column of the sums).  Rows at or beyond the count
    stay zero.  Under AutoResetWrapper(mode="fresh") the step is
    scored before the fresh reset rewrites the frame counters."""

    def __init__(self, env: Env, episodes_per_env: int = 1):
        super().__init__(env)
        if int(episodes_per_env) < 1:
            raise ValueError("episodes_per_env must be at least 1")
        self.episodes_per_env = int(episodes_per_env)
        self.after_score = None  # a RolloutRecorder's row, for the length of an unroll: after the scoring, before a fresh reset

    def _score_step(self, state: State) -> None:
        self.score(state)
        if self.after_score is not None:
            self.after_score(state)

    def reset(self, rng=None, **kw) -> State:
        state = self.env.reset(rng, **kw)
        names = list(state.metrics.keys()) + ["reward"]
        state.info["eval_metrics"] = EvalMetrics(
            episode_metrics={k: torch.zeros_like(state.reward) for k in names},
            active_episodes=torch.ones_like(state.reward),
            episode_steps=torch.zeros_like(state.reward),
        )
        B, dev = state.reward.shape[0], state.reward.device
        buf = self._metrics_buffer(state)
        if buf is not None:  # (State.metrics are column views of it)
            self.columns = {k: v.storage_offset() - buf.storage_offset() for k, v in state.metrics.items()}
        else:
            self.columns = {k: i for i, k in enumerate(state.metrics)}
        n = 1 + (buf.shape[1] if buf is not None else len(state.metrics))
        self.columns["reward"] = n - 1
        state.info["eval_run"] = torch.zeros((B, n), dtype=torch.float32, device=dev)
        state.info["eval_count"] = torch.zeros(B, dtype=torch.int32, device=dev)
        state.info["eval_records"] = torch.zeros((B, self.episodes_per_env, 4 + n), dtype=torch.float32, device=dev)
        return state

    @staticmethod
    def _metrics_buffer(state: State):
        raw = state.info.get("_raw")
        return raw["metrics"] if isinstance(raw, dict) and "metrics" in raw else None

    def _fresh(self):
        ar = self.env
        return ar if isinstance(ar, AutoResetWrapper) and ar.mode == "fresh" else None

    def score(self, state: State) -> None:
        """vnl_rollout_eval in torch ops, on the state as the wrappers below have left it."""
        info, K = state.info, self.episodes_per_env
        run, count, rec = info["eval_run"], info["eval_count"], info["eval_records"]
        live = count < K
        buf = self._metrics_buffer(state)
        x = torch.cat([buf if buf is not None else torch.stack(list(state.metrics.values()), dim=1), state.reward[:, None]],
                      dim=1).to(torch.float32)
        r = run + x
        done = (state.done != 0) & live
        if all(k in info for k in ("cur_frame", "sub_clip_frame", "clip_id")):
            start, clip = (info["cur_frame"] - info["sub_clip_frame"]).to(torch.float32), info["clip_id"].to(torch.float32)
        else:
            start = clip = torch.full_like(state.reward, -1.0, dtype=torch.float32)
        trunc = info["truncation"] if "truncation" in info else torch.zeros_like(state.reward)
        row = torch.cat([torch.stack([start, clip, info["steps"].to(torch.float32), trunc.to(torch.float32)], dim=1), r], dim=1)
        env = torch.arange(rec.shape[0], device=rec.device)
        slot = count.clamp(max=K - 1).long()
        rec[env, slot] = torch.where(done[:, None], row, rec[env, slot])
        run.copy_(torch.where(live[:, None], torch.where(done[:, None], torch.zeros_like(r), r), run))
        count += done.to(torch.int32)

    def sync_eval_metrics(self, state: State) -> None:
        """info["eval_metrics"] from the records (the fused routes keep only those): the first episode of every env, or what
        has run of it."""
        em: EvalMetrics = state.info["eval_metrics"]
        run, rec = state.info["eval_run"], state.info["eval_records"]
        fin = state.info["eval_count"] >= 1
        for name, k in self.columns.items():
            em.episode_metrics[name].copy_(torch.where(fin, rec[:, 0, 4 + k], run[:, k]))
        em.episode_steps.copy_(torch.where(fin, rec[:, 0, 2], state.info["steps"]))
        em.active_episodes.copy_((~fin).to(em.active_episodes.dtype))

    def step(self, state: State, action: torch.Tensor) -> State:
        em: EvalMetrics = state.info["eval_metrics"]
        ar = self._fresh()
        if ar is not None:
            ar.before_reset = self._score_step
        try:
            nstate = self.env.step(state, action)
        finally:
            if ar is not None:
                ar.before_reset = None
        if ar is None:
            self._score_step(nstate)
        active = em.active_episodes
        em.episode_steps.copy_(torch.where(active.bool(), nstate.info["steps"], em.episode_steps))
        for k, acc in em.episode_metrics.items():
            acc += (nstate.reward if k == "reward" else nstate.metrics[k]) * active
        active *= 1.0 - nstate.done
        return nstate


def wrap(env: Env, episode_length: int = 1000, action_repeat: int = 1, randomization_fn=None,
         reset_info_on_autoreset: bool = False, auto_reset: str = "first_state", auto_reset_seed: int = 0,
         env_offset: int = 0, start_priority=None, domain_ranges=None, domain_shared=(), body_domain_ranges=None,
         body_domain_shared=(), body_inertia_with_mass: bool = False) -> Wrapper:
    """brax.envs.training.wrap minus the VmapWrapper (natively batched env).

    `randomization_fn(sys) -> {field: (num_envs, n) values}` (brax's contract once its `rng` is bound; train.py binds
    num_envs and rng): its result goes to `env.with_domain` (cg_friction, act_gain, dof_damping, dof_armature) and, for the
    keys body_mass, body_inertia, body_ipos, to `env.with_body_domain`: a NEW env with per-env model parameters.  An unknown
    key raises.  The caller's env is left as it is.

    `auto_reset`: "first_state" (brax: a done env returns to the cached first state) or "fresh" (a new start frame, clip
    and reset noise per episode, drawn on the device; AutoResetWrapper), with `auto_reset_seed` and `env_offset` (the global
    index of this batch's env 0, for sharded runs) keying the draws.  `start_priority`: with "fresh", a StartPriority
    (envs/start_priority.py) whose table the draws follow and whose counters the resets feed.

    `domain_ranges` ({field: (lo, hi)}, `domain_shared`: `env.with_domain_ranges`), with "fresh" only: every fresh reset draws
    the env's physical domain anew inside the reset kernel, and the wrapper's `reset` draws that of the first episodes.
    Applied after `randomization_fn`, whose values an env keeps until its first redraw.  `body_domain_ranges`
    (`body_domain_shared`, `body_inertia_with_mass`: `env.with_body_domain_ranges`) does the same for body mass, principal
    moments and centre of mass, under the same rule."""
    if body_domain_ranges is not None and auto_reset != "fresh":
        raise ValueError("body_domain_ranges needs auto_reset='fresh': the cached first state belongs to one domain")
    if body_domain_ranges is None and (tuple(body_domain_shared) or body_inertia_with_mass):
        raise ValueError("body_domain_shared / body_inertia_with_mass without body_domain_ranges")
    if domain_ranges is not None and auto_reset != "fresh":
        raise ValueError("domain_ranges needs auto_reset='fresh': the cached first state belongs to one domain")
    if domain_ranges is None and tuple(domain_shared):
        raise ValueError("domain_shared without domain_ranges")
    if randomization_fn is not None:
        if not hasattr(env, "with_domain"):
            raise ValueError(f"{type(env).__name__} has no with_domain: domain randomisation needs a tracking env of this library")
        from .rodent import BODY_DOMAIN_FIELDS

        domain = dict(randomization_fn(env.sys))
        bodies = {k: domain.pop(k) for k in list(domain) if k in BODY_DOMAIN_FIELDS}
        if domain or not bodies:  # (an unknown key is with_domain's to refuse)
            env = env.with_domain(domain)
        if bodies:
            env = env.with_body_domain(bodies)
    if domain_ranges is not None:
        if not hasattr(env, "with_domain_ranges"):
            raise ValueError(f"{type(env).__name__} has no with_domain_ranges: a domain redraw needs a tracking env of this library")
        env = env.with_domain_ranges(domain_ranges, shared=domain_shared)
    if body_domain_ranges is not None:
        if not hasattr(env, "with_body_domain_ranges"):
            raise ValueError(f"{type(env).__name__} has no with_body_domain_ranges: a domain redraw needs a tracking env of this library")
        env = env.with_body_domain_ranges(body_domain_ranges, shared=body_domain_shared, inertia_with_mass=body_inertia_with_mass)
    return AutoResetWrapper(EpisodeWrapper(env, episode_length, action_repeat), reset_info_on_autoreset, mode=auto_reset,
                            seed=auto_reset_seed, env_offset=env_offset, start_priority=start_priority)
