"""Acting: counterpart of reference ppo_imitation/acting.py:34-156.

actor_step = policy call + env step + Transition row; generate_unroll = unroll_length of those
written into preallocated [T, B, ...] buffers (the env updates its State in place, so the
pre-step observation is copied into the buffer before stepping)."""
from __future__ import annotations

import dataclasses
import time
from typing import Any, Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ..envs.base import State
from ..envs.wrappers import EvalWrapper


@dataclasses.dataclass
class Transition:
    """brax.training.types.Transition [UPSTREAM]."""

    observation: torch.Tensor
    action: torch.Tensor
    reward: torch.Tensor
    discount: torch.Tensor
    next_observation: torch.Tensor
    extras: Dict[str, Dict[str, torch.Tensor]]

    def map(self, fn: Callable[[torch.Tensor], torch.Tensor]) -> "Transition":
        return Transition(fn(self.observation), fn(self.action), fn(self.reward), fn(self.discount),
                          fn(self.next_observation),
                          {k: {kk: fn(vv) for kk, vv in v.items()} for k, v in self.extras.items()})


def actor_step(env, env_state: State, policy, key, extra_fields: Sequence[str] = ()) -> Tuple[State, Transition]:
    """acting.py:34-57."""
    obs = env_state.obs.clone()
    traj = env_state.info["traj"]
    actions, policy_extras = policy(traj, obs, key)
    nstate = env.step(env_state, actions)
    state_extras = {x: nstate.info[x] for x in extra_fields}
    return nstate, Transition(observation=obs, action=actions, reward=nstate.reward, discount=1 - nstate.done,
                              next_observation=nstate.obs,
                              extras={"policy_extras": policy_extras, "state_extras": state_extras})


def _fusable(env, through_eval: bool = False):
    """AutoReset(Episode(RodentTracking)) with action_repeat 1 on the native library: the wrappers and the
    Transition logging of one step then collapse into ONE launch of vnl_rollout_post.  `through_eval`: the same under an
    EvalWrapper, for `evaluate_unroll`, which scores the steps on the device (a rollout that logged Transitions through
    the fused route would leave the wrapper's scores behind)."""
    from ..envs import wrappers as W

    if through_eval and isinstance(env, W.EvalWrapper):
        env = env.env
    if not isinstance(env, W.AutoResetWrapper) or not isinstance(env.env, W.EpisodeWrapper):
        return None
    ep, base = env.env, env.env.env
    if ep.action_repeat != 1 or base is not base.unwrapped or not hasattr(getattr(base, "_L", None), "vnl_rollout_post"):
        return None
    return env, ep, base


def _device_noise(policy) -> bool:
    """a policy of make_inference_fn(...)(params, noise="device"): draws keyed by (seed, counter + offset, env index)"""
    return getattr(policy, "noise", None) == "device"


# Private switch (tests compare the two): with a device-noise policy the unroll hands row t of its log buffers to the policy,
# which writes action / raw_action / log_prob / rand_log_prob / logits there itself; False = the policy allocates its outputs
# and vnl_rollout_post copies them into the log, as on the generator path.
_DIRECT_LOG = True
# Private switch (tests compare the two): the wrappers and the Transition logging of a step run as the EPILOGUE of the env
# step kernel (vnl_env_step_post: each wave post-processes the env it has just stepped); False = two launches,
# vnl_env_step + vnl_rollout_post.  A library without the entry, or an env whose `step` does more than launch the kernel
# (AntTracking), takes the two launches.
_POST_EPILOGUE = True


def _generate_unroll_fused(fz, env_state: State, policy, key, unroll_length: int, extra_fields) -> Tuple[State, Transition]:
    """Same results as the generic loop below (tests compare the two), 1 launch per step besides the
    policy: the env step kernel, whose waves run the post-processing of vnl_rollout_post (which also writes the
    Transition's observation row) as their epilogue (vnl_env_step_post; `_POST_EPILOGUE = False`: a launch of its own).  The
    step's descriptor reaches the kernel through `base.step`: a one-shot attribute of the env object, so that a hook around
    `base.step(state, action)` (bench.py's kernel events) sees the same call.  With
    AutoResetWrapper(mode="fresh") a further launch, vnl_env_reset_done, starts the new episodes and writes the rows the reset
    changes (next_observation, the logged info fields); its draws are keyed by info["reset_step"] + t.

    With a device-noise policy step t draws at `policy.counter + t` and the counter advances by T once, after the loop (one
    small launch per unroll instead of three noise launches per step; inside a captured graph the offsets are baked in and the
    add is a node of the graph)."""
    import ctypes as C

    from .. import _lib

    ar, ep, base = fz
    st = env_state
    T, info, dev = unroll_length, env_state.info, env_state.obs.device
    B = st.obs.shape[0]
    new = lambda *shape, like: torch.empty((T, *shape), dtype=like.dtype, device=dev)  # noqa: E731
    # Transition.observation[t + 1] IS next_observation[t] (the auto-reset wrapper's obs is what the next step sees), so only
    # the first row is copied; the policy reads the live observation buffer
    obs0, nobs_log = st.obs.clone(), new(*st.obs.shape, like=st.obs)
    rew_log, disc_log = new(B, like=st.reward), new(B, like=st.reward)
    sx_log = {x: new(*info[x].shape, like=info[x]) for x in extra_fields}
    prev_done = st.done.clone()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    width = lambda t: 1 if t.dim() == 1 else t.shape[1]  # noqa: E731

    d = _lib.PostDesc()
    d.steps, d.prev_done, d.done, d.truncation, d.reward = (ptr(info["steps"]), ptr(prev_done), ptr(st.done),
                                                            ptr(info["truncation"]), ptr(st.reward))
    d.episode_length, d.action_repeat = ep.episode_length, 1
    ops = []  # (dst, src, first, log rows [T, B, w] or None)
    fresh = getattr(ar, "mode", "first_state") == "fresh"
    if fresh:
        # a done env starts a NEW episode (vnl_env_reset_done after the post launch, mask = the finalised done): nothing is
        # restored from a first state, and what the reset rewrites -- obs, the info fields -- is logged by that launch
        reset_logs = [(st.obs, nobs_log)] + [(info[x], sx_log[x]) for x in extra_fields if x != "truncation"]
        # (a StartPriority of the wrapper's: the draws follow its table and the launch counts the ended episodes, those the
        # post-processing has just marked as truncated excepted; the tensors are fixed for a captured graph's life)
        prio_args = ar.priority_args(st)
    else:
        fps = info["first_pipeline_state"]
        for name in st.pipeline_state._FIELDS:
            cur = st.pipeline_state.raw(name)
            ops.append((cur, cur, fps.raw(name), None))
        ops.append((st.obs, st.obs, info["first_obs"], nobs_log))
        logged = set()
        if ar.reset_info:
            for k2, v in info["first_info"].items():
                ops.append((info[k2], info[k2], v, sx_log.get(k2)))
                logged.add(k2)
        for x in extra_fields:
            if x not in logged and x != "truncation":
                ops.append((None, info[x], None, sx_log[x]))
    n_static = len(ops)
    px_log: Optional[dict] = None
    act_log = None
    dev_noise = _device_noise(policy)
    direct = dev_noise and _DIRECT_LOG
    # (only where `step` IS the kernel launch: an env that works on the state after it -- AntTracking assembles its
    # observation there -- must be post-processed after that work, i.e. by the launch of its own)
    from ..envs.rodent import RodentTracking
    epilogue = _POST_EPILOGUE and hasattr(base._L, "vnl_env_step_post") and type(base).step is RodentTracking.step
    if direct:  # the policy writes row t of the log itself (contiguous [B, w] slices); the env step reads its action there
        na = base.action_size
        f32 = lambda *shape: torch.empty((T, *shape), dtype=torch.float32, device=dev)  # noqa: E731
        act_log = f32(B, na)
        px_log = {} if policy.deterministic else {"log_prob": f32(B), "rand_log_prob": f32(B), "raw_action": f32(B, na),
                                                  "logits": f32(B, 2 * na)}
    for t in range(T):
        if direct:
            actions, pex = policy(info["traj"], st.obs, None, step_offset=t, advance=False,
                                  out={"action": act_log[t], **{k2: v[t] for k2, v in px_log.items()}})
        elif dev_noise:
            actions, pex = policy(info["traj"], st.obs, None, step_offset=t, advance=False)
        else:
            actions, pex = policy(info["traj"], st.obs, key)
        if not epilogue:
            base.step(st, actions)
        if px_log is None:
            act_log = new(*actions.shape, like=actions)
            px_log = {k2: new(*v.shape, like=v) for k2, v in pex.items()}
        step_ops = ops[:n_static] if direct else ops[:n_static] + [(None, actions.contiguous(), None, act_log)] + \
            [(None, v.contiguous(), None, px_log[k2]) for k2, v in pex.items()]
        assert len(step_ops) <= _lib.POST_MAX_OPS
        d.num_ops = len(step_ops)
        keep = []
        for i, (dst, src, first, log) in enumerate(step_ops):
            assert src.dtype in (torch.float32, torch.int32) and src.is_contiguous()
            o = d.ops[i]
            o.dst, o.src, o.first, o.width = ptr(dst), ptr(src), ptr(first), width(src)
            o.log = ptr(log[t]) if log is not None else C.c_void_p(0)
            keep.append(src)
        d.log_reward, d.log_discount = ptr(rew_log[t]), ptr(disc_log[t])
        d.log_truncation = ptr(sx_log["truncation"][t]) if "truncation" in sx_log else C.c_void_p(0)
        if epilogue:  # (the descriptor is copied into the launch's arguments by the call)
            base._post_desc = d
            try:
                base.step(st, actions)
            finally:
                base._post_desc = None
        else:
            _lib.check(base._L, base._L.vnl_rollout_post(C.byref(d), B, stream))
        _generate_unroll_fused.hold = keep  # the launch is asynchronous: keep this step's sources alive
        if fresh:
            base.reset_done(st, st.done, seed=ar.seed, step_base=info["reset_step"], step_offset=t, env_offset=ar.env_offset,
                            logs=[(src, log[t]) for src, log in reset_logs], **prio_args)
    if fresh:  # (like policy.counter: the launches carry offsets 0..T-1, one add per unroll -- a node of a captured graph)
        info["reset_step"].add_(T)
    if dev_noise:
        policy.counter.add_(T)
    obs_log = torch.cat((obs0[None], nobs_log[:-1]), dim=0)
    data = Transition(observation=obs_log, action=act_log, reward=rew_log, discount=disc_log, next_observation=nobs_log,
                      extras={"policy_extras": px_log, "state_extras": sx_log})
    return st, data


class GraphedUnroll:
    """acting.generate_unroll (reference acting.py:60-80) captured ONCE into a hipGraph and replayed: the `unroll_length`
    policy launches, env step kernels, wrapper / logging launches and noise draws of an unroll are one graph launch instead
    of ~11 launches per step issued from Python (the eager loop leaves ~0.13 ms of launch gaps and small copies per control
    step on an MI355X).  Bit-identical to the eager fused unroll: same kernels, same arguments, same Philox stream
    (tests/test_fused_rollout.py).

    The graph works on fixed buffers: `env_state` (the env mutates it in place), the policy's parameter tensors (update them
    IN PLACE between replays: the trainer's flat parameter buffer already is; a normaliser state must be copied into the one
    given here) and the returned Transition, whose tensors are overwritten by the next replay.  `key` must be a generator
    on the device; it is registered with the graph, so every replay continues its stream as eager calls would.

    With a device-noise policy (make_policy(..., noise="device")) `key` is not used and no generator is registered: the
    launches carry step offsets 0..T-1 and the graph's last node adds T to `policy.counter`, the only state of the noise."""

    def __init__(self, env, env_state: State, policy, key: torch.Generator, unroll_length: int,
                 extra_fields: Sequence[str] = ()):
        fz = _fusable(env)
        dev = env_state.obs.device
        if fz is None or dev.type != "cuda":
            raise ValueError("GraphedUnroll needs AutoResetWrapper(EpisodeWrapper(<env on a HIP device>)), action_repeat 1")
        dev_noise = _device_noise(policy)
        if not dev_noise and (key is None or key.device.type != "cuda"):
            raise ValueError("GraphedUnroll needs a torch.Generator on the device (its stream is captured with the graph)")
        self._args = (fz, env_state, policy, key, int(unroll_length), tuple(extra_fields))
        self.state = env_state
        # warm-up on a side stream (library handles, the policy's kernel object, allocator pools), with the generator and the
        # env state put back afterwards: building the graph must not consume randomness or advance the envs
        gen_state = policy.counter.clone() if dev_noise else key.get_state()
        saved = _snapshot_state(env_state)
        prio = fz[0].start_priority  # (the warm-up's resets must not count either)
        counters = [prio.count_ended, prio.count_failed] if prio is not None else []
        saved_counters = [c.clone() for c in counters]
        # (.. nor redraw the domain: with ranges the warm-up's fresh resets write the library-owned tables)
        base = fz[0].unwrapped
        saved_domain = (base._copy_domain_tables() if getattr(base, "domain_ranges", None) is not None or
                        getattr(base, "body_domain_ranges", None) is not None else None)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _generate_unroll_fused(*self._args)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _restore_state(env_state, saved)
        for c, s0 in zip(counters, saved_counters):
            c.copy_(s0)
        if saved_domain is not None:
            base._copy_domain_tables(saved_domain)
        self.graph = torch.cuda.CUDAGraph()
        if dev_noise:
            policy.counter.copy_(gen_state)
        else:
            key.set_state(gen_state)
            self.graph.register_generator_state(key)
        with torch.cuda.graph(self.graph):
            _, self.data = _generate_unroll_fused(*self._args)
        self._hold = getattr(_generate_unroll_fused, "hold", None)
        _restore_state(env_state, saved)  # (capture does not execute, but keep the contract explicit)

    def __call__(self) -> Tuple[State, Transition]:
        self.graph.replay()
        return self.state, self.data


# Private switch (tests compare the two): the scoring of an evaluation step runs in the step kernel's launch
# (vnl_env_step_post_eval); False = three launches, vnl_env_step + vnl_rollout_post + vnl_rollout_eval, which an env whose
# `step` does more than launch the kernel (AntTracking) takes in any case.
_EVAL_EPILOGUE = True


def _eval_fusable(env):
    """EvalWrapper(AutoReset(Episode(tracking env))), action_repeat 1, on a library with the scoring entries"""
    from ..envs import wrappers as W

    fz = _fusable(env, through_eval=True) if isinstance(env, W.EvalWrapper) else None
    if fz is None or not hasattr(fz[2]._L, "vnl_rollout_eval"):
        return None
    return fz


def _evaluate_unroll_fused(ew, fz, st: State, policy, key, unroll_length: int, recorder=None) -> State:
    """`unroll_length` evaluation steps with no Transition log: per step the policy, ONE launch that steps, applies the
    Episode / AutoReset wrappers (its ops are the first-state restores only, every log pointer null) and scores
    (vnl_env_step_post_eval) and, with AutoResetWrapper(mode="fresh"), vnl_env_reset_done with no logs.  The device-noise
    and reset counters advance once, after the loop, as in `_generate_unroll_fused`.  `recorder` (a RolloutRecorder): one
    more launch per step, vnl_env_record, after the step's launch and before the fresh reset."""
    import ctypes as C

    from .. import _lib
    from ..envs.rodent import RodentTracking

    ar, ep, base = fz
    T, info, dev = unroll_length, st.info, st.obs.device
    B = st.obs.shape[0]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    raw = info["_raw"]
    prev_done = st.done.clone()
    d = _lib.PostDesc()
    d.steps, d.prev_done, d.done, d.truncation, d.reward = (ptr(info["steps"]), ptr(prev_done), ptr(st.done),
                                                            ptr(info["truncation"]), ptr(st.reward))
    d.episode_length, d.action_repeat = ep.episode_length, 1
    fresh = getattr(ar, "mode", "first_state") == "fresh"
    ops = []
    if not fresh:
        fps = info["first_pipeline_state"]
        for name in st.pipeline_state._FIELDS:
            cur = st.pipeline_state.raw(name)
            ops.append((cur, fps.raw(name)))
        ops.append((st.obs, info["first_obs"]))
        if ar.reset_info:
            ops += [(info[k2], v) for k2, v in info["first_info"].items()]
    d.num_ops = len(ops)
    for o, (cur, first) in zip(d.ops, ops):
        assert cur.dtype in (torch.float32, torch.int32) and cur.is_contiguous() and first.is_contiguous()
        o.dst, o.src, o.first, o.log, o.width = ptr(cur), ptr(cur), ptr(first), C.c_void_p(0), 1 if cur.dim() == 1 else cur.shape[1]
    e = _lib.EvalDesc()
    e.done, e.steps, e.truncation, e.reward, e.metrics = (ptr(st.done), ptr(info["steps"]), ptr(info["truncation"]),
                                                          ptr(st.reward), ptr(raw["metrics"]))
    e.cur_frame, e.sub_clip_frame, e.clip_id = ptr(raw["cur_frame"]), ptr(raw["sub_clip_frame"]), ptr(raw["clip_id"])
    e.run, e.count, e.records = ptr(info["eval_run"]), ptr(info["eval_count"]), ptr(info["eval_records"])
    e.episodes_per_env = ew.episodes_per_env
    assert info["eval_records"].shape[1:] == (ew.episodes_per_env, _lib.EVAL_WIDTH) and info["eval_run"].shape[1] == 8
    epilogue = _EVAL_EPILOGUE and hasattr(base._L, "vnl_env_step_post_eval") and type(base).step is RodentTracking.step
    dev_noise = _device_noise(policy)
    for t in range(T):
        if dev_noise:
            actions, pex = policy(info["traj"], st.obs, None, step_offset=t, advance=False)
        else:
            actions, pex = policy(info["traj"], st.obs, key)
        if epilogue:  # (the descriptors are copied into the launch's arguments by the call)
            base._post_desc, base._eval_desc = d, e
            try:
                base.step(st, actions)
            finally:
                base._post_desc = base._eval_desc = None
        else:
            base.step(st, actions)
            _lib.check(base._L, base._L.vnl_rollout_post(C.byref(d), B, stream))
            _lib.check(base._L, base._L.vnl_rollout_eval(C.byref(e), B, stream))
        if recorder is not None:  # (first_state: the done row's state columns are the restored first state, as brax returns it)
            recorder.record(st, actions, pex)
        if fresh:
            base.reset_done(st, st.done, seed=ar.seed, step_base=info["reset_step"], step_offset=t, env_offset=ar.env_offset)
    _evaluate_unroll_fused.hold = prev_done  # the launches are asynchronous
    if fresh:
        info["reset_step"].add_(T)
    if dev_noise:
        policy.counter.add_(T)
    return st


def evaluate_unroll(env, env_state: State, policy, key, unroll_length: int, fused: Optional[bool] = None,
                    recorder=None) -> State:
    """`unroll_length` steps of EvalWrapper(...) `env` for their scores alone (info["eval_records"] and its companions): no
    Transition is kept.  `fused` (default: whenever possible) runs the wrappers and the scoring on the device,
    `_evaluate_unroll_fused`; otherwise the wrappers step in torch ops.  The two give the same records, bit for bit.
    `recorder` (a RolloutRecorder): one row per step, written after the step's post-processing and scoring and before a fresh
    auto-reset -- in "fresh" mode the done row holds the true terminal state, in "first_state" mode its state columns hold the
    restored first state (what brax's wrapped env returns) beside the terminal step's reward, done, metrics and
    termination_error.  Row 0, the reset state, is the caller's: `recorder.record(state)` after `env.reset`."""
    fz = _eval_fusable(env) if fused is not False else None
    if fused is True and fz is None:
        raise ValueError("fused evaluation needs EvalWrapper(AutoResetWrapper(EpisodeWrapper(<tracking env>))), action_repeat 1")
    if fz is not None:
        st = _evaluate_unroll_fused(env, fz, env_state, policy, key, unroll_length, recorder)
        env.sync_eval_metrics(st)
        return st
    # (under a fresh auto-reset the row must be written inside the step, between the scoring and the reset: EvalWrapper's hook)
    hooked = recorder is not None and isinstance(env, EvalWrapper) and env._fresh() is not None
    for _ in range(unroll_length):
        actions, pex = policy(env_state.info["traj"], env_state.obs, key)
        if hooked:
            env.after_score = lambda st, a=actions, x=pex: recorder.record(st, a, x)
        try:
            env_state = env.step(env_state, actions)
        finally:
            if hooked:
                env.after_score = None
        if recorder is not None and not hooked:
            recorder.record(env_state, actions, pex)
    return env_state


class GraphedEval:
    """`evaluate_unroll` on the fused route with `graph_steps` steps captured ONCE into a hipGraph: an evaluation of
    `unroll_length` steps is `unroll_length // graph_steps` replays and an eager tail of the remaining steps.  Same kernels,
    same arguments, same streams of noise as the eager fused route: the same records.  `recorder` (a RolloutRecorder): its
    launch is captured with every step; the cursor lives on the device, so replays advance it.

    The graph works on the buffers of the `env_state` given here; `__call__(state)` copies another state of the same env
    (a new `env.reset`) into them first.  The policy's parameter tensors are fixed likewise (update them in place).  A
    generator policy needs `key` on the device (registered with the graph); a device-noise policy carries step offsets
    0..graph_steps-1 in the captured launches and the graph's last node advances its counter, as in GraphedUnroll."""

    def __init__(self, env, env_state: State, policy, key, unroll_length: int, graph_steps: int = 20, recorder=None):
        fz = _eval_fusable(env)
        dev = env_state.obs.device
        if fz is None or dev.type != "cuda":
            raise ValueError("GraphedEval needs EvalWrapper(AutoResetWrapper(EpisodeWrapper(<env on a HIP device>))), action_repeat 1")
        dev_noise = _device_noise(policy)
        if not dev_noise and (key is None or key.device.type != "cuda"):
            raise ValueError("GraphedEval needs a torch.Generator on the device (its stream is captured with the graph)")
        self.env, self.state, self.policy, self.key = env, env_state, policy, key
        self.graph_steps = max(1, min(int(graph_steps), int(unroll_length)))
        self.replays, self.tail = divmod(int(unroll_length), self.graph_steps)
        self._fz, self.recorder = fz, recorder
        args = (env, fz, env_state, policy, key, self.graph_steps, recorder)
        # warm-up on a side stream with everything put back afterwards, as in GraphedUnroll
        gen_state = policy.counter.clone() if dev_noise else key.get_state()
        saved = _snapshot_state(env_state)
        saved_rec = recorder._snapshot() if recorder is not None else None
        base = fz[0].unwrapped
        saved_domain = (base._copy_domain_tables() if getattr(base, "domain_ranges", None) is not None or
                        getattr(base, "body_domain_ranges", None) is not None else None)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _evaluate_unroll_fused(*args)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _restore_state(env_state, saved)
        if saved_rec is not None:
            recorder._restore(saved_rec)
        if saved_domain is not None:
            base._copy_domain_tables(saved_domain)
        self.graph = torch.cuda.CUDAGraph()
        if dev_noise:
            policy.counter.copy_(gen_state)
        else:
            key.set_state(gen_state)
            self.graph.register_generator_state(key)
        with torch.cuda.graph(self.graph):
            _evaluate_unroll_fused(*args)
        _restore_state(env_state, saved)

    def __call__(self, state: Optional[State] = None) -> State:
        if state is not None and state is not self.state:
            for dst, src in zip(_state_tensors(self.state), _state_tensors(state)):
                dst.copy_(src)
        for _ in range(self.replays):
            self.graph.replay()
        if self.tail:
            _evaluate_unroll_fused(self.env, self._fz, self.state, self.policy, self.key, self.tail, self.recorder)
        self.env.sync_eval_metrics(self.state)
        return self.state


def _state_tensors(st: State):
    out = [st.pipeline_state.raw(n) for n in st.pipeline_state._FIELDS] + [st.obs, st.reward, st.done]
    for k in sorted(st.info):
        v = st.info[k]
        if isinstance(v, torch.Tensor):
            out.append(v)
        elif isinstance(v, dict):
            out += [v[k2] for k2 in sorted(v) if isinstance(v[k2], torch.Tensor)]
        elif hasattr(v, "_FIELDS") and hasattr(v, "raw"):  # (the cached first pipeline state of a first_state auto-reset)
            out += [v.raw(n) for n in v._FIELDS]
    seen, uniq = set(), []
    for t in out:  # (info["_raw"] aliases obs / reward / ...: each storage once)
        if t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            uniq.append(t)
    return uniq


def _snapshot_state(st: State):
    return [t.clone() for t in _state_tensors(st)]


def _restore_state(st: State, saved) -> None:
    for t, s in zip(_state_tensors(st), saved):
        t.copy_(s)


def generate_unroll(env, env_state: State, policy, key, unroll_length: int,
                    extra_fields: Sequence[str] = (), fused: Optional[bool] = None) -> Tuple[State, Transition]:
    """acting.py:60-80: Transitions stacked on a leading time axis [T, B, ...], written row by row into
    buffers allocated once per call (the env mutates its State in place).
    NB (reference behaviour): state_extras['traj'] is nstate.info['traj'], i.e. the reference
    trajectory features AFTER the step (acting.py:49), not the ones the policy saw.
    `fused` (default: whenever possible) routes the wrappers + logging through vnl_rollout_post.  With
    AutoResetWrapper(mode="fresh") the fused route logs obs and every extra field but "truncation" through the 8 log slots
    of vnl_env_reset_done: at most 7 such extra fields (ValueError beyond; `fused=False` has no such limit)."""
    fz = _fusable(env) if fused is not False else None
    if fused is True and fz is None:
        raise ValueError("fused rollout needs AutoResetWrapper(EpisodeWrapper(RodentTracking)), action_repeat 1")
    if fz is not None:
        return _generate_unroll_fused(fz, env_state, policy, key, unroll_length, tuple(extra_fields))
    data: Optional[Transition] = None
    for t in range(unroll_length):
        env_state, tr = actor_step(env, env_state, policy, key, extra_fields=extra_fields)
        if data is None:
            alloc = lambda x: torch.empty((unroll_length, *x.shape), dtype=x.dtype, device=x.device)  # noqa: E731
            data = tr.map(alloc)
        for dst, src in zip(_leaves(data), _leaves(tr)):
            dst[t].copy_(src)
    return env_state, data


def _leaves(tr: Transition):
    out = [tr.observation, tr.action, tr.reward, tr.discount, tr.next_observation]
    for g in sorted(tr.extras):
        out += [tr.extras[g][k] for k in sorted(tr.extras[g])]
    return out


def _clone_param(p):
    if dataclasses.is_dataclass(p):
        return dataclasses.replace(p, **{f.name: getattr(p, f.name).clone() for f in dataclasses.fields(p)
                                         if isinstance(getattr(p, f.name), torch.Tensor)})
    return p.clone() if isinstance(p, torch.Tensor) else p


def _copy_params(dst, src) -> None:
    """the (normaliser state, flat parameters) pair of make_inference_fn, in place"""
    for a, b in zip(dst, src):
        if isinstance(a, torch.Tensor):
            a.copy_(b)
        elif dataclasses.is_dataclass(a):
            for f in dataclasses.fields(a):
                if isinstance(getattr(a, f.name), torch.Tensor):
                    getattr(a, f.name).copy_(getattr(b, f.name))


class Evaluator:
    """acting.py:84-156, with `episodes_per_env` scored episodes per env (envs/wrappers.py EvalWrapper; 1 = the reference).

    The unroll is `episodes_per_env * episode_length // action_repeat` steps.  A fusable env (`_eval_fusable`) is stepped,
    wrapped and scored on the device (`evaluate_unroll`); `graphed` (default: on a HIP device, when the policy draws
    device noise or `key` lives on the device) replays `graph_steps` captured steps at a time (GraphedEval).  Any other env
    goes through the generic `generate_unroll` loop.  `fused=False` forces that loop.
    `records` is the (N, 12) float32 array of the last evaluation's completed episodes (`_lib.EVAL_COLUMNS`, then the seven
    metrics and the reward), envs in order, each env's episodes in order.
    `record_envs` > 0: the first episode of the first `record_envs` envs is recorded step by step on the device
    (RolloutRecorder: the reset row, then at most `record_steps` rows, default the unroll's length); `recorded` holds the last
    evaluation's RecordedRollout.  With 0 nothing is allocated or launched."""

    def __init__(self, eval_env, eval_policy_fn, num_eval_envs: int, episode_length: int, action_repeat: int,
                 key: Optional[torch.Generator], episodes_per_env: int = 1, graphed: Optional[bool] = None,
                 graph_steps: int = 20, fused: Optional[bool] = None, record_envs: int = 0, record_steps: Optional[int] = None):
        self._key = key
        self._eval_walltime = 0.0
        self._K = int(episodes_per_env)
        self._env = EvalWrapper(eval_env, episodes_per_env=self._K)
        self._policy_fn = eval_policy_fn
        self._unroll = self._K * episode_length // action_repeat
        self._steps_per_unroll = self._K * episode_length * num_eval_envs
        self._fused = fused is not False and _eval_fusable(self._env) is not None
        if fused is True and not self._fused:
            raise ValueError("fused evaluation needs AutoResetWrapper(EpisodeWrapper(<tracking env>)), action_repeat 1")
        self._graphed, self._graph_steps, self._graph = graphed, int(graph_steps), None
        self.records: Optional[np.ndarray] = None
        self.state: Optional[State] = None  # the eval envs as the last evaluation left them
        # recorded rollouts: the first episode of the first `record_envs` envs, one row per step after the reset row
        self._recorder = None
        if int(record_envs) > 0:
            self._recorder = RolloutRecorder(self._env, num_record=int(record_envs),
                                             capacity=1 + int(self._unroll if record_steps is None else record_steps))
        self.recorded: Optional[RecordedRollout] = None  # the last evaluation's (None without record_envs)

    def _unroll_state(self, policy_params) -> State:
        """the state after the evaluation's unroll, by the route chosen at construction"""
        state = self._env.reset(self._key)
        rec = self._recorder
        if rec is not None:
            rec.reset()
            rec.record(state)
        if not self._fused:
            if rec is not None:  # (the same steps as the loop below, the state alone kept)
                return evaluate_unroll(self._env, state, self._policy_fn(policy_params), self._key, self._unroll, fused=False,
                                       recorder=rec)
            state, _ = generate_unroll(self._env, state, self._policy_fn(policy_params), self._key, self._unroll)
            return state
        if self._graph is None:
            policy = self._policy_fn(policy_params)
            on_dev = state.obs.device.type == "cuda"
            can = on_dev and (_device_noise(policy) or (self._key is not None and self._key.device.type == "cuda"))
            if self._graphed and not can:
                raise ValueError("a graphed evaluation needs a HIP device and device noise or a generator on the device")
            if not (can if self._graphed is None else self._graphed):
                return evaluate_unroll(self._env, state, policy, self._key, self._unroll, fused=True, recorder=rec)
            # (the graph reads fixed parameter tensors: copies of its own, refreshed before every evaluation)
            self._params = tuple(_clone_param(p) for p in policy_params)
            self._graph = GraphedEval(self._env, state, self._policy_fn(self._params), self._key, self._unroll,
                                      graph_steps=self._graph_steps, recorder=rec)
        _copy_params(self._params, policy_params)
        return self._graph(state)

    def run_evaluation(self, policy_params, training_metrics: Dict[str, Any], aggregate_episodes: bool = True):
        t = time.time()
        state = self.state = self._unroll_state(policy_params)
        em = state.info["eval_metrics"]
        if em.active_episodes.is_cuda:
            torch.cuda.synchronize(em.active_episodes.device)
        epoch_eval_time = time.time() - t
        count = state.info["eval_count"].cpu().numpy()
        recs = state.info["eval_records"].cpu().numpy()
        self.records = recs[np.arange(recs.shape[1])[None, :] < count[:, None]]
        if self._recorder is not None:
            self.recorded = self._recorder.result()
        metrics = {}
        if self._K == 1:
            per_episode = {name: v.cpu().numpy() for name, v in em.episode_metrics.items()}
            lengths = em.episode_steps.cpu().numpy()
        else:  # over all completed episodes
            per_episode = {name: self.records[:, 4 + self._env.columns[name]] for name in em.episode_metrics}
            lengths = self.records[:, 2]
        for fn in (np.mean, np.std):
            suffix = "_std" if fn is np.std else ""
            metrics.update({f"eval/episode_{name}{suffix}": (fn(v) if aggregate_episodes else v)
                            for name, v in per_episode.items()})
        metrics["eval/avg_episode_length"] = float(np.mean(lengths))
        if self._K > 1:
            metrics["eval/episodes_scored"] = int(self.records.shape[0])
            metrics["eval/truncated_fraction"] = float(np.mean(self.records[:, 3] != 0))
        metrics["eval/epoch_eval_time"] = epoch_eval_time
        metrics["eval/sps"] = self._steps_per_unroll / epoch_eval_time
        self._eval_walltime += epoch_eval_time
        return {"eval/walltime": self._eval_walltime, **training_metrics, **metrics}


# ---- recorded rollouts: per-step traces of chosen envs, written on the device (include/vnl.h vnl_record_desc) ----
RECORD_COLUMNS = ("cur_frame", "clip_id", "steps", "done", "reward", "termination_error", "metrics", "qpos", "qvel", "action",
                  "logits", "log_prob", "rand_log_prob")
_RECORD_POLICY_COLUMNS = ("action", "logits", "log_prob", "rand_log_prob")
# Private switch (tests compare the two): a row is written by vnl_env_record; False = by the restatement in torch ops,
# which a library without the entry takes in any case.
_RECORD_KERNEL = True


@dataclasses.dataclass
class RecordedRollout:
    """What a RolloutRecorder has written, as NumPy arrays: `length` (R,) rows recorded per recorder, `env_index` (R,) the env
    each watched, and per column an (R, capacity, w) array in `columns` (also reachable as attributes: `rec.qpos`), rows at or
    beyond `length` zero.  `ref_qpos` (R, capacity, nq) is the reference clip's pose at the env's frame and
    `render_qpos = concatenate([ref_qpos, qpos], -1)` what the reference hands its renderer (train.py:289-293).  Row 0 is the
    reset state (its policy columns are NaN); row k pairs the policy outputs that chose action k with the state it led to."""

    length: np.ndarray
    env_index: np.ndarray
    columns: Dict[str, np.ndarray]
    ref_qpos: Optional[np.ndarray] = None

    def __getattr__(self, name):
        cols = self.__dict__.get("columns") or {}
        if name in cols:
            return cols[name]
        raise AttributeError(name)

    @property
    def render_qpos(self) -> np.ndarray:
        return np.concatenate([self.ref_qpos, self.columns["qpos"]], axis=-1)

    def save(self, path) -> None:
        extra = {} if self.ref_qpos is None else {"ref_qpos": self.ref_qpos}
        np.savez(path, length=self.length, env_index=self.env_index, **extra, **{"col." + k: v for k, v in self.columns.items()})

    @classmethod
    def load(cls, path) -> "RecordedRollout":
        with np.load(path) as z:
            return cls(length=z["length"], env_index=z["env_index"], ref_qpos=z["ref_qpos"] if "ref_qpos" in z else None,
                       columns={k[4:]: z[k] for k in z.files if k.startswith("col.")})


class RolloutRecorder:
    """One row per `record(state, action, policy_extras)` call for each of R recorders, in ONE launch (vnl_env_record): the
    reference pose of the env's clip at its frame, then the columns RECORD_COLUMNS read from `state` and the policy's outputs,
    then `extra` -- {name: (B[, w]) float32 / int32 tensor on the env's device}, read live at every call (a decoder policy's
    `latent_out`, say); at most 16 columns in all.  Recorder r watches env `env_index[r]` (default: env r of the first
    `num_record`); an index outside the batch records nothing.  `capacity` rows per recorder; with `stop_at_done` a recorder
    closes after the row on which its env's `done` is set.  `rows`, `count` and `open` live on the device and the call has no
    host synchronisation: it can be captured in a hipGraph, whose replays advance the cursor.  A column the state or the call
    does not have (no `steps` without an EpisodeWrapper; no policy outputs and no `extra` on the reset row, the call without
    an action) is NaN words."""

    def __init__(self, env, num_record: Optional[int] = None, env_index=None, capacity: int = 1, stop_at_done: bool = True,
                 extra: Optional[Dict[str, torch.Tensor]] = None):
        base = env.unwrapped
        self.base, self.device, B = base, base.device, base.num_envs
        if (num_record is None) == (env_index is None):
            raise ValueError("give num_record or env_index")
        if env_index is not None:
            self.env_index = torch.as_tensor(env_index, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
            R = int(self.env_index.numel())
        else:
            self.env_index, R = None, int(num_record)
        if R < 1 or int(capacity) < 1:
            raise ValueError("a recorder needs at least one env and a capacity of at least 1")
        d = base.dims
        nq, nv, nu = int(d.nq), int(d.nv), int(d.nu)
        widths = dict(cur_frame=1, clip_id=1, steps=1, done=1, reward=1, termination_error=1, metrics=7, qpos=nq, qvel=nv,
                      action=nu, logits=2 * nu, log_prob=1, rand_log_prob=1)
        self.extra = dict(extra or {})
        for k, t in self.extra.items():
            if k in widths or t.dtype not in (torch.float32, torch.int32) or t.dim() not in (1, 2) or t.shape[0] != B or \
                    not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"extra[{k!r}] must be a new name and a contiguous float32 / int32 ({B}[, w]) tensor on the env's device")
        self.columns = [(k, widths[k]) for k in RECORD_COLUMNS] + [(k, t.numel() // B) for k, t in self.extra.items()]
        from .. import _lib

        if len(self.columns) > _lib.RECORD_MAX_COLS:
            raise ValueError(f"at most {_lib.RECORD_MAX_COLS} columns: {_lib.RECORD_MAX_COLS - len(RECORD_COLUMNS)} extra ones")
        self._int = {"cur_frame", "clip_id"} | {k for k, t in self.extra.items() if t.dtype == torch.int32}
        self.nq, self.num_record, self.capacity, self.stop_at_done = nq, R, int(capacity), bool(stop_at_done)
        self.row_width = nq + sum(w for _, w in self.columns)
        self.rows = torch.zeros((R, self.capacity, self.row_width), dtype=torch.float32, device=self.device)
        self.count = torch.zeros(R, dtype=torch.int32, device=self.device)
        self.open = torch.ones(R, dtype=torch.int32, device=self.device)
        self._ref = None  # (C, T, nq) int32 words of the clip's pose, for the restatement
        self._hold = None

    def reset(self) -> None:
        """rearm: every recorder open at row 0 (the rows are zeroed)"""
        self.rows.zero_()
        self.count.zero_()
        self.open.fill_(1)

    def _sources(self, state: State, action, policy_extras):
        raw, info, ps = state.info["_raw"], state.info, state.pipeline_state
        px = dict(policy_extras or {})
        src = dict(cur_frame=raw["cur_frame"], clip_id=raw["clip_id"], steps=info.get("steps"), done=state.done,
                   reward=state.reward, termination_error=raw["termination_error"], metrics=raw["metrics"], qpos=ps.raw("qpos"),
                   qvel=ps.raw("qvel"), action=action, logits=px.get("logits"), log_prob=px.get("log_prob"),
                   rand_log_prob=px.get("rand_log_prob"),
                   **{k: (t if action is not None else None) for k, t in self.extra.items()})  # (no action: the reset row)
        B, out = self.base.num_envs, []
        for k, w in self.columns:
            t = src[k]
            if t is not None:
                want = torch.int32 if k in self._int else torch.float32
                if t.dtype != want or t.device != self.device or t.shape[0] != B or t.numel() != B * w:
                    raise ValueError(f"column {k!r} must be a {want} ({B}, {w}) tensor on the env's device, got {t.dtype} "
                                     f"{tuple(t.shape)}")
                t = t.contiguous()
            out.append(t)
        return out, raw

    def record(self, state: State, action: Optional[torch.Tensor] = None, policy_extras: Optional[dict] = None) -> None:
        """one row for every open recorder: the state as it stands, beside the action that led to it and the policy outputs
        that chose the action (none: the reset row)"""
        from .. import _lib

        srcs, raw = self._sources(state, action, policy_extras)
        L = self.base._L
        if not (_RECORD_KERNEL and hasattr(L, "vnl_env_record")):
            return self._record_torch(srcs, raw, state.done)
        import ctypes as C

        d = _lib.RecordDesc()
        d.env_index = self.env_index.data_ptr() if self.env_index is not None else None
        d.done, d.ref_frame, d.ref_clip = state.done.data_ptr(), raw["cur_frame"].data_ptr(), raw["clip_id"].data_ptr()
        d.count, d.open, d.rows = self.count.data_ptr(), self.open.data_ptr(), self.rows.data_ptr()
        d.num_rec, d.capacity, d.row_width = self.num_record, self.capacity, self.row_width
        d.stop_at_done, d.num_cols = int(self.stop_at_done), len(self.columns)
        for o, t, (_, w) in zip(d.cols, srcs, self.columns):
            o.src, o.width = (t.data_ptr() if t is not None else None), w
        _lib.check(L, L.vnl_env_record(self.base._env_h, C.byref(d), self.base._stream()))
        self._hold = srcs  # the launch is asynchronous: keep this step's sources alive

    def _record_torch(self, srcs, raw, done) -> None:
        """include/vnl.h above vnl_record_desc in torch ops: the same words in rows, count and open"""
        base, dev, R, B = self.base, self.device, self.num_record, self.base.num_envs
        if self._ref is None:
            c = base._clip
            pose = np.concatenate([c["position"], c["quaternion"], c["joints"]], axis=-1).astype(np.float32)
            self._ref = torch.from_numpy(np.ascontiguousarray(pose)).to(dev).view(torch.int32)
        idx = (self.env_index if self.env_index is not None else torch.arange(R, dtype=torch.int32, device=dev)).long()
        valid = (idx >= 0) & (idx < B) & (self.open != 0) & (self.count < self.capacity)
        e = idx.clamp(0, B - 1)
        Cn, Tn = self._ref.shape[:2]
        frame, clip = raw["cur_frame"][e].long().clamp(0, Tn - 1), raw["clip_id"][e].long().clamp(0, Cn - 1)
        parts = [self._ref[clip, frame]]
        for t, (_, w) in zip(srcs, self.columns):
            parts.append(t.view(torch.int32).reshape(B, w)[e] if t is not None else
                         torch.full((R, w), 0x7FC00000, dtype=torch.int32, device=dev))
        row = torch.cat(parts, dim=1)
        words = self.rows.view(torch.int32)
        r, slot = torch.arange(R, device=dev), self.count.clamp(max=self.capacity - 1).long()
        words[r, slot] = torch.where(valid[:, None], row, words[r, slot])
        self.count += valid.to(torch.int32)
        if self.stop_at_done:
            self.open.copy_(torch.where(valid & (done[e] != 0), torch.zeros_like(self.open), self.open))

    def result(self) -> RecordedRollout:
        """the rows recorded so far (synchronises with the device)"""
        rows = self.rows.cpu().numpy()  # (rows at or beyond the count are zero: zeroed by `reset`, never written since)
        length = self.count.cpu().numpy().copy()
        at, cols = self.nq, {}
        ref = np.ascontiguousarray(rows[:, :, :at])
        for k, w in self.columns:
            a = np.ascontiguousarray(rows[:, :, at:at + w])
            cols[k] = a.view(np.int32) if k in self._int else a
            at += w
        idx = self.env_index.cpu().numpy().copy() if self.env_index is not None else np.arange(self.num_record, dtype=np.int32)
        return RecordedRollout(length=length, env_index=idx, columns=cols, ref_qpos=ref)

    # (a graph capture's warm-up runs real steps: what it wrote is put back)
    def _snapshot(self):
        return self.rows.clone(), self.count.clone(), self.open.clone()

    def _restore(self, saved) -> None:
        for t, s in zip((self.rows, self.count, self.open), saved):
            t.copy_(s)
