"""Shared by tests/test_eval_epilogue.py (host build) and tests/test_gpu_eval_epilogue.py (device): the scored episodes of an
evaluation (include/vnl.h vnl_eval_desc) -- vnl_rollout_eval against a NumPy restatement, vnl_env_step_post_eval against the
three launches it replaces, and the routes of acting.Evaluator against each other, bit for bit."""
import contextlib
import ctypes as C
import functools

import numpy as np
import torch

import post_epilogue_cases as PE
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import EvalWrapper, wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics

W = _lib.EVAL_WIDTH
SENTINEL = -77.0
_ptr = PE._ptr


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---------------------------------------------------------------------------------------------- 1. the standalone kernel
T_SYN, K_SYN = 7, 2


def synthetic(B, seed=0):
    """T_SYN steps of inputs for B envs.  env % 4 == 0: done on step 1, again on steps 4 and 6 (the third episode is beyond K);
    1: never done; 2: a NaN metric on step 2, done on steps 3 and 7; 3: done at random."""
    rng = np.random.default_rng(seed)
    e = np.arange(B)
    done = np.zeros((T_SYN, B), np.float32)
    done[0, e % 4 == 0] = done[3, e % 4 == 0] = done[5, e % 4 == 0] = 1
    done[2, e % 4 == 2] = done[6, e % 4 == 2] = 1
    done[:, e % 4 == 3] = (rng.random((T_SYN, int((e % 4 == 3).sum()))) < 0.3)
    metrics = rng.standard_normal((T_SYN, B, 7)).astype(np.float32)
    metrics[1, e % 4 == 2, 3] = np.nan
    f = lambda: rng.standard_normal((T_SYN, B)).astype(np.float32)  # noqa: E731
    i = lambda hi: rng.integers(0, hi, (T_SYN, B)).astype(np.int32)  # noqa: E731
    sub = i(40)
    return dict(done=done, steps=np.floor(10 * np.abs(f())).astype(np.float32), truncation=(rng.random((T_SYN, B)) < 0.5)
                .astype(np.float32) * done, reward=f(), metrics=metrics, sub_clip_frame=sub, cur_frame=sub + i(200), clip_id=i(3))


def restatement(inp, K, frames=True, truncation=True):
    """include/vnl.h above vnl_eval_desc, env by env and step by step, float32 adds"""
    Tn, B = inp["done"].shape
    run, count = np.zeros((B, 8), np.float32), np.zeros(B, np.int32)
    rec = np.full((B, K, W), SENTINEL, np.float32)
    for t in range(Tn):
        for e in range(B):
            c = count[e]
            if c >= K:
                continue
            for k in range(7):
                run[e, k] = np.float32(run[e, k] + inp["metrics"][t, e, k])
            run[e, 7] = np.float32(run[e, 7] + inp["reward"][t, e])
            if inp["done"][t, e] != 0:
                rec[e, c, 0] = np.float32(inp["cur_frame"][t, e] - inp["sub_clip_frame"][t, e]) if frames else -1
                rec[e, c, 1] = np.float32(inp["clip_id"][t, e]) if frames else -1
                rec[e, c, 2] = inp["steps"][t, e]
                rec[e, c, 3] = inp["truncation"][t, e] if truncation else 0
                rec[e, c, 4:] = run[e]
                run[e] = 0
                count[e] = c + 1
    return dict(run=run, count=count, records=rec)


def run_standalone(L, dev, inp, K, frames=True, truncation=True):
    Tn, B = inp["done"].shape
    d_in = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    run, count = torch.zeros(B, 8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    rec = torch.full((B, K, W), SENTINEL, device=dev)
    stream = PE._stream(dev)
    for t in range(Tn):
        d = _lib.EvalDesc()
        for k in ("done", "steps", "reward", "metrics") + (("truncation",) if truncation else ()) + \
                (("cur_frame", "sub_clip_frame", "clip_id") if frames else ()):
            setattr(d, k, _ptr(d_in[k][t]))
        d.run, d.count, d.records, d.episodes_per_env = _ptr(run), _ptr(count), _ptr(rec), K
        _lib.check(L, L.vnl_rollout_eval(C.byref(d), B, stream))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return dict(run=run.cpu().numpy(), count=count.cpu().numpy(), records=rec.cpu().numpy())


def check_standalone(L, dev, B):
    inp = synthetic(B, seed=B)
    for frames, truncation in ((True, True), (False, False)):
        want = restatement(inp, K_SYN, frames, truncation)
        got = run_standalone(L, dev, inp, K_SYN, frames, truncation)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), (k, frames)
        rows = np.arange(K_SYN)[None, :] >= got["count"][:, None]
        assert np.all(got["records"][rows] == SENTINEL)  # rows at or beyond count are never written
        rec, e = got["records"], np.arange(B)
        assert got["count"][0] == K_SYN and np.all(got["count"][e % 4 == 1] == 0)  # done on step 1 (then twice); never done
        if B > 2:  # the NaN stays in the episode it fell into: the first of env 2, not its second
            assert np.isnan(rec[2, 0, 4 + 3]) and not np.isnan(rec[2, 1]).any() and not np.isnan(np.delete(rec[2, 0], 7)).any()
            assert not np.isnan(rec[e % 4 != 2][rec[e % 4 != 2] != SENTINEL]).any()
        if not frames:
            assert np.all(rec[~rows][:, :2] == -1) and np.all(rec[~rows][:, 3] == 0)


# ---------------------------------------------------------------------------------- 2. the fused entry = three launches
EPISODE_LENGTH, K_DIRECT = 4, 2


def direct_case(base, fused: bool):
    """One step on a freshly reset state of `base` (5 envs), as post_epilogue_cases.direct_case builds it: env 0 terminates on
    its own, env 1 reaches the episode length (truncation 1), env 2 comes with count == K, env 3 is in the middle of an
    episode, env 4 completes its K-th episode.  The post ops restore the state and the frame counter from a 'first' row, so
    that the scoring reads rows the post-processing has just written.  Returns every buffer of both descriptors and every
    state row (CPU)."""
    B, dev = base.num_envs, base.device
    assert B == 5
    g = torch.Generator().manual_seed(3)
    sf = torch.randint(0, 100, (B,), generator=g, dtype=torch.int32)
    nq, nu = int(base.dims.nq), int(base.dims.nu)
    st = base.reset(start_frame=sf, noise=1e-3 * torch.randn(B, nq, generator=g))
    st.pipeline_state.raw("qpos")[0, 2] += 5.0
    action = (0.3 * torch.randn(B, nu, generator=g)).clamp(-1, 1).to(dev)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    c = {"steps": torch.tensor([0, EPISODE_LENGTH - 1, 1, 1, EPISODE_LENGTH - 1]).float().to(dev), "prev_done": torch.zeros(B).to(dev),
         "truncation": r(B), "run": r(B, 8), "count": torch.tensor([0, 0, K_DIRECT, 0, K_DIRECT - 1], dtype=torch.int32).to(dev),
         "records": r(B, K_DIRECT, W)}
    raw, ps = st.info["_raw"], st.pipeline_state
    ops = [(ps.raw("qpos"), ps.raw("qpos") + 1), (raw["obs"], raw["obs"] + 1), (raw["cur_frame"], raw["cur_frame"] + 5)]
    d = _lib.PostDesc()
    d.steps, d.prev_done, d.truncation, d.done, d.reward = (_ptr(c["steps"]), _ptr(c["prev_done"]), _ptr(c["truncation"]),
                                                            _ptr(raw["done"]), _ptr(raw["reward"]))
    d.episode_length, d.action_repeat, d.num_ops = EPISODE_LENGTH, 1, len(ops)
    for o, (cur, first) in zip(d.ops, ops):
        o.dst, o.src, o.first, o.width = _ptr(cur), _ptr(cur), _ptr(first), 1 if cur.dim() == 1 else cur.shape[1]
    e = _lib.EvalDesc()
    e.done, e.steps, e.truncation, e.reward, e.metrics = (_ptr(raw["done"]), _ptr(c["steps"]), _ptr(c["truncation"]),
                                                          _ptr(raw["reward"]), _ptr(raw["metrics"]))
    e.cur_frame, e.sub_clip_frame, e.clip_id = _ptr(raw["cur_frame"]), _ptr(raw["sub_clip_frame"]), _ptr(raw["clip_id"])
    e.run, e.count, e.records, e.episodes_per_env = _ptr(c["run"]), _ptr(c["count"]), _ptr(c["records"]), K_DIRECT
    before = {k: v.cpu().clone() for k, v in c.items()}
    L, p = base._L, base._ptrs(st)
    if fused:
        _lib.check(L, L.vnl_env_step_post_eval(base._env_h, action.data_ptr(), C.byref(p), C.byref(d), C.byref(e), PE._stream(dev)))
    else:
        _lib.check(L, L.vnl_env_step(base._env_h, action.data_ptr(), C.byref(p), PE._stream(dev)))
        own_done = raw["done"].clone()
        _lib.check(L, L.vnl_rollout_post(C.byref(d), B, PE._stream(dev)))
        _lib.check(L, L.vnl_rollout_eval(C.byref(e), B, PE._stream(dev)))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    out = {k: v.cpu() for k, v in c.items()}
    out.update({"state." + n: ps.raw(n).cpu() for n in ps._FIELDS})
    out.update({"state." + k: v.cpu() for k, v in raw.items()})
    out.update({f"first{k}": first.cpu() for k, (_, first) in enumerate(ops)})
    if not fused:  # the case is what it claims to be (judged on the three-launch form)
        own, done, tr, cnt, rec = own_done.cpu(), out["state.done"], out["truncation"], out["count"], out["records"]
        assert own[0] == 1 and done[0] == 1 and tr[0] == 0 and cnt[0] == 1 and rec[0, 0, 3] == 0   # env 0: on its own
        assert own[1] == 0 and done[1] == 1 and tr[1] == 1 and cnt[1] == 1 and rec[1, 0, 3] == 1   # env 1: the episode length
        cur, sub = out["state.cur_frame"], out["state.sub_clip_frame"]  # .. steps and frame as the post launch left them
        assert rec[1, 0, 2] == EPISODE_LENGTH and cur[1] == sf[1] + 5 and rec[1, 0, 0] == float(cur[1] - sub[1])
        for k in ("run", "count", "records"):                                         # env 2: nothing of its rows changes
            assert torch.equal(out[k][2], before[k][2]), k
        assert done[3] == 0 and cnt[3] == 0 and torch.equal(out["records"][3], before["records"][3])  # env 3: mid-episode
        assert torch.equal(out["run"][3], before["run"][3] + torch.cat([out["state.metrics"][3], out["state.reward"][3:4]]))
        assert done[4] == 1 and cnt[4] == K_DIRECT and bool((out["run"][4] == 0).all())              # env 4: its K-th episode
        assert torch.equal(out["records"][4, 0], before["records"][4, 0]) and not torch.equal(out["records"][4, 1], before["records"][4, 1])
    return out


# ------------------------------------------------------------------------------------------- 3. the Evaluator's routes
@contextlib.contextmanager
def eval_epilogue(on: bool):
    prev = acting._EVAL_EPILOGUE
    acting._EVAL_EPILOGUE = on
    try:
        yield
    finally:
        acting._EVAL_EPILOGUE = prev


def policy_fn(base, dev, noise=None):
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,), decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    fn = ppo_networks.make_inference_fn(nets)
    # (one counter for every policy made from the function, as train() hands the evaluator's policies theirs)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    return (functools.partial(fn, noise=noise, seed=9, counter=counter) if noise else fn), (norm, flat)


ROUTES = {"generic": dict(fused=False), "eager": dict(fused=True, graphed=False), "graphed": dict(fused=True, graphed=True)}


def evaluator_case(make_base, dev, route, *, K=1, mode="first_state", episode_length=6, ranges=None, graph_steps=20, noise=None,
                   runs=1, hook=None):
    """`runs` evaluations of acting.Evaluator on wrap(make_base()) by one route: (metrics dict of the last, records,
    eval_metrics tensors, per-env counts after each step of the last unroll or None)."""
    base = make_base()
    env = wrap(base, episode_length=episode_length, auto_reset=mode, auto_reset_seed=17, domain_ranges=ranges)
    fn, params = policy_fn(env.unwrapped, dev, noise)
    torch.manual_seed(123)
    ev = acting.Evaluator(env, fn, num_eval_envs=base.num_envs, episode_length=episode_length, action_repeat=1,
                          key=torch.Generator().manual_seed(11), episodes_per_env=K, graph_steps=graph_steps, **ROUTES[route])
    if hook is not None:
        hook(ev._env.unwrapped)
    for _ in range(runs):
        metrics = ev.run_evaluation(params, {})
    assert (ev._graph is not None) == (route == "graphed") and ev._fused == (route != "generic")
    return metrics, ev.records, ev


def assert_same_evaluation(a, b, timing=("eval/walltime", "eval/epoch_eval_time", "eval/sps")):
    (ma, ra, _), (mb, rb, _) = a, b
    assert sorted(ma) == sorted(mb)
    for k in ma:
        if k not in timing:
            assert np.array_equal(bits(np.asarray(ma[k])), bits(np.asarray(mb[k]))), k
    assert ra.shape == rb.shape and ra.dtype == rb.dtype and np.array_equal(bits(ra), bits(rb))


def eval_metrics_of(ev):
    em = ev.state.info["eval_metrics"]
    out = {"m." + k: v.cpu().numpy() for k, v in em.episode_metrics.items()}
    out.update(steps=em.episode_steps.cpu().numpy(), active=em.active_episodes.cpu().numpy())
    return out


def unroll_states(make_base, dev, *, K, mode, episode_length, T, fused, ranges=None, seed=17):
    """EvalWrapper(wrap(base)) stepped T times through acting.evaluate_unroll one step at a time: the state's info and
    done / count after every step (CPU) -- for the checks that need to know WHEN an episode ended."""
    base = make_base()
    env = EvalWrapper(wrap(base, episode_length=episode_length, auto_reset=mode, auto_reset_seed=seed, domain_ranges=ranges), K)
    fn, params = policy_fn(env.unwrapped, dev)
    policy = fn(params)
    torch.manual_seed(123)
    key = torch.Generator().manual_seed(11)
    st = env.reset(key)
    dones, counts = [], []
    for _ in range(T):
        st = acting.evaluate_unroll(env, st, policy, key, 1, fused=fused)
        dones.append(st.done.cpu().clone())
        counts.append(st.info["eval_count"].cpu().clone())
    return env, st, torch.stack(dones), torch.stack(counts)


def check_fresh_records(make_base, dev, fused, K=3, episode_length=4, T=12):
    """4.: under the fresh auto-reset every record after an env's first carries the start frame and clip that
    philox.reset_draws gives for that env at the step of the reset that began it, and its length is the distance between
    its two resets."""
    env, st, dones, counts = unroll_states(make_base, dev, K=K, mode="fresh", episode_length=episode_length, T=T, fused=fused)
    base, ar = env.unwrapped, env.env
    rec, count = st.info["eval_records"].cpu(), st.info["eval_count"].cpu()
    B, nq = base.num_envs, int(base.dims.nq)
    checked = 0
    for e in range(B):
        ends = [t for t in range(T) if dones[t, e] != 0][:K]  # the reset counter starts at 0 and advances one per step
        assert int(count[e]) == len(ends)
        for c, t_end in enumerate(ends):
            t_begin = ends[c - 1] if c else -1
            assert rec[e, c, 2] == t_end - t_begin
            if c:
                sf, clip, _ = philox.reset_draws(ar.seed, t_begin, torch.tensor([e + ar.env_offset]), nq, base._start_hi(),
                                                 base._num_clips, base._reset_noise_scale)
                assert rec[e, c, 0] == float(sf[0]) and rec[e, c, 1] == float(clip[0]), (e, c)
                checked += 1
    assert checked >= B  # later episodes did occur
    return rec


# ------------------------------------------------------------------------------------------------------ 5. the validation
DEFAULT_EVAL_KEYS = {"eval/walltime", "eval/avg_episode_length", "eval/epoch_eval_time", "eval/sps"} | \
    {f"eval/episode_{n}{s}" for n in ("rcom", "rvel", "rtrunk", "rquat", "ract", "rapp", "termination_error", "reward")
     for s in ("", "_std")}


def check_validation(base):
    """Every malformed scoring descriptor fails with VNL_ERR_ARG and the field's name, on both entries, and nothing runs (the
    state and the scoring buffers keep their bits); vnl_env_step_post without a scoring descriptor is what it was."""
    B, dev = base.num_envs, base.device
    L = base._L
    st = base.reset(torch.Generator().manual_seed(0))
    p = base._ptrs(st)
    raw = st.info["_raw"]
    action = torch.zeros(B, int(base.dims.nu), device=dev)
    steps, trunc = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    own = {"run": torch.full((B, 8), 3.0, device=dev), "count": torch.zeros(B, dtype=torch.int32, device=dev),
           "records": torch.full((B, 2, W), SENTINEL, device=dev), "steps": steps, "truncation": trunc}
    snap = lambda: {**PE.state_tensors(st), **{k: v.cpu().clone() for k, v in own.items()}}  # noqa: E731
    before = snap()
    post = _lib.PostDesc()
    post.done, post.steps, post.truncation, post.reward = _ptr(raw["done"]), _ptr(steps), _ptr(trunc), _ptr(raw["reward"])
    post.episode_length, post.action_repeat, post.num_ops = 4, 1, 0

    def good():
        e = _lib.EvalDesc()
        e.done, e.steps, e.truncation, e.reward, e.metrics = (_ptr(raw["done"]), _ptr(steps), _ptr(trunc), _ptr(raw["reward"]),
                                                              _ptr(raw["metrics"]))
        e.cur_frame, e.sub_clip_frame, e.clip_id = _ptr(raw["cur_frame"]), _ptr(raw["sub_clip_frame"]), _ptr(raw["clip_id"])
        e.run, e.count, e.records, e.episodes_per_env = _ptr(own["run"]), _ptr(own["count"]), _ptr(own["records"]), 2
        return e

    def both(e, word):
        ref = None if e is None else C.byref(e)
        for rc in (L.vnl_rollout_eval(ref, B, PE._stream(dev)),
                   L.vnl_env_step_post_eval(base._env_h, action.data_ptr(), C.byref(p), C.byref(post), ref, PE._stream(dev))):
            assert rc == -1 and word in L.vnl_last_error(), (word, rc, L.vnl_last_error())

    both(None, b"desc")
    for field in ("done", "steps", "reward", "metrics", "run", "count", "records"):
        e = good()
        setattr(e, field, None)
        both(e, field.encode())
    for k in (0, -3):
        e = good()
        e.episodes_per_env = k
        both(e, b"episodes_per_env")
    for field in ("cur_frame", "sub_clip_frame", "clip_id"):  # one missing, then only one given
        e = good()
        setattr(e, field, None)
        both(e, b"cur_frame, sub_clip_frame and clip_id")
        e = good()
        for other in {"cur_frame", "sub_clip_frame", "clip_id"} - {field}:
            setattr(e, other, None)
        both(e, b"cur_frame, sub_clip_frame and clip_id")
    # the post descriptor keeps its own check and messages on the fused entry
    bad = _lib.PostDesc()
    e = good()
    assert L.vnl_env_step_post_eval(base._env_h, action.data_ptr(), C.byref(p), C.byref(bad), C.byref(e), PE._stream(dev)) == -1
    msg = L.vnl_last_error()
    assert L.vnl_rollout_post(C.byref(bad), B, PE._stream(dev)) == -1 and L.vnl_last_error() == msg and b"null" in msg
    assert L.vnl_env_step_post_eval(None, action.data_ptr(), C.byref(p), C.byref(post), C.byref(e), PE._stream(dev)) == -1
    assert L.vnl_rollout_eval(C.byref(e), 0, PE._stream(dev)) == -1
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    PE.assert_same(snap(), before)  # nothing ran
    # .. and vnl_env_step_post, given no scoring descriptor, is the step and the post-processing alone
    _lib.check(L, L.vnl_env_step_post(base._env_h, action.data_ptr(), C.byref(p), C.byref(post), PE._stream(dev)))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    after = snap()
    for k in ("run", "count", "records"):
        assert torch.equal(after[k], before[k]), k
    assert bool((after["steps"] == 1).all()) and not torch.equal(after["ps.qpos"], before["ps.qpos"])
