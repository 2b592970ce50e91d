"""Shared by tests/test_rollout_record.py (host build) and tests/test_gpu_rollout_record.py (device): recorded rollouts
(include/vnl.h vnl_record_desc) -- vnl_env_record against a NumPy restatement on synthetic buffers, its validation,
acting.RolloutRecorder through the evaluation routes against a plain Python loop that clones the same tensors, the replay of
recorded latents, and Evaluator / train with a recorder.  Every comparison is of bits."""
import contextlib
import ctypes as C
import dataclasses
import functools

import numpy as np
import torch

import helpers as H
import post_epilogue_cases as PE
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import EvalWrapper, wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

SENTINEL = np.float32(-77.0)
NAN_WORD = 0x7FC00000
_ptr = PE._ptr


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def two_clips():
    """The golden clip twice, the second moved by 0.01 along x: the clip an env tracks shows in its reference pose."""
    c = H.reference_clip()
    moved = dataclasses.replace(c, position=c.position + np.array([0.01, 0.0, 0.0], dtype=c.position.dtype))
    return type(c).stack([c, moved])


# ---------------------------------------------------------------------------------------------- 1. the standalone kernel
T_SYN = 6
# column kinds: f = float32 words of any bit pattern (NaN payloads among them), i = int32, n = NULL (the NaN word)
LAYOUTS = {
    "one": dict(ref=False, cols=((1, "i"),)),                                                    # a row of one word
    "straddle": dict(ref=False, cols=((1, "i"), (63, "f"), (64, "n"), (65, "f"), (130, "f"))),   # 323 words
    "pose": dict(ref=True, cols=()),                                                             # the reference pose alone
    "pose+cols": dict(ref=True, cols=((63, "f"), (1, "n"), (65, "i"), (130, "f"))),              # nq + 259 words
}


def synthetic(base, layout, seed):
    """T_SYN steps of inputs for the envs of `base` (two clips), and recorders that watch them in a permuted order with one
    env twice, one index -1 and one index num_envs."""
    B, Tc = base.num_envs, base._T
    rng = np.random.default_rng(seed)
    lay = LAYOUTS[layout]
    cols = []
    for w, kind in lay["cols"]:
        if kind == "n":
            cols.append(None)
            continue
        a = rng.integers(0, 2 ** 32, (T_SYN, B, w), dtype=np.uint64).astype(np.uint32)
        if kind == "f":  # NaN payloads, quiet and signalling, both signs
            a[:, :, 0] = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FC00000], np.uint32)[rng.integers(0, 4, (T_SYN, B))]
        cols.append(a)
    done = (rng.random((T_SYN, B)) < 0.25).astype(np.float32)
    done[:, 0] = 0
    if B > 1:
        done[0, 1] = 1
    frame = rng.integers(0, Tc, (T_SYN, B)).astype(np.int32)
    special = np.array([-3, 0, Tc - 1, Tc + 5], np.int32)
    pick = rng.integers(0, 8, (T_SYN, B))
    frame = np.where(pick < 4, special[pick % 4], frame).astype(np.int32)
    frame[0, :min(B, 4)] = special[:min(B, 4)]  # each of them occurs
    clip = rng.integers(0, 2, (T_SYN, B)).astype(np.int32)
    perm = rng.permutation(B)
    idx = np.concatenate([perm, [perm[0], -1, B]]).astype(np.int32)
    idx = idx[rng.permutation(len(idx))]
    return dict(cols=cols, kinds=[k for _, k in lay["cols"]], widths=[w for w, _ in lay["cols"]], ref=lay["ref"], done=done,
                frame=frame, clip=clip, env_index=idx)


def clip_pose_words(base):
    c = base._clip
    return np.ascontiguousarray(np.concatenate([c["position"], c["quaternion"], c["joints"]], axis=-1)).view(np.uint32)


def restatement(base, inp, capacity, stop_at_done, use_index=True, use_done=True):
    """include/vnl.h above vnl_record_desc, recorder by recorder and step by step, on 32-bit words"""
    B, nq, Tc = base.num_envs, int(base.dims.nq), base._T
    pose = clip_pose_words(base)
    idx = inp["env_index"] if use_index else np.arange(B, dtype=np.int32)
    R = len(idx)
    W = (nq if inp["ref"] else 0) + sum(inp["widths"])
    rows = np.full((R, capacity, W), SENTINEL, np.float32).view(np.uint32)
    count, open_ = np.zeros(R, np.int32), np.ones(R, np.int32)
    for t in range(T_SYN):
        for r in range(R):
            e = int(idx[r])
            if e < 0 or e >= B or open_[r] == 0 or count[r] >= capacity:
                continue
            parts = []
            if inp["ref"]:
                parts.append(pose[inp["clip"][t, e], min(max(int(inp["frame"][t, e]), 0), Tc - 1)])
            for a, w in zip(inp["cols"], inp["widths"]):
                parts.append(np.full(w, NAN_WORD, np.uint32) if a is None else a[t, e])
            rows[r, count[r]] = np.concatenate(parts) if parts else rows[r, count[r]]
            count[r] += 1
            if stop_at_done and use_done and inp["done"][t, e] != 0:
                open_[r] = 0
    return dict(rows=rows, count=count, open=open_)


def run_standalone(base, inp, capacity, stop_at_done, use_index=True, use_done=True):
    dev, L, B, nq = base.device, base._L, base.num_envs, int(base.dims.nq)
    idx = torch.from_numpy(inp["env_index"]).to(dev) if use_index else None
    R = len(inp["env_index"]) if use_index else B
    W = (nq if inp["ref"] else 0) + sum(inp["widths"])
    d_cols = [None if a is None else torch.from_numpy(a.view(np.int32 if k == "i" else np.float32)).to(dev)
              for a, k in zip(inp["cols"], inp["kinds"])]
    done, frame, clip = (torch.from_numpy(inp[k]).to(dev) for k in ("done", "frame", "clip"))
    rows = torch.full((R, capacity, W), float(SENTINEL), device=dev)
    count, open_ = torch.zeros(R, dtype=torch.int32, device=dev), torch.ones(R, dtype=torch.int32, device=dev)
    for t in range(T_SYN):
        d = _lib.RecordDesc()
        d.env_index, d.done = _ptr(idx), _ptr(done[t] if use_done else None)
        if inp["ref"]:
            d.ref_frame, d.ref_clip = _ptr(frame[t]), _ptr(clip[t])
        d.count, d.open, d.rows = _ptr(count), _ptr(open_), _ptr(rows)
        d.num_rec, d.capacity, d.row_width, d.stop_at_done, d.num_cols = R, capacity, W, int(stop_at_done), len(d_cols)
        for o, a, w in zip(d.cols, d_cols, inp["widths"]):
            o.src, o.width = _ptr(a[t] if a is not None else None), w
        _lib.check(L, L.vnl_env_record(base._env_h, C.byref(d), PE._stream(dev)))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return dict(rows=rows.cpu().numpy().view(np.uint32), count=count.cpu().numpy(), open=open_.cpu().numpy())


def check_standalone(base):
    B = base.num_envs
    for layout in LAYOUTS:
        inp = synthetic(base, layout, seed=B + len(layout))
        for capacity, stop, use_index, use_done in ((1, True, True, True), (4, True, True, True), (4, False, True, True),
                                                    (4, True, False, True), (4, True, True, False)):
            want = restatement(base, inp, capacity, stop, use_index, use_done)
            got = run_standalone(base, inp, capacity, stop, use_index, use_done)
            for k in want:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (layout, k)
                assert np.array_equal(got[k], want[k]), (layout, capacity, stop, use_index, use_done, k)
            beyond = np.arange(capacity)[None, :] >= got["count"][:, None]
            assert np.all(got["rows"].view(np.float32)[beyond] == SENTINEL)  # rows at or beyond count are never touched
            if use_index:  # the two bad indices record nothing; the env watched twice gives two equal traces
                idx = inp["env_index"]
                assert np.all(got["count"][(idx < 0) | (idx >= B)] == 0) and np.all(got["open"][(idx < 0) | (idx >= B)] == 1)
                twice = np.flatnonzero(idx == np.bincount(idx[(idx >= 0) & (idx < B)]).argmax())
                assert len(twice) == 2 and np.array_equal(got["rows"][twice[0]], got["rows"][twice[1]])
            assert got["count"].max() == capacity  # the cursor stops at the capacity
            if stop and use_done and capacity == 4 and B > 1:
                assert (got["open"] == 0).any() and ((got["open"] == 0) & (got["count"] < capacity)).any()


# ------------------------------------------------------------------------------------------------------ 2. the validation
def check_validation(base):
    """Every malformed descriptor fails with VNL_ERR_ARG and the field's name, and nothing is written."""
    dev, L, B, nq = base.device, base._L, base.num_envs, int(base.dims.nq)
    src = torch.arange(B * 3, dtype=torch.float32, device=dev).reshape(B, 3)
    frame, clip = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    own = {"rows": torch.full((B, 2, nq + 4), float(SENTINEL), device=dev), "count": torch.zeros(B, dtype=torch.int32, device=dev),
           "open": torch.ones(B, dtype=torch.int32, device=dev)}
    before = {k: v.cpu().clone() for k, v in own.items()}

    def good():
        d = _lib.RecordDesc()
        d.ref_frame, d.ref_clip = _ptr(frame), _ptr(clip)
        d.count, d.open, d.rows = _ptr(own["count"]), _ptr(own["open"]), _ptr(own["rows"])
        d.num_rec, d.capacity, d.row_width, d.stop_at_done, d.num_cols = B, 2, nq + 4, 1, 2
        d.cols[0].src, d.cols[0].width = _ptr(src), 3
        d.cols[1].src, d.cols[1].width = None, 1
        return d

    def bad(d, word, env=True):
        rc = L.vnl_env_record(base._env_h if env else None, None if d is None else C.byref(d), PE._stream(dev))
        assert rc == -1 and word in L.vnl_last_error(), (word, rc, L.vnl_last_error())

    bad(None, b"desc")
    bad(good(), b"env", env=False)
    for field in ("rows", "count", "open"):
        d = good()
        setattr(d, field, None)
        bad(d, field.encode())
    for field in ("num_rec", "capacity"):
        for v in (0, -2):
            d = good()
            setattr(d, field, v)
            bad(d, field.encode())
    for v in (-1, 17):
        d = good()
        d.num_cols = v
        bad(d, b"num_cols")
    for v in (0, -5):
        d = good()
        d.cols[1].width = v
        bad(d, b"width")
    for field in ("ref_frame", "ref_clip"):
        d = good()
        setattr(d, field, None)
        bad(d, b"ref_frame and ref_clip")
    for v in (nq + 3, nq + 5, 4):
        d = good()
        d.row_width = v
        bad(d, b"row_width")
    d = good()  # without the pose the row is the columns alone: nq + 4 is then wrong, 4 right
    d.ref_frame = d.ref_clip = None
    bad(d, b"row_width")
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    PE.assert_same({k: v.cpu() for k, v in own.items()}, before)  # nothing ran
    _lib.check(L, L.vnl_env_record(base._env_h, C.byref(good()), PE._stream(dev)))  # .. and the good one does
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert bool((own["count"] == 1).all()) and bool((own["rows"][:, 1] == float(SENTINEL)).all())
    assert torch.equal(own["rows"][:, 0, nq:nq + 3].cpu(), src.cpu()) and bool(own["rows"][:, 0, nq + 3].isnan().all())


# ------------------------------------------------------------------------------------- 3. RolloutRecorder on the rodent
B_ROD, T_ROD, EPISODE = 8, 12, 5
FALLING = dict(healthy_z_range=(0.0, 0.5))  # tests/test_eval_epilogue.py: envs fall out of the healthy range on their own


@contextlib.contextmanager
def record_kernel(on: bool):
    prev = acting._RECORD_KERNEL
    acting._RECORD_KERNEL = on
    try:
        yield
    finally:
        acting._RECORD_KERNEL = prev


def networks(base):
    return ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,), decoder_layer_sizes=(32,))


def make_policy(base, dev, kind, latent="prior"):
    """-> (policy, extra columns): the device-noise acting policy, or the decoder policy with its `latent_out`"""
    nets = networks(base)
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    if kind == "full":
        return ppo_networks.make_inference_fn(nets)((norm, flat), noise="device", seed=9), {}
    z = torch.zeros(base.num_envs, 16, device=dev)
    return ppo_networks.make_decoder_inference_fn(nets)((norm, flat), latent=latent, seed=9, latent_out=z), {"latent": z}


STATE_COLUMNS = ("cur_frame", "clip_id", "steps", "done", "reward", "termination_error", "metrics", "qpos", "qvel")


def clone_row(st, action, pex, extra):
    raw, ps = st.info["_raw"], st.pipeline_state
    src = dict(cur_frame=raw["cur_frame"], clip_id=raw["clip_id"], steps=st.info["steps"], done=st.done, reward=st.reward,
               termination_error=raw["termination_error"], metrics=raw["metrics"], qpos=ps.raw("qpos"), qvel=ps.raw("qvel"),
               action=action, **{k: (pex or {}).get(k) for k in ("logits", "log_prob", "rand_log_prob")}, **extra)
    return {k: None if v is None else v.detach().cpu().clone().reshape(v.shape[0], -1).numpy() for k, v in src.items()}


def clone_loop(make_base, dev, mode, kind, T=T_ROD):
    """The plain loop a user writes today: the wrappers in torch ops, every tensor cloned after every step (under the fresh
    auto-reset through the wrapper's hook in front of the reset) -> list of T + 1 rows {column: (B, w) array or None}"""
    base = make_base()
    env = wrap(base, episode_length=EPISODE, auto_reset=mode, auto_reset_seed=17)
    policy, extra = make_policy(base, dev, kind)
    st = env.reset(torch.Generator().manual_seed(11))
    rows = [clone_row(st, None, None, {k: None for k in extra})]
    for _ in range(T):
        a, pex = policy(st.info["traj"], st.obs, None)
        if mode == "fresh":
            env.before_reset = lambda s, a=a, pex=pex: rows.append(clone_row(s, a, pex, extra))
        st = env.step(st, a)
        env.before_reset = None
        if mode != "fresh":
            rows.append(clone_row(st, a, pex, extra))
    return rows, base


def recorded_case(make_base, dev, mode, kind, route, T=T_ROD, stop_at_done=False, env_index=None, kernel=True):
    """The same steps through acting.evaluate_unroll / GraphedEval with a RolloutRecorder -> (recorder, RecordedRollout)"""
    base = make_base()
    env = EvalWrapper(wrap(base, episode_length=EPISODE, auto_reset=mode, auto_reset_seed=17))
    policy, extra = make_policy(base, dev, kind)
    with record_kernel(kernel):
        rec = acting.RolloutRecorder(env, **(dict(env_index=env_index) if env_index is not None else dict(num_record=base.num_envs)),
                                     capacity=T + 1, stop_at_done=stop_at_done, extra=extra)
        st = env.reset(torch.Generator().manual_seed(11))
        rec.record(st)
        if route == "graphed":  # 12 steps: two replays of 5 and an eager tail of 2
            g = acting.GraphedEval(env, st, policy, None, T, graph_steps=5, recorder=rec)
            assert (g.replays, g.tail) == (T // 5, T % 5)
            g()
        else:
            acting.evaluate_unroll(env, st, policy, None, T, fused=(route == "eager"), recorder=rec)
        return rec, rec.result()


def check_against_clone_loop(rows, base, out, stop_at_done=False, env_index=None):
    """`out` (a RecordedRollout) holds, per recorder, the cloned rows of its env: all of them, or up to its first done row"""
    B, cap = base.num_envs, len(rows)
    idx = np.arange(B) if env_index is None else np.asarray(env_index)
    pose = clip_pose_words(base)
    assert np.array_equal(out.env_index, idx)
    for r, e in enumerate(idx):
        if e < 0 or e >= B:
            assert out.length[r] == 0
            continue
        dones = [k for k in range(1, cap) if rows[k]["done"][e, 0] != 0]
        n = (dones[0] + 1) if (stop_at_done and dones) else cap
        assert out.length[r] == n, (r, e, out.length[r], n)
        for k in range(n):
            for name, col in out.columns.items():
                want = rows[k][name]
                got = col[r, k]
                if want is None:
                    assert np.all(got.view(np.uint32) == NAN_WORD), (name, k)
                else:
                    assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want[e])), (r, e, k, name)
            f = min(max(int(rows[k]["cur_frame"][e, 0]), 0), base._T - 1)
            assert np.array_equal(out.ref_qpos[r, k].view(np.uint32), pose[int(rows[k]["clip_id"][e, 0]), f])
        for name, col in out.columns.items():  # beyond the length: zeroed
            assert not col[r, n:].any()
    assert out.render_qpos.shape == out.qpos.shape[:2] + (2 * out.qpos.shape[2],)
    assert np.array_equal(bits(out.render_qpos[..., :out.qpos.shape[2]]), bits(out.ref_qpos))


def check_terminal_rows(out, mode):
    """The stated consequences of where the row is written: under the fresh auto-reset the done row is the true terminal state,
    from the first state it carries the restored first state beside the terminal step's reward, done and metrics."""
    seen = 0
    for r in range(len(out.length)):
        for k in range(1, out.length[r]):
            if out.done[r, k, 0] == 0:
                continue
            seen += 1
            assert out.steps[r, k, 0] >= 1 and not np.array_equal(out.metrics[r, k], out.metrics[r, 0])
            same_first = np.array_equal(bits(out.qpos[r, k]), bits(out.qpos[r, 0])) and \
                np.array_equal(bits(out.qvel[r, k]), bits(out.qvel[r, 0]))
            assert same_first == (mode == "first_state"), (mode, r, k)
            if mode == "fresh" and k + 1 < out.length[r]:  # the row after it belongs to the new episode
                assert out.steps[r, k + 1, 0] == 1
    assert seen >= len(out.length)  # episodes did end


def same_recorder(a, b):
    for k in ("rows", "count", "open"):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), k


# ------------------------------------------------------------------------------------------------------ 4. latent replay
def check_latent_replay(make_base, dev, T=7):
    """z recorded under the prior-mode decoder policy, then fed back step by step through `latent=` from the same reset, seed
    and counter: the same actions and the same qpos rows."""
    _, first = recorded_case(make_base, dev, "first_state", "decoder", "eager", T=T)
    base = make_base()
    env = EvalWrapper(wrap(base, episode_length=EPISODE, auto_reset="first_state", auto_reset_seed=17))
    z = torch.zeros(base.num_envs, 16, device=dev)
    policy, _ = make_policy(base, dev, "decoder", latent=z)
    rec = acting.RolloutRecorder(env, num_record=base.num_envs, capacity=T + 1, stop_at_done=False)
    st = env.reset(torch.Generator().manual_seed(11))
    rec.record(st)
    for t in range(T):
        z.copy_(torch.from_numpy(first.latent[:, t + 1]).to(dev))  # the z that chose action t is on row t + 1
        st = acting.evaluate_unroll(env, st, policy, None, 1, fused=True, recorder=rec)
    again = rec.result()
    assert np.all(again.length == T + 1) and np.all(first.length == T + 1)
    for name in ("action", "qpos", "qvel", "logits", "log_prob", "reward", "done"):
        assert np.array_equal(bits(getattr(again, name)), bits(getattr(first, name))), name
    assert not np.isnan(first.latent[:, 1:]).any() and np.isnan(first.latent[:, 0]).all()
    assert len({first.latent[0, t].tobytes() for t in range(1, T + 1)}) == T  # a new draw every step


# ------------------------------------------------------------------------------------------- 5. Evaluator and train()
def evaluator_case(make_base, dev, route, record_envs, mode="first_state", **kw):
    base = make_base()
    env = wrap(base, episode_length=EPISODE, auto_reset=mode, auto_reset_seed=17)
    nets = networks(base)
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    fn = functools.partial(ppo_networks.make_inference_fn(nets), noise="device", seed=9, counter=counter)
    routes = {"generic": dict(fused=False), "eager": dict(fused=True, graphed=False), "graphed": dict(fused=True, graphed=True)}
    ev = acting.Evaluator(env, fn, num_eval_envs=base.num_envs, episode_length=EPISODE, action_repeat=1,
                          key=torch.Generator().manual_seed(11), record_envs=record_envs, **routes[route], **kw)
    ev.run_evaluation((norm, flat), {})
    return ev


def check_evaluator(make_base, dev, route, tmp_path, **kw):
    plain = evaluator_case(make_base, dev, route, 0, **kw)
    ev = evaluator_case(make_base, dev, route, 2, **kw)
    assert plain.recorded is None and plain._recorder is None
    for k in ("eval_records", "eval_count", "eval_run"):  # the evaluation itself is what it is without a recorder
        a, b = plain.state.info[k].cpu().numpy(), ev.state.info[k].cpu().numpy()
        assert np.array_equal(bits(a), bits(b)), k
    assert np.array_equal(bits(plain.records), bits(ev.records))
    out = ev.recorded
    first = ev.state.info["eval_records"].cpu().numpy()[:2, 0]  # the first episode of envs 0 and 1: steps in column 2
    assert np.array_equal(out.length, first[:, 2].astype(np.int64) + 1)  # the reset row, then one row per step to the done row
    for r in range(2):
        n = out.length[r]
        assert out.done[r, n - 1, 0] == 1 and not out.done[r, :n - 1].any()
        assert np.isnan(out.log_prob[r, 0, 0]) and not np.isnan(out.log_prob[r, 1:n]).any()
        # the scored episode's reward is the sum of the recorded steps' (float32 adds in step order)
        total = np.float32(0)
        for k in range(1, n):
            total = np.float32(total + out.reward[r, k, 0])
        assert total == first[r, 11]
    path = tmp_path / "rollout.npz"
    out.save(path)
    back = acting.RecordedRollout.load(path)
    assert sorted(back.columns) == sorted(out.columns) and np.array_equal(back.length, out.length)
    for k in out.columns:
        assert back.columns[k].dtype == out.columns[k].dtype and np.array_equal(bits(back.columns[k]), bits(out.columns[k])), k
    assert np.array_equal(bits(back.render_qpos), bits(out.render_qpos)) and np.array_equal(back.env_index, out.env_index)
    return ev
