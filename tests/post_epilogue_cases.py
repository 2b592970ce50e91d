"""Shared by tests/test_post_epilogue.py (host build) and tests/test_gpu_post_epilogue.py (device): the step kernel with the
rollout post-processing as its epilogue (vnl_env_step_post, acting._POST_EPILOGUE) against the two launches it replaces
(vnl_env_step, then vnl_rollout_post) -- every buffer a descriptor names, every Transition leaf and every carried state
tensor, bit for bit."""
import contextlib
import ctypes as C

import numpy as np
import torch

from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

EXTRA = ("truncation", "traj")
EPISODE_LENGTH = 4  # of the direct case below


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@contextlib.contextmanager
def post_epilogue(on: bool):
    prev = acting._POST_EPILOGUE
    acting._POST_EPILOGUE = on
    try:
        yield
    finally:
        acting._POST_EPILOGUE = prev


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else C.c_void_p(0)


def direct_case(base, fused: bool):
    """One call on a freshly reset state of `base` (at least 5 envs) in which all four decision branches occur: env 0
    terminates on its own (its root is lifted out of the healthy height range), env 1 reaches the episode length (truncation 1),
    env 2 comes with prev_done set (its count restarts), env 3 does nothing special.  Ops: dst == src with first (with and
    without a log row), dst null with log, a destination of its own, int32 rows, widths 1, 63, 64, 65 and 795.
    Returns {name: tensor on the CPU} of every buffer the descriptor names, the state's rows included."""
    B, dev = base.num_envs, base.device
    g = torch.Generator().manual_seed(3)
    sf = torch.randint(0, 100, (B,), generator=g, dtype=torch.int32)
    nq, nu = int(base.dims.nq), int(base.dims.nu)
    st = base.reset(start_frame=sf, noise=1e-3 * torch.randn(B, nq, generator=g))
    st.pipeline_state.raw("qpos")[0, 2] += 5.0
    action = (0.3 * torch.randn(B, nu, generator=g)).clamp(-1, 1).to(dev)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    env = torch.arange(B)
    c = {"steps": torch.where(env == 1, EPISODE_LENGTH - 1, env % 2).float().to(dev), "prev_done": (env == 2).float().to(dev),
         "truncation": r(B), "log_reward": r(B), "log_discount": r(B), "log_truncation": r(B)}
    raw, ps = st.info["_raw"], st.pipeline_state
    ops = []  # (dst, src, first, log)

    def op(src, dst, first, log):
        ops.append({"src": src, "dst": src if dst == "src" else (torch.full_like(src, 7) if dst == "own" else None),
                    "first": (src + 1 if src.dtype == torch.float32 else src + 5) if first else None,
                    "log": torch.full_like(src, 9) if log else None})

    op(ps.raw("qpos"), "src", True, False)                 # dst == src with first, no log
    op(raw["obs"], "src", True, True)                      # dst == src with first and log
    op(raw["traj"], None, False, True)                     # dst null with log
    op(raw["cur_frame"][:, None], "src", True, True)       # width 1, int32
    for w in (1, 63, 64, 65, 795):
        op(r(B, w), "own" if w != 64 else "src", w != 63, w != 65)
    d = _lib.PostDesc()
    for k in ("steps", "prev_done", "truncation", "log_reward", "log_discount", "log_truncation"):
        setattr(d, k, _ptr(c[k]))
    d.done, d.reward = _ptr(raw["done"]), _ptr(raw["reward"])
    d.episode_length, d.action_repeat, d.num_ops = EPISODE_LENGTH, 1, len(ops)
    for k, o in enumerate(ops):
        d.ops[k].dst, d.ops[k].src, d.ops[k].first, d.ops[k].log = _ptr(o["dst"]), _ptr(o["src"]), _ptr(o["first"]), _ptr(o["log"])
        d.ops[k].width = o["src"].shape[1]
    L, p = base._L, base._ptrs(st)
    if fused:
        _lib.check(L, L.vnl_env_step_post(base._env_h, action.data_ptr(), C.byref(p), C.byref(d), _stream(dev)))
    else:
        _lib.check(L, L.vnl_env_step(base._env_h, action.data_ptr(), C.byref(p), _stream(dev)))
        own_done = raw["done"].clone()
        _lib.check(L, L.vnl_rollout_post(C.byref(d), B, _stream(dev)))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    out = {k: v.cpu() for k, v in c.items()}
    out.update({"state." + n: ps.raw(n).cpu() for n in ps._FIELDS})
    out.update({"state." + k: v.cpu() for k, v in raw.items()})
    for k, o in enumerate(ops):
        out.update({f"op{k}.{f}": o[f].cpu() for f in ("src", "dst", "first", "log") if o[f] is not None})
    if not fused:  # the case is what it claims to be (judged on the two-launch form)
        own, done, tr = own_done.cpu(), out["state.done"], out["truncation"]
        assert own[0] == 1 and own[1] == 0 and own[3] == 0, own          # env 0 terminates on its own
        assert done[0] == 1 and tr[0] == 0                                 # .. and that is no truncation
        assert done[1] == 1 and tr[1] == 1 and out["steps"][1] == EPISODE_LENGTH  # env 1 reaches the episode length
        assert out["steps"][2] == 1                                        # env 2: prev_done restarted its count
        assert done[3] == 0 and tr[3] == 0 and out["steps"][3] == 2        # env 3: nothing special
    return out


def assert_same(a: dict, b: dict):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].numpy().view(np.uint8), b[k].numpy().view(np.uint8)), k  # the same BITS (NaN-proof)


def make_policy(base, dev, noise=None):
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
    norm = running_statistics.init_state(base.observation_size, device=dev)
    fn = ppo_networks.make_inference_fn(nets)
    return fn((norm, flat)) if noise is None else fn((norm, flat), noise=noise, seed=9)


def state_tensors(st):
    out = {"ps." + n: st.pipeline_state.raw(n) for n in st.pipeline_state._FIELDS}
    out.update(obs=st.obs, reward=st.reward, done=st.done)
    for k, v in st.info.items():
        if isinstance(v, torch.Tensor):
            out["info." + k] = v
        elif isinstance(v, dict):
            out.update({f"info.{k}.{k2}": v2 for k2, v2 in v.items() if isinstance(v2, torch.Tensor)})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def unroll_case(make_base, dev, epilogue: bool, *, T=3, episode_length=2, noise=None, mode="first_state", graphed=False,
                calls=1, hook=None):
    """`calls` unrolls of T steps on AutoReset(Episode(base)) with the switch set: [leaves of every call], carried state.
    `hook(base)` may wrap base.step before the unrolls (as bench.py does)."""
    base = make_base()
    kw = {} if mode == "first_state" else {"mode": mode, "seed": 17}
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1), **kw)
    policy = make_policy(base, dev, noise)
    torch.manual_seed(123)  # rand_log_prob's uniform draw comes from the global generator on HIP devices
    state = env.reset(torch.Generator().manual_seed(5))
    key = torch.Generator(device=dev).manual_seed(11)
    if hook is not None:
        hook(base)
    datas = []
    with post_epilogue(epilogue):
        g = acting.GraphedUnroll(env, state, policy, key, T, extra_fields=EXTRA) if graphed else None
        for _ in range(calls):
            state, data = g() if graphed else acting.generate_unroll(env, state, policy, key, T, extra_fields=EXTRA, fused=True)
            datas.append([x.detach().cpu().clone() for x in acting._leaves(data)])
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return datas, state_tensors(state)


def assert_unrolls_same(a, b):
    (da, sa), (db, sb) = a, b
    assert len(da) == len(db)
    for x_, y_ in zip(da, db):
        assert len(x_) == len(y_)
        for x, y in zip(x_, y_):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)
    assert_same(sa, sb)
