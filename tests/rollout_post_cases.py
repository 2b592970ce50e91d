"""vnl_rollout_post against a torch restatement of include/vnl.h's description, exact equality, shared by
tests/test_gpu_rollout_post.py (the device) and tests/test_rollout_post.py (the host simulation): `check` takes the library
and the device."""
import ctypes as C

import torch

from vnl_brax_imitation_amd import _lib

EPISODE_LENGTH, ACTION_REPEAT = 7, 1
# (width, dst: "src" = in place | "own" = a buffer of its own | None, first state?, log row?)
OPS = [(1, "src", True, True), (3, "src", True, False), (73, None, False, True), (232, "src", True, True),
       (795, "src", False, True), (795, "own", True, False), (73, "src", True, True), (3, "own", False, True),
       (1, None, True, True)]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _case(B, logs, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    env = torch.arange(B)
    c = {"done": (env % 3 == 1).float(),                       # finished and running envs mixed
         "prev_done": (env % 4 == 2).float(),                  # some start a new episode: their count restarts at 0
         "steps": (env % 5 + EPISODE_LENGTH - 3).float(),      # 4 .. 8: some cross episode_length = 7 with this step
         "truncation": r(B), "reward": r(B)}
    if logs:
        c.update(log_reward=r(B), log_discount=r(B), log_truncation=r(B))
    ops = []
    for k, (w, dst, first, log) in enumerate(OPS):
        src = r(B, w) if k else torch.randint(0, 1 << 30, (B, w), generator=g, dtype=torch.int32)  # (int32 rows move bit-exactly)
        ops.append({"src": src, "dst": None if dst is None else (src if dst == "src" else torch.full_like(src, 7)),
                    "first": (src + 1 if k else src // 2) if first else None, "log": torch.full_like(src, 9) if log else None})
    return c, ops


def _restate(c, ops):
    """include/vnl.h, vnl_rollout_post, in torch on copies: returns the buffers as the launch must leave them."""
    c = {k: v.clone() for k, v in c.items()}
    st = torch.where(c["prev_done"] != 0, torch.zeros_like(c["steps"]), c["steps"]) + ACTION_REPEAT
    over = st >= EPISODE_LENGTH
    trunc = torch.where(over, 1 - c["done"], torch.zeros_like(st))
    done = torch.where(over, torch.ones_like(st), c["done"])
    c.update(steps=st, prev_done=done, done=done, truncation=trunc)
    if "log_reward" in c:
        c.update(log_reward=c["reward"].clone(), log_discount=1 - done, log_truncation=trunc)
    out = []
    for o in ops:
        v = o["src"] if o["first"] is None else torch.where((done != 0)[:, None], o["first"], o["src"])
        out.append({"src": o["src"].clone() if o["dst"] is not o["src"] else v.clone(),
                    "dst": None if o["dst"] is None else v.clone(), "log": None if o["log"] is None else v.clone(),
                    "first": o["first"]})
    return c, out


def check(lib, dev, B, logs):
    c, ops = _case(B, logs, seed=B)
    want_c, want_ops = _restate(c, ops)
    assert 0 < int(want_c["done"].sum()) < B and (want_c["truncation"] != 0).any() and (want_c["steps"] == 1).any()
    dc = {k: v.to(dev) for k, v in c.items()}
    dops = []
    for o in ops:
        src = o["src"].to(dev)
        dops.append({"src": src, "dst": None if o["dst"] is None else (src if o["dst"] is o["src"] else o["dst"].to(dev)),
                     "first": None if o["first"] is None else o["first"].to(dev), "log": None if o["log"] is None else o["log"].to(dev)})
    d = _lib.PostDesc()
    for k in ("steps", "prev_done", "done", "truncation", "reward", "log_reward", "log_discount", "log_truncation"):
        setattr(d, k, _ptr(dc.get(k)))
    d.episode_length, d.action_repeat, d.num_ops = EPISODE_LENGTH, ACTION_REPEAT, len(dops)
    for k, o in enumerate(dops):
        d.ops[k].dst, d.ops[k].src, d.ops[k].first, d.ops[k].log = _ptr(o["dst"]), _ptr(o["src"]), _ptr(o["first"]), _ptr(o["log"])
        d.ops[k].width = o["src"].shape[1]
    cuda = torch.device(dev).type == "cuda"
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(dev)).cuda_stream) if cuda else C.c_void_p(0)
    _lib.check(lib, lib.vnl_rollout_post(C.byref(d), B, stream))
    if cuda:
        torch.cuda.synchronize()
    for k, v in want_c.items():
        assert torch.equal(dc[k].cpu(), v), k
    for k, (got, want) in enumerate(zip(dops, want_ops)):
        for f in ("src", "dst", "log", "first"):
            assert (got[f] is None) == (want[f] is None)
            if want[f] is not None:
                assert torch.equal(got[f].cpu(), want[f]), (k, f)
