"""Checks of the domain redraw at fresh resets (vnl_env_set_domain_ranges, vnl_env_redraw_domain, the redraw inside
vnl_env_reset_done) shared by tests/test_domain_redraw.py (host builds) and tests/test_gpu_domain_redraw.py: the draw against
its restatement ppo_imitation/philox.py domain_draws, the redrawn tables against vnl_env_set_domain of the same values, the
fused redraw against the separate launch, sharding, degenerate and absent ranges, the argument checks, the wrapper paths.
Every comparison is of bits; every function takes a base env WITHOUT ranges (rodent: the specialised randomised kernels,
nv = 73 makes a second lane trip; ant: the generic ones, partial trips and a last Philox block used in part)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import domain_cases as D
import fresh_reset_cases as F
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper, wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics

TABLES = ("dom_mu", "dom_invw", "dom_gain", "dom_damp", "dom_arm")
FIELD_TABLE = {"cg_friction": "dom_mu", "act_gain": "dom_gain", "dof_damping": "dom_damp", "dof_armature": "dom_arm"}
STEP = F.STEP_BASE + F.STEP_OFFSET
ENV_OFFSET = 1000003


def ranges_for(sys, seed=0) -> dict:
    """Independent bounds per element on all four fields, lo < hi everywhere: multiples U[0.5, 0.9] and U[1.1, 1.6] of the
    compiled value, plus an absolute U[0.01, 0.02] / U[0.03, 0.05] for damping and armature (compiled 0 on the root's dofs)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, c in D.compiled(sys).items():
        a, b = c * rng.uniform(0.5, 0.9, c.size), c * rng.uniform(1.1, 1.6, c.size)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        if k in ("dof_damping", "dof_armature"):
            lo, hi = lo + rng.uniform(0.01, 0.02, c.size), hi + rng.uniform(0.03, 0.05, c.size)
        assert bool((lo < hi).all())
        out[k] = (lo, hi)
    return out


def half_mask(B: int) -> torch.Tensor:
    m = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.float32).repeat((B + 7) // 8)[:B]
    return m


def tables(env) -> dict:
    return {k: env.domain_table(k) for k in TABLES}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_tables(a: dict, b: dict, rows=None, keys=TABLES) -> None:
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(bits(x), bits(y)), k


def drawn(env, ranges, shared=(), step=STEP, env_offset=ENV_OFFSET, initial=False, seed=F.SEED) -> dict:
    """{field: float64 (B, n)} of philox.domain_draws for every env of the batch"""
    ids = torch.arange(env.num_envs) + env_offset
    return {k: philox.domain_draws(seed, step, ids, k, lo, hi, shared=k in shared, initial=initial) for k, (lo, hi) in ranges.items()}


def expected_tables(env, values: dict) -> dict:
    """the tables of float64 values: cast to the env's real type; dom_invw by the NumPy float64 formula of
    tests/test_domain_randomization.py::test_derived_inverse_weight_is_the_float64_formula"""
    m = env.sys
    out = {FIELD_TABLE[k]: v.to(env._dtype) for k, v in values.items()}
    if "cg_friction" in values:
        iw0 = np.asarray(m.body_invweight0, np.float64).reshape(-1)
        t = iw0[0] + iw0[2 * np.asarray(m.cg_bodyid)]
        mu = values["cg_friction"].numpy()
        out["dom_invw"] = torch.from_numpy((t + mu * mu * t) * 2 * mu * mu / float(m.scalars["impratio"])).to(env._dtype)
    return out


def redraw(env, mask=None, env_offset=ENV_OFFSET, initial=False) -> None:
    base = torch.tensor([F.STEP_BASE], dtype=torch.int64, device=env.device)
    env.redraw_domain(seed=F.SEED, step_base=base, step_offset=F.STEP_OFFSET, env_offset=env_offset, mask=mask, initial=initial)
    if env.device.type == "cuda":
        torch.cuda.synchronize(env.device)
    assert int(base) == F.STEP_BASE


def clear_ranges_keep_tables(env) -> None:
    """vnl_env_set_domain_ranges(null): the ranges go, the tables stay"""
    _lib.check(env._L, env._L.vnl_env_set_domain_ranges(env._env_h, None, env._stream()))
    env._domain_ranges = None


def uniform_priority(env):
    """a StartPriority-shaped object with the uniform table and zero counters"""
    ncell = env._num_clips * env._start_hi()
    cdf, _, _ = philox.start_priority_table(torch.zeros(ncell, dtype=torch.int64), torch.zeros(ncell, dtype=torch.int64))
    words = torch.from_numpy(cdf.numpy().astype(np.uint32).view(np.int32).copy()).to(env.device)
    z = lambda: torch.zeros(ncell, dtype=torch.int32, device=env.device)  # noqa: E731
    return types.SimpleNamespace(cdf=words, count_ended=z(), count_failed=z())


def reset_done(env, st, mask, env_offset=ENV_OFFSET, priority=None) -> None:
    base = torch.tensor([F.STEP_BASE], dtype=torch.int64, device=env.device)
    env.reset_done(st, mask.to(env.device), seed=F.SEED, step_base=base, step_offset=F.STEP_OFFSET, env_offset=env_offset,
                   priority=priority)
    if env.device.type == "cuda":
        torch.cuda.synchronize(env.device)


EVERY = lambda B: torch.ones(B, dtype=torch.bool)  # noqa: E731


# ---- case 1 ----------------------------------------------------------------------------------------------------------------
def check_draw_is_the_restatement(base) -> None:
    B, rg = base.num_envs, ranges_for(base.sys)
    mask = half_mask(B)
    m = mask.bool()
    env = base.with_domain_ranges(rg)
    assert set(env.domain_ranges) == set(rg) | {"shared"} and base.domain_ranges is None
    before = tables(env)
    same_tables(before, tables(base.with_domain(D.identity(base.sys, B))))  # allocated at the compiled values
    redraw(env, mask)
    after = tables(env)
    want = expected_tables(env, drawn(env, rg))
    same_tables(after, want, m)
    same_tables(after, before, ~m)
    assert not torch.equal(after["dom_arm"][m], before["dom_arm"][m])
    # one uniform per (env, episode) for the whole of a shared field
    shared = ("cg_friction", "dof_damping")
    env2 = base.with_domain_ranges(rg, shared=shared)
    assert env2.domain_ranges["shared"] == shared
    redraw(env2)
    vals = drawn(env2, rg, shared)
    same_tables(tables(env2), expected_tables(env2, vals))
    for k in shared:  # (through the restatement: every element of a row sits at the same fraction of its interval)
        lo, hi = (torch.from_numpy(x) for x in rg[k])
        u = (vals[k] - lo) / (hi - lo)
        assert float((u - u[:, :1]).abs().max()) < 1e-12 and float(u[:, 0].std()) > 0.05
    u = (vals["act_gain"] - torch.from_numpy(rg["act_gain"][0])) / torch.from_numpy(rg["act_gain"][1] - rg["act_gain"][0])
    assert float(u.std(dim=1).min()) > 0.05  # .. and an unshared one does not
    # the first episode's block range is its own
    env3 = base.with_domain_ranges(rg)
    redraw(env3, initial=True)
    first = tables(env3)
    same_tables(first, expected_tables(env3, drawn(env3, rg, initial=True)))
    for k in TABLES:
        assert not bool((bits(first[k]) == bits(want[k])).all(dim=1).any()), k


# ---- case 2 ----------------------------------------------------------------------------------------------------------------
def check_redraw_is_set_domain_of_the_same_values(base) -> None:
    B, rg = base.num_envs, ranges_for(base.sys, 1)
    env = base.with_domain_ranges(rg)
    redraw(env)
    env2 = base.with_domain({k: v for k, v in drawn(env, rg).items()})
    same_tables(tables(env), tables(env2))
    a, b = F.snapshot(F.stepped_state(env, 4)), F.snapshot(F.stepped_state(env2, 4))
    F.same_rows(a, b, EVERY(B), F.WRITTEN + F.KEPT)
    c = F.snapshot(F.stepped_state(base, 4))
    assert not torch.equal(a["qvel"], c["qvel"])  # the domain did change the dynamics


# ---- case 3 ----------------------------------------------------------------------------------------------------------------
def check_fused_is_separate(base, weighted: bool) -> None:
    B, rg = base.num_envs, ranges_for(base.sys, 2)
    mask = half_mask(B)
    out = []
    for fused in (True, False):
        env = base.with_domain_ranges(rg)
        st = F.stepped_state(env, 3)
        st.done.copy_(mask.to(device=env.device, dtype=st.done.dtype))
        prio = uniform_priority(env) if weighted else None
        sf0 = (st.info["cur_frame"] - st.info["sub_clip_frame"]).cpu()  # the finished episodes' start frames
        if not fused:
            redraw(env, mask)
            clear_ranges_keep_tables(env)
        reset_done(env, st, mask, priority=prio)
        out.append((F.snapshot(st), tables(env), prio))
    (s0, t0, p0), (s1, t1, p1) = out
    F.same_rows(s0, s1, EVERY(B), tuple(s0))
    same_tables(t0, t1)
    same_tables(t0, expected_tables(base.with_domain_ranges(rg), drawn(base, rg)), mask.bool())
    if weighted:
        assert torch.equal(p0.count_ended, p1.count_ended) and torch.equal(p0.count_failed, p1.count_failed)
        # counted from the FINISHED episode, whatever the redraw did (the ant starts at frame 0 only: others are out of range)
        assert int(p0.count_ended.sum()) == int(((sf0 >= 0) & (sf0 < base._start_hi()) & mask.bool()).sum())


# ---- case 4 ----------------------------------------------------------------------------------------------------------------
def check_sharding(make) -> None:
    whole = make(8)
    rg = ranges_for(whole.sys, 3)
    nq, nu = int(whole.dims.nq), whole.action_size
    g = torch.Generator().manual_seed(9)
    sf = torch.randint(0, max(whole._T - 10, 1), (8,), generator=g, dtype=torch.int32)
    nz = 1e-3 * torch.randn((8, nq), generator=g)
    clip = torch.randint(0, whole._num_clips, (8,), generator=g, dtype=torch.int32)
    act = 0.3 * torch.randn((2, 8, nu), generator=g)
    mask = half_mask(8)

    def run(env, sl, lo):
        env = env.with_domain_ranges(rg)
        redraw(env, env_offset=lo, initial=True)  # the first episode's domain, then two steps in it, then the fresh reset
        st = F.stepped_state(env, 0, clip[sl], sf[sl], nz[sl], act[:, sl])
        reset_done(env, st, mask[sl], env_offset=lo)
        return F.snapshot(st), tables(env)

    full, tab = run(whole, slice(0, 8), 0)
    for lo in (0, 4):
        sl = slice(lo, lo + 4)
        snap, t = run(make(4), sl, lo)
        F.same_rows({k: v[sl] for k, v in full.items()}, snap, EVERY(4), tuple(snap))
        same_tables({k: v[sl] for k, v in tab.items()}, t)


# ---- case 5 ----------------------------------------------------------------------------------------------------------------
def check_degenerate_and_absent_ranges(base) -> None:
    B = base.num_envs
    mask = half_mask(B)
    ident = D.identity(base.sys, B)
    plain = base.with_domain(ident)
    env = base.with_domain_ranges({k: (v, v) for k, v in D.compiled(base.sys).items()})
    snaps = []
    for e in (plain, env):
        st = F.stepped_state(e, 6)
        reset_done(e, st, mask)
        snaps.append(F.snapshot(st))
    F.same_rows(snaps[0], snaps[1], EVERY(B), tuple(snaps[0]))
    same_tables(tables(plain), tables(env))
    # a field without bounds is never written, even with with_domain values in it
    dom = D.random_domain(base.sys, B, 5)
    given = base.with_domain(dom)
    before = tables(given)
    only = given.with_domain_ranges({"act_gain": ranges_for(base.sys)["act_gain"]})
    same_tables(before, tables(only))  # the with_domain values are kept until the first redraw
    st = F.stepped_state(only, 7)
    reset_done(only, st, mask)
    after = tables(only)
    same_tables(before, after, keys=("dom_mu", "dom_invw", "dom_damp", "dom_arm"))
    same_tables(before, after, ~mask.bool(), keys=("dom_gain",))
    assert not bool((bits(before["dom_gain"]) == bits(after["dom_gain"]))[mask.bool()].any())
    # no ranges: a fresh reset leaves all five tables alone
    st = F.stepped_state(given, 7)
    reset_done(given, st, mask)
    same_tables(before, tables(given))


# ---- case 6 ----------------------------------------------------------------------------------------------------------------
def check_errors_launch_nothing(base) -> None:
    B, rg = base.num_envs, ranges_for(base.sys)
    env = base.with_domain_ranges(rg)
    redraw(env)
    st = F.stepped_state(env, 1)
    snap, tab = F.snapshot(st), tables(env)
    L, d = env._L, env.dims
    n = {"cg_friction": int(d.ngeom_collide), "act_gain": int(d.nu), "dof_damping": int(d.nv), "dof_armature": int(d.nv)}

    def c_call(f, lo, hi):
        """vnl_env_set_domain_ranges with field f's bounds alone (None: a null pointer)"""
        keep = [None if x is None else torch.as_tensor(x, dtype=torch.float64).to(env.device).contiguous() for x in (lo, hi)]
        desc = _lib.DomainRanges()
        desc.lo[f], desc.hi[f] = (None if t is None else t.data_ptr() for t in keep)
        return L.vnl_env_set_domain_ranges(env._env_h, C.byref(desc), env._stream())

    fr_lo, fr_hi = rg["cg_friction"]
    nan = np.full(n["act_gain"], np.nan)
    bad_c = [(0, fr_hi, fr_lo), (0, np.zeros_like(fr_lo), fr_hi), (2, np.full(n["dof_damping"], -0.1), np.ones(n["dof_damping"])),
             (3, np.full(n["dof_armature"], -1e-9), np.ones(n["dof_armature"])), (1, nan, nan), (1, rg["act_gain"][0], np.inf + nan),
             (1, rg["act_gain"][0], None), (2, None, rg["dof_damping"][1])]
    for f, lo, hi in bad_c:
        assert c_call(f, lo, hi) == -1, (f, lo, hi)
        assert philox.DOMAIN_FIELDS[f].encode() in L.vnl_last_error()  # the field's name
    assert L.vnl_env_set_domain_ranges(None, None, None) == -1
    bad_py = [{"cg_friction": (fr_hi, fr_lo)}, {"cg_friction": (0.0, 1.0)}, {"dof_damping": (-0.1, 1.0)},
              {"act_gain": (float("nan"), 1.0)}, {"act_gain": (1.0, float("inf"))}, {"dof_armature": (np.zeros(3), np.ones(3))},
              {"dof_armature": (np.zeros(n["dof_armature"]), np.ones(n["dof_armature"] + 1))}, {"dof_armature": 1.0},
              {"body_mass": (0.5, 1.0)}]
    for r in bad_py:
        with pytest.raises(ValueError):
            env.with_domain_ranges(r)
    with pytest.raises(ValueError, match="no range"):
        env.with_domain_ranges({"act_gain": (0.5, 1.0)}, shared=("cg_friction",))
    # redraw_domain without ranges, at both levels
    with pytest.raises(ValueError, match="no domain ranges"):
        base.redraw_domain(seed=1, step_base=0)
    step = torch.zeros(1, dtype=torch.int64, device=env.device)
    nz = _lib.ResetNoise(seed=1, step_base=step.data_ptr())
    given = base.with_domain(D.identity(base.sys, B))
    assert given._L.vnl_env_redraw_domain(given._env_h, None, C.byref(nz), 0, given._stream()) == -1
    for kw, initial in ((dict(step_base=None), 0), (dict(step_offset=-1), 0), (dict(env_offset=-1), 0), ({}, 2)):
        z = _lib.ResetNoise(seed=1, step_base=step.data_ptr())
        for k, v in kw.items():
            setattr(z, k, v)
        assert L.vnl_env_redraw_domain(env._env_h, None, C.byref(z), initial, env._stream()) == -1, kw
    assert L.vnl_env_redraw_domain(env._env_h, None, None, 0, env._stream()) == -1
    with pytest.raises(ValueError, match="auto_reset='fresh'"):
        wrap(base, episode_length=3, domain_ranges=rg)
    with pytest.raises(ValueError, match="auto_reset='fresh'"):
        wrap(base, episode_length=3, auto_reset="first_state", domain_ranges=rg)
    if env.device.type == "cuda":
        torch.cuda.synchronize(env.device)
    F.same_rows(snap, F.snapshot(st), EVERY(B), tuple(snap))
    same_tables(tab, tables(env))
    assert env.domain_ranges is not None
    redraw(env, initial=True)  # .. and the ranges are still the ones set: a valid call draws from them
    same_tables(tables(env), expected_tables(env, drawn(env, rg, initial=True)))
    w = wrap(base, episode_length=3, auto_reset="fresh", domain_ranges=rg, domain_shared=("act_gain",))
    assert w.mode == "fresh" and w.unwrapped.domain_ranges["shared"] == ("act_gain",)
    assert w.unwrapped.with_num_envs(2).domain_ranges["shared"] == ("act_gain",)


# ---- case 7 ----------------------------------------------------------------------------------------------------------------
def wrapper_paths(make, device, graphed: bool, seed=77):
    """Episodes of 3 steps ending on different steps, T = 7 then 3, as test_eager_wrapper_equals_fused_unroll_in_fresh_mode:
    eager wrapper == fused unroll (== one replay of GraphedUnroll per unroll length, on the device), tables included."""
    extra = ("truncation", "traj", "cur_frame", "sub_clip_frame", "clip_id")
    out = []
    for mode in ("eager", "fused") + (("graphed",) if graphed else ()):
        base = make()
        B, rg = base.num_envs, ranges_for(base.sys, 4)
        env = wrap(base, episode_length=3, auto_reset="fresh", auto_reset_seed=seed, domain_ranges=rg)
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=16, encoder_layer_sizes=(32,), decoder_layer_sizes=(32,))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(device)
        # (on the device the policy draws its own counter-based noise, as in tests/test_gpu_fresh_reset.py: nothing of the
        # graph's depends on a generator)
        noise = dict(noise="device", seed=9) if device.type == "cuda" else {}
        policy = ppo_networks.make_inference_fn(nets)((running_statistics.init_state(base.observation_size, device=device), flat),
                                                      **noise)
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        inner = env.unwrapped
        first = tables(inner)
        same_tables(first, expected_tables(inner, drawn(inner, rg, step=0, env_offset=0, initial=True, seed=seed)))
        state.info["steps"].copy_((torch.arange(B) % 3).to(state.info["steps"].dtype))
        key = None if noise else torch.Generator(device=device).manual_seed(11)
        datas = []
        for T in (7, 3):
            if mode == "graphed":
                state, data = acting.GraphedUnroll(env, state, policy, key, T, extra_fields=extra)()
            else:
                state, data = acting.generate_unroll(env, state, policy, key, T, extra_fields=extra, fused=mode == "fused")
            datas.append(data)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        out.append((state, [x.clone() for d in datas for x in acting._leaves(d)], tables(inner), first, datas[0], rg, inner))
    s0, l0, t0, first, d0, rg, inner = out[0]
    B = inner.num_envs
    for s1, l1, t1, f1, _, _, _ in out[1:]:
        for a, b in zip(l0, l1):
            assert a.shape == b.shape and torch.equal(a, b)
        F.same_rows(F.snapshot(s0), F.snapshot(s1), EVERY(B), F.WRITTEN + F.KEPT)
        same_tables(t0, t1)
        same_tables(first, f1)
        assert int(s1.info["reset_step"]) == 10
    ended = (d0.discount == 0).cpu()  # [7, B]
    assert ended.any(dim=1).sum() >= 3 and not bool(ended.all())
    finished = ended.any(dim=0)
    return t0, first, finished, s0


def check_wrapper_paths(make, device, graphed: bool) -> None:
    t0, first, finished, s0 = wrapper_paths(make, device, graphed)
    # (every env finishes within the first unroll of 7: episodes of 3 steps)
    assert bool(finished.all())
    for k in TABLES:
        assert not bool((bits(t0[k]) == bits(first[k])).all(dim=1).any()), k


def check_unfinished_envs_keep_their_first_domain(make, device) -> None:
    """two steps of the eager wrapper, episodes of 3 steps staggered: the envs that finished were redrawn at THAT step's
    counter, the others still hold their initial draw"""
    base = make()
    B, rg = base.num_envs, ranges_for(base.sys, 4)
    env = wrap(base, episode_length=3, auto_reset="fresh", auto_reset_seed=77, env_offset=16, domain_ranges=rg)
    state = env.reset(torch.Generator().manual_seed(5))
    inner = env.unwrapped
    first = tables(inner)
    same_tables(first, expected_tables(inner, drawn(inner, rg, step=0, env_offset=16, initial=True, seed=77)))
    state.info["steps"].copy_((torch.arange(B) % 3).to(state.info["steps"].dtype))
    want, touched = {k: v.clone() for k, v in first.items()}, torch.zeros(B, dtype=torch.bool)
    for t in range(2):
        state = env.step(state, torch.zeros((B, base.action_size), device=device))
        done = state.done.bool().cpu()
        exp = expected_tables(inner, drawn(inner, rg, step=t, env_offset=16, seed=77))
        for k in TABLES:
            want[k][done] = exp[k][done]
        touched |= done
    assert bool(touched.any()) and not bool(touched.all())
    now = tables(inner)
    same_tables(now, want)
    same_tables(now, first, ~touched)
    for k in TABLES:
        assert not bool((bits(now[k]) == bits(first[k])).all(dim=1)[touched].any()), k


# ---- case 9 ----------------------------------------------------------------------------------------------------------------
def check_restatement_alone() -> None:
    n, B, steps = 9, 4096, 4
    lo = torch.tensor([0.5, 1.0, 1e-3, 2.0, 0.25, 3.0, 7.0, 0.1, 5.0], dtype=torch.float64)
    hi = lo * torch.tensor([1.5, 1.0, 3.0, 2.0, 1.01, 1.0 + 2 ** -40, 4.0, 10.0, 1.0], dtype=torch.float64)
    env = torch.arange(B) + 12345
    wide = hi > lo
    for f in range(4):
        for shared in (False, True):
            v = torch.stack([philox.domain_draws(F.SEED, F.STEP_BASE + t, env, f, lo, hi, shared=shared) for t in range(steps)])
            assert v.dtype == torch.float64 and tuple(v.shape) == (steps, B, n)
            assert bool((v >= lo).all()) and bool((v <= hi).all())
            assert torch.equal(v[..., ~wide], lo[~wide].expand(steps, B, -1))  # lo == hi gives exactly lo
            mid = lo + (hi - lo) / 2
            assert bool((v[..., wide] < mid[wide]).any(dim=0).any(dim=0).all()) and bool((v[..., wide] > mid[wide]).any(dim=0).any(dim=0).all())
    # no two of (env, step, field, element, initial) share a (counter, word), except by the shared rule
    B2 = 64
    env = torch.arange(B2) + 7
    seen = set()
    for initial in (0, 1):
        for f in range(4):
            block0 = philox.DOMAIN_BLOCK + initial * philox.DOMAIN_INITIAL + f * philox.DOMAIN_FIELD_STRIDE
            for t in range(steps):
                for j in range(n):
                    for e in env.tolist():
                        key = (block0 + j // 4, e, t, j % 4)
                        assert key not in seen
                        seen.add(key)
    assert all(0x40000000 <= k[0] < 0x80000000 for k in seen)  # beside the noise blocks 0.. and the integer block 0x80000000
    # .. and the restatement does use those counters: its words are philox4x32 of them
    x = philox._words(F.SEED, 5, env, n, philox.STREAM_RESET, block0=philox.DOMAIN_BLOCK + 2 * philox.DOMAIN_FIELD_STRIDE)
    u = (x.reshape(B2, -1)[:, :n].double() + 0.5) * 2.0 ** -32
    assert torch.equal(philox.domain_draws(F.SEED, 5, env, "dof_damping", lo, hi), lo + u * (hi - lo))
    one = philox.domain_draws(F.SEED, 5, env, "dof_damping", lo, hi, shared=True)
    assert torch.equal(one, lo + u[:, :1] * (hi - lo))
    assert bool((u > 0).all()) and bool((u < 1).all())
