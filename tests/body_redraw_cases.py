"""Checks of the body-domain redraw at fresh resets (vnl_env_set_body_domain_ranges, the body part of vnl_env_redraw_domain and
of the redraw inside vnl_env_reset_done) shared by tests/test_body_redraw.py (host builds) and tests/test_gpu_body_redraw.py:
the draw against its restatement ppo_imitation/philox.py body_domain_draws, the folded tables against with_body_domain of the
same values, the fused redraw against the separate launch, both range sets together, sharding, degenerate and absent ranges,
the argument checks, the wrapper paths.  Every comparison is of bits; every function takes a base env WITHOUT ranges (rodent: the
specialised randomised kernels, 66 bodies as given make a second lane trip, 53 dynamic ones with at most 2 members; ant: the
generic ones, 10 dynamic bodies with up to 5 members)."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_domain_cases as BD
import domain_redraw_cases as R
import fresh_reset_cases as F
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics

TABLES = ("dom_mass", "dom_ipos", "dom_inertia6", "dom_tminv")
FIELDS = philox.BODY_DOMAIN_FIELDS
STEP, ENV_OFFSET, EVERY = R.STEP, R.ENV_OFFSET, R.EVERY
bits, half_mask, redraw, reset_done = R.bits, R.half_mask, R.redraw, R.reset_done


def ranges_for(sys, with_mass=False) -> dict:
    """Bounds with the spread of tests/body_domain_cases.py: mass x [0.7, 1.3]; moments x [0.7 * 0.8, 1.3 * 1.25] (`with_mass`:
    the mass multiples, a change of density); ipos -/+ 0.2 |ipos| per component.  lo < hi wherever the compiled value -- for
    ipos the body's |ipos| -- is non-zero."""
    c = BD.compiled(sys)
    m, i, p = c["body_mass"], c["body_inertia"], c["body_ipos"]
    r = BD.IPOS * np.linalg.norm(p, axis=1, keepdims=True)
    a, b = (BD.MASS[0], BD.MASS[1]) if with_mass else (BD.MASS[0] * BD.AXIS[0], BD.MASS[1] * BD.AXIS[1])
    return {"body_mass": (m * BD.MASS[0], m * BD.MASS[1]), "body_inertia": (i * a, i * b), "body_ipos": (p - r, p + r)}


def tables(env) -> dict:
    return {k: env.domain_table(k) for k in TABLES}


def same_tables(a, b, rows=None, keys=TABLES) -> None:
    R.same_tables(a, b, rows, keys)


def differ_in_every_row(a: dict, b: dict, rows=None) -> None:
    """every table differs in every (given) env; dom_mass etc. hold non-zero compiled values in every row"""
    for k in TABLES:
        same = (bits(a[k]) == bits(b[k])).all(dim=1)
        assert not bool((same if rows is None else same[rows]).any()), k


def drawn(env, step=STEP, env_offset=ENV_OFFSET, initial=False, seed=F.SEED) -> dict:
    """{field: float64 (B, nbody[, 3])} of philox.body_domain_draws from the env's own ranges, for every env of the batch"""
    rg = env.body_domain_ranges
    ids = torch.arange(env.num_envs) + env_offset
    return philox.body_domain_draws(seed, step, ids, rg, shared=rg["shared"], inertia_with_mass=rg["inertia_with_mass"], initial=initial)


def by_hand(base, values: dict) -> "object":
    return base.with_body_domain({k: v for k, v in values.items()})


def clear_ranges_keep_tables(env) -> None:
    """vnl_env_set_body_domain_ranges(null): the ranges go, the tables stay"""
    _lib.check(env._L, env._L.vnl_env_set_body_domain_ranges(env._env_h, None, env._stream()))
    env._body_domain_ranges = None


# ---- case 1 ----------------------------------------------------------------------------------------------------------------
def check_draw_is_the_restatement(base) -> None:
    B = base.num_envs
    mask = half_mask(B)
    m = mask.bool()
    rg = ranges_for(base.sys)
    env = base.with_body_domain_ranges(rg)
    assert set(env.body_domain_ranges) == set(rg) | {"shared", "inertia_with_mass"} and base.body_domain_ranges is None
    before = tables(env)
    same_tables(before, tables(by_hand(base, BD.identity(base.sys, B))))  # allocated at the compiled values
    redraw(env, mask)
    after = tables(env)
    vals = drawn(env)
    c = BD.compiled(base.sys)
    for k in FIELDS:  # row 0, the world body, holds the compiled values; the others lie inside the bounds
        assert np.array_equal(vals[k][:, 0].numpy(), np.broadcast_to(c[k][0], vals[k][:, 0].shape))
        assert bool((vals[k] >= env.body_domain_ranges[k][0]).all()) and bool((vals[k] <= env.body_domain_ranges[k][1]).all())
    want = tables(by_hand(base, vals))
    same_tables(after, want, m)
    same_tables(after, before, ~m)
    differ_in_every_row(after, before, m)
    # one uniform per (env, episode) for the whole of a shared field
    env2 = base.with_body_domain_ranges(rg, shared=("body_mass",))
    assert env2.body_domain_ranges["shared"] == ("body_mass",)
    redraw(env2)
    v2 = drawn(env2)
    same_tables(tables(env2), tables(by_hand(base, v2)))
    lo, hi = env2.body_domain_ranges["body_mass"]
    wide = hi > lo
    u = ((v2["body_mass"] - lo) / (hi - lo))[:, wide]
    assert float((u - u[:, :1]).abs().max()) < 1e-12 and float(u[:, 0].std()) > 0.05
    u1 = ((vals["body_mass"] - lo) / (hi - lo))[:, wide]
    assert float(u1.std(dim=1).min()) > 0.05  # .. and an unshared one does not
    # moments on the uniform of their body's mass: a change of density
    rgm = ranges_for(base.sys, with_mass=True)
    env3 = base.with_body_domain_ranges(rgm, inertia_with_mass=True)
    assert env3.body_domain_ranges["inertia_with_mass"] is True
    redraw(env3)
    v3 = drawn(env3)
    same_tables(tables(env3), tables(by_hand(base, v3)))
    (lm, hm), (li, hi_) = env3.body_domain_ranges["body_mass"], env3.body_domain_ranges["body_inertia"]
    um = (v3["body_mass"] - lm) / (hm - lm)
    ui = (v3["body_inertia"] - li) / (hi_ - li)
    both = ((hm > lm)[:, None] & (hi_ > li))
    assert bool(both.any()) and float((ui - um[:, :, None])[:, both].abs().max()) < 1e-12
    alone = philox.body_domain_draws(F.SEED, STEP, torch.arange(B) + ENV_OFFSET, {"body_mass": env3.body_domain_ranges["body_mass"]})
    assert torch.equal(v3["body_mass"], alone["body_mass"])  # the mass draw is the one made without the flag
    # the first episode's block range is its own
    env4 = base.with_body_domain_ranges(rg)
    redraw(env4, initial=True)
    first = tables(env4)
    same_tables(first, tables(by_hand(base, drawn(env4, initial=True))))
    differ_in_every_row(first, want)


# ---- case 2 ----------------------------------------------------------------------------------------------------------------
def check_redrawn_env_is_the_env_set_by_hand(base) -> None:
    B = base.num_envs
    env = base.with_body_domain_ranges(ranges_for(base.sys))
    redraw(env)
    env2 = by_hand(base, drawn(env))
    same_tables(tables(env), tables(env2))
    a, b = F.snapshot(F.stepped_state(env, 4)), F.snapshot(F.stepped_state(env2, 4))
    F.same_rows(a, b, EVERY(B), F.WRITTEN + F.KEPT)
    c = F.snapshot(F.stepped_state(base, 4))
    assert not torch.equal(a["qvel"], c["qvel"])  # the bodies did change the dynamics


# ---- case 3 ----------------------------------------------------------------------------------------------------------------
def check_fused_is_separate(base, weighted: bool) -> None:
    B, rg = base.num_envs, ranges_for(base.sys)
    mask = half_mask(B)
    out = []
    for fused in (True, False):
        env = base.with_body_domain_ranges(rg)
        st = F.stepped_state(env, 3)
        st.done.copy_(mask.to(device=env.device, dtype=st.done.dtype))
        prio = R.uniform_priority(env) if weighted else None
        sf0 = (st.info["cur_frame"] - st.info["sub_clip_frame"]).cpu()
        want = tables(by_hand(base, drawn(env)))
        if not fused:
            redraw(env, mask)
            clear_ranges_keep_tables(env)
        reset_done(env, st, mask, priority=prio)
        out.append((F.snapshot(st), tables(env), prio))
    (s0, t0, p0), (s1, t1, p1) = out
    F.same_rows(s0, s1, EVERY(B), tuple(s0))
    same_tables(t0, t1)
    same_tables(t0, want, mask.bool())
    if weighted:
        assert torch.equal(p0.count_ended, p1.count_ended) and torch.equal(p0.count_failed, p1.count_failed)
        assert int(p0.count_ended.sum()) == int(((sf0 >= 0) & (sf0 < base._start_hi()) & mask.bool()).sum())


# ---- case 4 ----------------------------------------------------------------------------------------------------------------
def check_both_range_sets_together(base) -> None:
    rg4, rgb = R.ranges_for(base.sys, 6), ranges_for(base.sys)
    four, body = base.with_domain_ranges(rg4), base.with_body_domain_ranges(rgb)
    ab = base.with_domain_ranges(rg4).with_body_domain_ranges(rgb)
    ba = base.with_body_domain_ranges(rgb).with_domain_ranges(rg4)
    for e in (four, body, ab, ba):
        redraw(e, half_mask(base.num_envs))
    for e in (ab, ba):
        assert e.domain_ranges is not None and e.body_domain_ranges is not None
        R.same_tables(R.tables(e), R.tables(four))
        same_tables(tables(e), tables(body))
    differ_in_every_row(tables(ab), tables(four), half_mask(base.num_envs).bool())


# ---- case 5 ----------------------------------------------------------------------------------------------------------------
def check_sharding(make) -> None:
    whole = make(8)
    rg = ranges_for(whole.sys)
    nq, nu = int(whole.dims.nq), whole.action_size
    g = torch.Generator().manual_seed(9)
    sf = torch.randint(0, max(whole._T - 10, 1), (8,), generator=g, dtype=torch.int32)
    nz = 1e-3 * torch.randn((8, nq), generator=g)
    clip = torch.randint(0, whole._num_clips, (8,), generator=g, dtype=torch.int32)
    act = 0.3 * torch.randn((2, 8, nu), generator=g)
    mask = half_mask(8)

    def run(env, sl, lo):
        env = env.with_body_domain_ranges(rg)
        redraw(env, env_offset=lo, initial=True)  # the first episode's bodies, then two steps with them, then the fresh reset
        st = F.stepped_state(env, 0, clip[sl], sf[sl], nz[sl], act[:, sl])
        reset_done(env, st, mask[sl], env_offset=lo)
        return F.snapshot(st), tables(env)

    full, tab = run(whole, slice(0, 8), 0)
    for lo in (0, 4):
        sl = slice(lo, lo + 4)
        snap, t = run(make(4), sl, lo)
        F.same_rows({k: v[sl] for k, v in full.items()}, snap, EVERY(4), tuple(snap))
        same_tables({k: v[sl] for k, v in tab.items()}, t)


# ---- case 6 ----------------------------------------------------------------------------------------------------------------
def check_degenerate_and_absent_ranges(base) -> None:
    B = base.num_envs
    mask = half_mask(B)
    m = mask.bool()
    plain = by_hand(base, BD.identity(base.sys, B))
    env = base.with_body_domain_ranges({k: (v, v) for k, v in BD.compiled(base.sys).items()})
    snaps = []
    for e in (plain, env):
        st = F.stepped_state(e, 6)
        reset_done(e, st, mask)
        snaps.append(F.snapshot(st))
    F.same_rows(snaps[0], snaps[1], EVERY(B), tuple(snaps[0]))
    same_tables(tables(plain), tables(env))
    # a field without bounds keeps the with_body_domain values through a reset
    dom = BD.random_body_domain(base.sys, B, 5)
    given = by_hand(base, dom)
    before = tables(given)
    only = given.with_body_domain_ranges({"body_mass": ranges_for(base.sys)["body_mass"]})
    same_tables(before, tables(only))  # the with_body_domain values are kept until the first redraw
    st = F.stepped_state(only, 7)
    reset_done(only, st, mask)
    after = tables(only)
    want = tables(by_hand(base, dict(dom, body_mass=drawn(only)["body_mass"].numpy())))
    same_tables(after, want, m)
    same_tables(after, before, ~m)
    differ_in_every_row(after, before, m)
    # no body ranges: a fresh reset leaves the four body tables alone, four-field ranges or not
    for e in (given, given.with_domain_ranges(R.ranges_for(base.sys))):
        st = F.stepped_state(e, 7)
        reset_done(e, st, mask)
        same_tables(before, tables(e))


# ---- case 7 ----------------------------------------------------------------------------------------------------------------
def check_errors_launch_nothing(base) -> None:
    B, rg = base.num_envs, ranges_for(base.sys)
    env = base.with_body_domain_ranges(rg)
    redraw(env)
    st = F.stepped_state(env, 1)
    snap, tab = F.snapshot(st), tables(env)
    L, nb = env._L, int(env.dims.nbody)
    shape = {"body_mass": (nb,), "body_inertia": (nb, 3), "body_ipos": (nb, 3)}

    def c_call(bounds: dict, flags=0):
        """vnl_env_set_body_domain_ranges with the given {field index: (lo, hi)} (None: a null pointer)"""
        desc, keep = _lib.BodyDomainRanges(), []
        for f, pair in bounds.items():
            ts = [None if x is None else torch.as_tensor(np.broadcast_to(x, shape[FIELDS[f]]).copy(), dtype=torch.float64).to(env.device).contiguous()
                  for x in pair]
            keep += ts
            desc.lo[f], desc.hi[f] = (None if t is None else t.data_ptr() for t in ts)
        desc.flags = flags
        return L.vnl_env_set_body_domain_ranges(env._env_h, C.byref(desc), env._stream())

    (ml, mh), (il, ih), (pl, ph) = rg["body_mass"], rg["body_inertia"], rg["body_ipos"]
    bad_c = [(0, {0: (mh + 1e-3, ml)}), (0, {0: (-0.1, mh)}), (1, {1: (-1e-9, ih)}), (2, {2: (np.nan, ph)}), (2, {2: (pl, np.inf)}),
             (1, {1: (il, np.inf)}), (0, {0: (ml, None)}), (2, {2: (None, ph)}),
             (0, {0: (0.0, mh)}),   # at the lower bounds the bodies with dofs are massless
             (1, {1: (0.0, ih)})]   # .. or no member of them has three moments > 0
    for f, bounds in bad_c:
        assert c_call(bounds) == -1, (f, bounds)
        assert FIELDS[f].encode() in L.vnl_last_error(), L.vnl_last_error()  # the field's name
    assert c_call({1: (il, ih)}, flags=_lib.BODY_RANGES_INERTIA_WITH_MASS) == -1 and b"body_mass" in L.vnl_last_error()
    assert L.vnl_env_set_body_domain_ranges(None, None, None) == -1
    bad_py = [{"body_mass": (mh + 1e-3, ml)}, {"body_mass": (-0.1, 1.0)}, {"body_inertia": (-1e-9, ih)}, {"body_ipos": (float("nan"), 1.0)},
              {"body_ipos": (pl, float("inf"))}, {"body_mass": (np.zeros(3), np.ones(3))}, {"body_inertia": (np.zeros(nb), np.ones(nb))},
              {"body_mass": 1.0}, {"body_mass": (0.0, mh)}, {"body_inertia": (0.0, ih)}, {"cg_friction": (0.5, 1.0)}]
    for r in bad_py:
        with pytest.raises(ValueError):
            env.with_body_domain_ranges(r)
    with pytest.raises(ValueError, match="no range"):
        env.with_body_domain_ranges({"body_mass": (ml, mh)}, shared=("body_ipos",))
    with pytest.raises(ValueError, match="body_mass"):
        env.with_body_domain_ranges({"body_inertia": (il, ih)}, inertia_with_mass=True)
    with pytest.raises(ValueError):  # with_domain_ranges goes on refusing the body field names
        env.with_domain_ranges({"body_mass": (0.5, 1.0)})
    with pytest.raises(ValueError, match="no domain ranges"):
        base.redraw_domain(seed=1, step_base=0)
    for kw in ({}, dict(auto_reset="first_state")):
        with pytest.raises(ValueError, match="auto_reset='fresh'"):
            wrap(base, episode_length=3, body_domain_ranges=rg, **kw)
    with pytest.raises(ValueError):
        wrap(base, episode_length=3, auto_reset="fresh", body_inertia_with_mass=True)
    if env.device.type == "cuda":
        torch.cuda.synchronize(env.device)
    F.same_rows(snap, F.snapshot(st), EVERY(B), tuple(snap))
    same_tables(tab, tables(env))
    assert env.body_domain_ranges is not None
    redraw(env, initial=True)  # .. and the ranges are still the ones set: a valid call draws from them
    same_tables(tables(env), tables(by_hand(base, drawn(env, initial=True))))
    w = wrap(base, episode_length=3, auto_reset="fresh", body_domain_ranges=rg, body_domain_shared=("body_mass",))
    assert w.mode == "fresh" and w.unwrapped.body_domain_ranges["shared"] == ("body_mass",)
    small = w.unwrapped.with_num_envs(2)
    assert small.body_domain_ranges["shared"] == ("body_mass",) and small.domain is None
    # the ranges go with vnl_env_set_body_domain(null), not with vnl_env_set_domain(null)
    _lib.check(L, L.vnl_env_set_domain(env._env_h, None, env._stream()))
    redraw(env)
    _lib.check(L, L.vnl_env_set_body_domain(env._env_h, None, env._stream()))
    step = torch.zeros(1, dtype=torch.int64, device=env.device)
    nz = _lib.ResetNoise(seed=1, step_base=step.data_ptr())
    assert L.vnl_env_redraw_domain(env._env_h, None, C.byref(nz), 0, env._stream()) == -1 and b"no ranges" in L.vnl_last_error()


# ---- case 8 ----------------------------------------------------------------------------------------------------------------
def wrapper_paths(make, device, graphed: bool, seed=77):
    """Episodes of 3 steps ending on different steps, T = 7 then 3: eager wrapper == fused unroll (== one replay of
    GraphedUnroll per unroll length, on the device), body tables included."""
    extra = ("truncation", "traj", "cur_frame", "sub_clip_frame", "clip_id")
    out = []
    for mode in ("eager", "fused") + (("graphed",) if graphed else ()):
        base = make()
        B, rg = base.num_envs, ranges_for(base.sys)
        env = wrap(base, episode_length=3, auto_reset="fresh", auto_reset_seed=seed, body_domain_ranges=rg)
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=16, encoder_layer_sizes=(32,), decoder_layer_sizes=(32,))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(device)
        noise = dict(noise="device", seed=9) if device.type == "cuda" else {}
        policy = ppo_networks.make_inference_fn(nets)((running_statistics.init_state(base.observation_size, device=device), flat),
                                                      **noise)
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        inner = env.unwrapped
        first = tables(inner)
        same_tables(first, tables(by_hand(base, drawn(inner, step=0, env_offset=0, initial=True, seed=seed))))
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
        out.append((state, [x.clone() for d in datas for x in acting._leaves(d)], tables(inner), first, datas[0]))
    s0, l0, t0, first, d0 = out[0]
    B = t0["dom_mass"].shape[0]
    for s1, l1, t1, f1, _ in out[1:]:
        for a, b in zip(l0, l1):
            assert a.shape == b.shape and torch.equal(a, b)
        F.same_rows(F.snapshot(s0), F.snapshot(s1), EVERY(B), F.WRITTEN + F.KEPT)
        same_tables(t0, t1)
        same_tables(first, f1)
        assert int(s1.info["reset_step"]) == 10
    ended = (d0.discount == 0).cpu()
    assert ended.any(dim=1).sum() >= 3 and not bool(ended.all())
    return t0, first, ended.any(dim=0)


def check_wrapper_paths(make, device, graphed: bool) -> None:
    t0, first, finished = wrapper_paths(make, device, graphed)
    assert bool(finished.all())  # (every env finishes within the first unroll of 7: episodes of 3 steps)
    differ_in_every_row(t0, first)


def check_unfinished_envs_keep_their_first_bodies(make, device) -> None:
    """two steps of the eager wrapper, episodes of 3 steps staggered: the envs that finished were redrawn at THAT step's
    counter, the others still hold their initial draw"""
    base = make()
    B, rg = base.num_envs, ranges_for(base.sys)
    env = wrap(base, episode_length=3, auto_reset="fresh", auto_reset_seed=77, env_offset=16, body_domain_ranges=rg)
    state = env.reset(torch.Generator().manual_seed(5))
    inner = env.unwrapped
    first = tables(inner)
    same_tables(first, tables(by_hand(base, drawn(inner, step=0, env_offset=16, initial=True, seed=77))))
    state.info["steps"].copy_((torch.arange(B) % 3).to(state.info["steps"].dtype))
    want, touched = {k: v.clone() for k, v in first.items()}, torch.zeros(B, dtype=torch.bool)
    for t in range(2):
        state = env.step(state, torch.zeros((B, base.action_size), device=device))
        done = state.done.bool().cpu()
        exp = tables(by_hand(base, drawn(inner, step=t, env_offset=16, seed=77)))
        for k in TABLES:
            want[k][done] = exp[k][done]
        touched |= done
    assert bool(touched.any()) and not bool(touched.all())
    now = tables(inner)
    same_tables(now, want)
    same_tables(now, first, ~touched)
    differ_in_every_row(now, first, touched)


# ---- case 10 ---------------------------------------------------------------------------------------------------------------
def check_restatement_alone() -> None:
    nb, B, steps = 7, 512, 3
    g = np.random.default_rng(0)
    lo = {"body_mass": g.uniform(0.5, 1.0, nb), "body_inertia": g.uniform(1e-3, 2e-3, (nb, 3)), "body_ipos": g.uniform(-1, 1, (nb, 3))}
    hi = {k: v + g.uniform(0.1, 1.0, v.shape) * np.abs(v) for k, v in lo.items()}
    hi["body_mass"][2], hi["body_inertia"][3], hi["body_ipos"][4, 1] = lo["body_mass"][2], lo["body_inertia"][3], lo["body_ipos"][4, 1]
    rg = {k: (lo[k], hi[k]) for k in FIELDS}
    env = torch.arange(B) + 12345
    for shared, with_mass in (((), False), (("body_mass", "body_ipos"), False), ((), True), (("body_mass",), True)):
        v = [philox.body_domain_draws(F.SEED, F.STEP_BASE + t, env, rg, shared=shared, inertia_with_mass=with_mass) for t in range(steps)]
        for k in FIELDS:
            x = torch.stack([d[k] for d in v])
            l, h = torch.from_numpy(lo[k]), torch.from_numpy(hi[k])
            assert x.dtype == torch.float64 and tuple(x.shape) == (steps, B) + lo[k].shape
            assert bool((x >= l).all()) and bool((x <= h).all())
            assert torch.equal(x[:, :, 0], l[0].expand(steps, B, *l.shape[1:]))  # row 0 is never drawn
            eq = h == l
            assert torch.equal(x[..., eq], l[eq].expand(steps, B, -1))  # lo == hi gives exactly lo
            wide = (h > l).clone()
            wide[0] = False
            mid = l + (h - l) / 2
            assert bool((x[..., wide] < mid[wide]).any(dim=0).any(dim=0).all()) and bool((x[..., wide] > mid[wide]).any(dim=0).any(dim=0).all())
    # no two of (env, step, field 0..6, element, initial) share a (counter, word), except by the shared and with-mass rules
    n4 = 9
    seen = set()
    for initial in (0, 1):
        for f, n in [(f, n4) for f in range(4)] + [(4, nb), (5, 3 * nb), (6, 3 * nb)]:
            block0 = philox.DOMAIN_BLOCK + initial * philox.DOMAIN_INITIAL + f * philox.DOMAIN_FIELD_STRIDE
            for t in range(steps):
                for j in range(n):
                    for e in range(7, 7 + 16):
                        key = (block0 + j // 4, e, t, j % 4)
                        assert key not in seen
                        seen.add(key)
    assert all(0x40000000 <= k[0] < 0x80000000 for k in seen)  # beside the noise blocks 0.. and the integer block 0x80000000
    # .. and the restatement does use those counters: its words are philox4x32 of them
    e2 = torch.arange(16) + 7
    for f, k in enumerate(FIELDS):
        n = lo[k].size
        x = philox._words(F.SEED, 5, e2, n, philox.STREAM_RESET, block0=philox.DOMAIN_BLOCK + philox.DOMAIN_INITIAL + (4 + f) * philox.DOMAIN_FIELD_STRIDE)
        u = ((x.reshape(16, -1)[:, :n].double() + 0.5) * 2.0 ** -32).cpu()
        l, h = torch.from_numpy(lo[k]).reshape(-1), torch.from_numpy(hi[k]).reshape(-1)
        want = (l + u * (h - l)).reshape((16,) + lo[k].shape)
        got = philox.body_domain_draws(F.SEED, 5, e2, rg, initial=True)[k]
        assert torch.equal(got[:, 1:], want[:, 1:])
        assert bool((u > 0).all()) and bool((u < 1).all())
    # .. for a later draw (initial=False) at another step as well, a shared field that is not the mass among them
    step = F.STEP_BASE + 2
    later = philox.body_domain_draws(F.SEED, step, e2, rg, shared=("body_ipos",))
    for f, k in enumerate(FIELDS):
        n = lo[k].size
        x = philox._words(F.SEED, step, e2, n, philox.STREAM_RESET, block0=philox.DOMAIN_BLOCK + (4 + f) * philox.DOMAIN_FIELD_STRIDE)
        u = ((x.reshape(16, -1)[:, :n].double() + 0.5) * 2.0 ** -32).cpu()
        if k == "body_ipos":
            u = u[:, :1].expand(16, n)  # word 0 of block 0 for every element
        l, h = torch.from_numpy(lo[k]).reshape(-1), torch.from_numpy(hi[k]).reshape(-1)
        want = (l + u * (h - l)).reshape((16,) + lo[k].shape)
        assert torch.equal(later[k][:, 1:], want[:, 1:]), k
        assert not torch.equal(later[k][:, 1:], philox.body_domain_draws(F.SEED, step, e2, rg, shared=("body_ipos",), initial=True)[k][:, 1:])
    one = philox.body_domain_draws(F.SEED, 5, e2, rg, shared=("body_mass",), inertia_with_mass=True, initial=True)
    x = philox._words(F.SEED, 5, e2, 1, philox.STREAM_RESET, block0=philox.DOMAIN_BLOCK + philox.DOMAIN_INITIAL + 4 * philox.DOMAIN_FIELD_STRIDE)
    u0 = ((x.reshape(16, -1)[:, :1].double() + 0.5) * 2.0 ** -32).cpu()
    l, h = torch.from_numpy(lo["body_inertia"]), torch.from_numpy(hi["body_inertia"])
    assert torch.equal(one["body_inertia"][:, 1:], (l + u0[:, :, None] * (h - l))[:, 1:])  # the shared mass word reaches the moments
