"""Checks of the prioritised start frames (vnl_env_reset_done_weighted, vnl_start_priority_update, envs/start_priority.py)
shared by tests/test_start_priority.py (host builds) and tests/test_gpu_start_priority.py: the weighted draws against their
torch restatement, the reset against vnl_env_reset fed the recorded draws, the outcome counters against torch bincounts, and
the table update against its integer restatement."""
import ctypes as C
import types

import numpy as np
import torch

import fresh_reset_cases as F
import model_cases as M
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.ppo_imitation import philox

U32 = 1 << 32
UPDATE_NCELLS = (1, 2, 63, 64, 65, 705, 4096, 4097, 15040, 32768)


def ant_env(num_envs, device="cpu"):
    """AntTracking on three copies of model_cases.ant_clip"""
    return M.ant_env(num_envs, "float", device, clips=3)


def as_words(values) -> torch.Tensor:
    """unsigned values below 2^32 -> the int32 tensor holding the same 32-bit words (CPU)"""
    v = torch.as_tensor(np.asarray(values, dtype=np.int64))
    assert bool(((v >= 0) & (v < U32)).all())
    return ((v + (1 << 31)) % U32 - (1 << 31)).to(torch.int32)


def ncells(env) -> int:
    return int(env._start_hi()) * int(env._num_clips)


def table_from_widths(widths) -> torch.Tensor:
    """int32 words of the table whose cell c owns widths[c] / sum(widths) of the 2^32 words (Python integers: exact)"""
    total, run, out = int(sum(int(w) for w in widths)), 0, []
    for w in widths:
        run += int(w)
        out.append(min((run << 32) // total, U32 - 1))
    return as_words(out)


def widths_of(cdf: torch.Tensor) -> torch.Tensor:
    """int64 width of every cell: cell c owns [cdf[c - 1], cdf[c]), the last one the rest (entry ncell - 1 is not read)"""
    edges = torch.cat((torch.zeros(1, dtype=torch.int64), philox.words_u32(cdf)[:-1], torch.tensor([U32])))
    return edges[1:] - edges[:-1]


def tables(n: int, seed: int = 0) -> dict:
    """The four tables of check 1 for `n` cells, int32 words on the CPU."""
    g = np.random.default_rng(seed)
    zeros = torch.zeros(n, dtype=torch.int32)
    out = {"uniform": as_words(philox.start_priority_table(zeros, zeros)[0])}
    k = n // 2  # (b) all mass but the one word 0xFFFFFFFF, which belongs to the last cell, on one interior cell
    out["one_cell"] = as_words([0] * k + [U32 - 1] * (n - k))
    # (c) from random counters, floor 1: a cell that never failed in 2^20 episodes has weight 1, the smallest there is
    ended = g.integers(0, 1 << 21, n)
    failed = np.where(g.random(n) < 0.5, 0, g.integers(0, 1 << 21, n))
    ended[::3] = 1 << 20
    failed[::3] = 0
    cdf_c = as_words(philox.start_priority_table(as_words(ended), as_words(failed), prior=1, floor_q16=1, decay_shift=0)[0])
    out["min_width"] = cdf_c
    w = widths_of(cdf_c)
    assert int(w.min()) >= 1 and (n < 4 or (int(w.max()) > 100 * int(w.min()) and int((w == w.min()).sum()) >= 1))
    # (d) hand-made, every third cell (the first one included) of width zero
    wd = g.integers(1, 1000, n)
    if n >= 2:
        wd[::3] = 0
    out["zero_width"] = table_from_widths(wd)
    assert n < 2 or int((widths_of(out["zero_width"]) == 0).sum()) >= (n + 2) // 3
    return out


def priority(env, cdf: torch.Tensor, counters: bool = True):
    """what RodentTracking.reset_done takes as `priority`: the table on the env's device, with zero counters or none"""
    dev = env.device
    zeros = lambda: torch.zeros(cdf.numel(), dtype=torch.int32, device=dev) if counters else None  # noqa: E731
    return types.SimpleNamespace(cdf=cdf.to(dev).contiguous(), count_ended=zeros(), count_failed=zeros())


def reset_done(env, st, mask, prio=None, truncation=None, env_offset=0, null_descriptor=False):
    """F.reset_done with a priority: RodentTracking.reset_done at (F.SEED, F.STEP_BASE + F.STEP_OFFSET) with records, which
    are returned (CPU; rows the kernel does not write keep -7 / NaN).  `null_descriptor`: the weighted entry itself, called
    with no descriptor."""
    B, dev, nq = env.num_envs, env.device, int(env.dims.nq)
    rec = {"start_frame": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "clip_id": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "noise": torch.full((B, nq), float("nan"), dtype=env._dtype, device=dev)}
    base = torch.tensor([F.STEP_BASE], dtype=torch.int64, device=dev)
    if null_descriptor:
        mk = mask.to(device=dev, dtype=torch.float32).contiguous()
        nz = _lib.ResetNoise(seed=F.SEED, step_base=base.data_ptr(), step_offset=F.STEP_OFFSET, env_offset=env_offset,
                             start_hi=env._start_hi(), noise_scale=env._reset_noise_scale,
                             start_frame_out=rec["start_frame"].data_ptr(), clip_id_out=rec["clip_id"].data_ptr(),
                             noise_out=rec["noise"].data_ptr())
        p = env._ptrs(st)
        assert env._L.vnl_env_reset_done_weighted(env._env_h, mk.data_ptr(), C.byref(nz), None, C.byref(p), None, 0,
                                                  env._stream()) == 0
    else:
        kw = {} if prio is None else {"priority": prio, "truncation": None if truncation is None else truncation.to(dev)}
        env.reset_done(st, mask.to(dev), seed=F.SEED, step_base=base, step_offset=F.STEP_OFFSET, env_offset=env_offset,
                       record=rec, **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert int(base) == F.STEP_BASE
    return {k: v.cpu() for k, v in rec.items()}


def check_weighted_draws(env, rec: dict, mask: torch.Tensor, cdf: torch.Tensor, uniform_rec: dict, env_offset=0) -> torch.Tensor:
    """check 1: start frame and clip of the masked envs == weighted_cells decoded, as integers; their noise == the uniform
    entry's, bit for bit; unmasked record rows keep their fill values.  Returns the cells."""
    B, hi = env.num_envs, int(env._start_hi())
    m = mask.bool().cpu()
    cells = philox.weighted_cells(F.SEED, F.STEP_BASE + F.STEP_OFFSET, torch.arange(B) + env_offset, cdf)
    assert bool(((cells >= 0) & (cells < cdf.numel())).all())
    assert torch.equal(rec["start_frame"][m].long(), (cells % hi)[m]), (rec["start_frame"][m], (cells % hi)[m])
    assert torch.equal(rec["clip_id"][m].long(), (cells // hi)[m])
    assert bool((widths_of(cdf)[cells] > 0).all())  # a cell of width zero is never drawn
    F.same_rows(rec, uniform_rec, m, ("noise",))
    assert bool((rec["start_frame"][~m] == -7).all()) and bool((rec["clip_id"][~m] == -7).all())
    assert bool(torch.isnan(rec["noise"][~m]).all())
    return cells


def check_draws_and_reset(env, mask: torch.Tensor, seed: int = 3, reset_check: bool = True, null_check: bool = True) -> None:
    """Checks 1, 2 and 4 on one env batch.  One stepped state serves every table (a reset leaves a state that can be reset
    again, and the draws do not depend on it); the uniform entry's record gives the noise bits to compare with."""
    dev, n = env.device, ncells(env)
    st = F.stepped_state(env, seed)
    st.done.copy_(mask.to(device=dev, dtype=st.done.dtype))
    before = F.snapshot(st)
    if null_check:  # check 4: no descriptor == vnl_env_reset_done, draws and state
        st_u = F.stepped_state(env, seed)
        st_u.done.copy_(st.done)
        uniform_rec = F.reset_done(env, st_u, mask)
        F.check_draws(env, uniform_rec, mask)
        st_n = F.stepped_state(env, seed)
        st_n.done.copy_(st.done)
        null_rec = reset_done(env, st_n, mask, null_descriptor=True)
        F.same_rows(null_rec, uniform_rec, mask.bool().cpu(), tuple(null_rec))
        F.same_rows(F.snapshot(st_u), F.snapshot(st_n), torch.ones(env.num_envs, dtype=torch.bool), tuple(before))
    else:
        uniform_rec = F.reset_done(env, F.stepped_state(env, seed), mask)
    seen = []
    for k, (name, cdf) in enumerate(tables(n, seed).items()):
        prio = priority(env, cdf)
        rec = reset_done(env, st, mask, prio)
        cells = check_weighted_draws(env, rec, mask, cdf, uniform_rec)
        seen.append(cells[mask.bool().cpu()])
        if name == "one_cell":
            assert bool((seen[-1] == n // 2).all())
        if k == 0:
            after = F.snapshot(st)
            F.check_nothing_else_moves(before, after, mask)
            if reset_check:  # check 2
                F.check_is_the_existing_reset(env, after, rec, mask)
    if n > 4:
        assert not torch.equal(seen[0], seen[2])  # the table decides, not the word alone


def counter_case(env, seed: int = 11):
    """A state for check 3 and what its counters must be.  The rodent env's sub_clip_length is 2: after stepped_state's two
    steps every env stands at its sub-clip's end (an env without a sub-clip term, the ant, is put there by hand); every
    second one is then put one frame back (ended early: a failure).  The envs share at most 4 cells; one env's start
    frame is forced below 0 and one's to start_hi; a few are marked truncated."""
    B, hi, n, L = env.num_envs, int(env._start_hi()), ncells(env), int(env._sub_clip_length)
    assert B >= 8
    g = torch.Generator().manual_seed(seed)
    frames = torch.tensor([0, min(3, hi - 1), hi - 1, min(7, hi - 1)], dtype=torch.int32)[torch.arange(B) % 4]
    clips = (torch.arange(B, dtype=torch.int32) % 4) % env._num_clips
    st = F.stepped_state(env, seed, clips, frames, 1e-3 * torch.randn((B, int(env.dims.nq)), generator=g),
                         0.3 * torch.randn((2, B, env.action_size), generator=g))
    raw = st.info["_raw"]
    cur, sub = raw["cur_frame"].cpu().clone(), raw["sub_clip_frame"].cpu().clone()
    assert torch.equal(sub, torch.full_like(sub, 2)) and torch.equal(cur, frames + 2)
    cur, sub = cur + (L - 2), sub + (L - 2)  # (nothing to do for the rodent env: L == 2)
    early = torch.arange(B) % 2 == 1
    cur[early] -= 1
    sub[early] -= 1
    cur[4] = sub[4] - 1   # start frame -1
    cur[5] = sub[5] + hi  # start frame start_hi
    raw["cur_frame"].copy_(cur), raw["sub_clip_frame"].copy_(sub)
    trunc = torch.zeros(B)
    trunc[[2, 7]] = 1.0
    mask = torch.ones(B)
    mask[[3, 6]] = 0.0
    sf0, clip = (cur - sub).long(), raw["clip_id"].cpu().long()
    valid = mask.bool() & (sf0 >= 0) & (sf0 < hi) & (clip >= 0) & (clip < env._num_clips) & (trunc == 0)
    cell = (clip * hi + sf0).clamp(0, n - 1)
    ended = torch.bincount(cell[valid], minlength=n)
    failed = torch.bincount(cell[valid & (sub < int(env._sub_clip_length))], minlength=n)
    assert int(ended.sum()) == B - 6 and 0 < int(failed.sum()) < int(ended.sum()) and int((ended > 0).sum()) <= 4
    return st, mask, trunc, ended, failed


def check_counters(env) -> None:
    """check 3"""
    n = ncells(env)
    cdf = tables(n, 5)["min_width"]
    st, mask, trunc, ended, failed = counter_case(env)
    prio = priority(env, cdf)
    reset_done(env, st, torch.zeros_like(mask), prio, trunc)  # an all-zero mask changes no counter
    assert int(prio.count_ended.abs().sum()) == 0 and int(prio.count_failed.abs().sum()) == 0
    uniform_rec = F.reset_done(env, F.stepped_state(env, 3), mask)
    rec = reset_done(env, st, mask, prio, trunc)
    assert torch.equal(prio.count_ended.cpu().long(), ended), (prio.count_ended.cpu().nonzero(), ended.nonzero())
    assert torch.equal(prio.count_failed.cpu().long(), failed)
    check_weighted_draws(env, rec, mask, cdf, uniform_rec)
    # null counters: nothing is counted (there is nothing to count into) and the draws are the same
    st2 = counter_case(env)[0]
    rec2 = reset_done(env, st2, mask, priority(env, cdf, counters=False), trunc)
    F.same_rows(rec, rec2, mask.bool(), tuple(rec))
    # without a truncation vector the truncated envs count too
    st3 = counter_case(env)[0]
    prio3 = priority(env, cdf)
    reset_done(env, st3, mask, prio3)
    assert int(prio3.count_ended.sum()) == int(ended.sum()) + 2


def update_counters(n: int, seed: int):
    """counters for check 5 (int32 words): zeros, failed > ended, values above 2^20 and above 2^31"""
    g = np.random.default_rng(seed)
    ended = g.integers(0, 1 << 12, n)
    failed = (ended * g.random(n)).astype(np.int64)
    pick = lambda p: g.random(n) < p  # noqa: E731
    ended[pick(0.2)] = 0
    failed[pick(0.1)] = 5000               # failed > ended
    big = pick(0.1)
    ended[big] = g.integers(1 << 20, U32, int(big.sum()))
    failed[pick(0.05)] = U32 - 1
    ended[-1], failed[0] = U32 - 1, 0
    return as_words(ended), as_words(failed)


def run_update(L, device, ended, failed, prior, floor_q16, decay_shift, stream=None):
    e, f = ended.to(device).clone(), failed.to(device).clone()
    cdf = torch.full_like(e, 0x55555555)
    rc = L.vnl_start_priority_update(e.data_ptr(), f.data_ptr(), cdf.data_ptr(), e.numel(), prior, floor_q16, decay_shift, stream)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return rc, cdf.cpu(), e.cpu(), f.cpu()


def check_update(L, device) -> None:
    """check 5: the library's update == philox.start_priority_table as exact integers, table and decayed counters"""
    for n in UPDATE_NCELLS:
        ended, failed = update_counters(n, n)
        for prior in (1, 7):
            for floor_q16 in (1, 6554, 65536):
                for shift in (0, 1, 31):
                    rc, cdf, e, f = run_update(L, device, ended, failed, prior, floor_q16, shift)
                    assert rc == 0
                    want = philox.start_priority_table(ended, failed, prior, floor_q16, shift)
                    for got, ref, name in zip((cdf, e, f), want, ("cdf", "ended", "failed")):
                        assert torch.equal(philox.words_u32(got), ref), (name, n, prior, floor_q16, shift)
                    w = widths_of(cdf)
                    assert int(w.min()) >= 1 and int(w.sum()) == U32 and int(philox.words_u32(cdf)[-1]) == U32 - 1
        zeros = torch.zeros(n, dtype=torch.int32)
        rc, cdf, e, f = run_update(L, device, zeros, zeros, 1, 6554, 1)
        assert rc == 0 and philox.words_u32(cdf)[:-1].tolist() == [((c + 1) << 32) // n for c in range(n - 1)]
        assert int(e.abs().sum()) == 0 and int(f.abs().sum()) == 0


def check_update_argument_errors(L, device) -> None:
    """check 6 for vnl_start_priority_update: the stated code, and table and counters as they were"""
    ended, failed = update_counters(64, 1)
    big = torch.zeros(32769, dtype=torch.int32)
    bad = [(dict(prior=0), -1), (dict(floor_q16=0), -1), (dict(floor_q16=65537), -1), (dict(decay_shift=-1), -1),
           (dict(decay_shift=32), -1)]
    for kw, code in bad:
        args = dict(prior=1, floor_q16=6554, decay_shift=1)
        args.update(kw)
        rc, cdf, e, f = run_update(L, device, ended, failed, **args)
        assert rc == code, kw
        assert bool((cdf == 0x55555555).all()) and torch.equal(e, ended) and torch.equal(f, failed)
    rc, cdf, e, f = run_update(L, device, big, big, 1, 6554, 1)
    assert rc == -5 and bool((cdf == 0x55555555).all())
    e = ended.to(device).clone()
    for ptrs in ((None, e.data_ptr(), e.data_ptr()), (e.data_ptr(), None, e.data_ptr()), (e.data_ptr(), e.data_ptr(), None)):
        assert L.vnl_start_priority_update(*ptrs, 64, 1, 6554, 1, None) == -1
    assert L.vnl_start_priority_update(e.data_ptr(), e.data_ptr(), e.data_ptr(), 0, 1, 6554, 1, None) == -1
    assert torch.equal(e.cpu(), ended) and L.vnl_last_error()
