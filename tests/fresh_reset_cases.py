"""Checks of the fresh episode reset (vnl_env_reset_done, RodentTracking.reset_done) shared by tests/test_fresh_reset.py (host
builds) and tests/test_gpu_fresh_reset.py: the draws against their torch restatement, the reset against vnl_env_reset fed
the recorded draws, and that nothing else moves."""
import dataclasses

import numpy as np
import torch

import helpers as H
from vnl_brax_imitation_amd.envs.base import PipelineState
from vnl_brax_imitation_amd.ppo_imitation import philox

RAW = ("obs", "reward", "done", "metrics", "traj", "termination_error", "cur_frame", "sub_clip_frame", "clip_id")
KEPT = ("reward", "done", "metrics")  # the terminal step's values stay (brax auto-reset)
WRITTEN = tuple(PipelineState._FIELDS) + tuple(k for k in RAW if k not in KEPT)
SEED = 0x9E3779B97F4A7C15  # both key words in use
STEP_BASE, STEP_OFFSET = (1 << 32) + 5, 3  # the high counter word in use


def three_clips():
    """The golden clip three times, clip k moved by 0.01 k along x: the clip an env tracks shows in every reference row."""
    c = H.reference_clip()
    shift = lambda a, k: a + np.array([0.01 * k, 0.0, 0.0], dtype=a.dtype)  # noqa: E731
    return type(c).stack([dataclasses.replace(c, position=shift(c.position, k), body_positions=shift(c.body_positions, k))
                          for k in range(3)])


def snapshot(st) -> dict:
    out = {n: st.pipeline_state.raw(n).detach().cpu().clone() for n in PipelineState._FIELDS}
    out.update({k: st.info["_raw"][k].detach().cpu().clone() for k in RAW})
    return out


def same_rows(a: dict, b: dict, rows: torch.Tensor, fields) -> None:
    """bitwise equality of the rows `rows` (bool [B]) of the named buffers (NaN-safe: compared as integers)"""
    assert bool(rows.any())
    for k in fields:
        x, y = a[k][rows], b[k][rows]
        if x.is_floating_point():
            it = torch.int64 if x.dtype == torch.float64 else torch.int32
            x, y = x.contiguous().view(it), y.contiguous().view(it)
        assert torch.equal(x, y), k


def stepped_state(env, seed: int, clip_id=None, start_frame=None, noise=None, actions=None):
    """A state two control steps after a reset: reward, metrics and the frame counters are nonzero."""
    B, dev = env.num_envs, env.device
    g = torch.Generator().manual_seed(seed)
    if start_frame is None:
        start_frame = torch.randint(0, max(env._T - 10, 1), (B,), generator=g, dtype=torch.int32)
        noise = 1e-3 * torch.randn((B, int(env.dims.nq)), generator=g)
        clip_id = torch.randint(0, env._num_clips, (B,), generator=g, dtype=torch.int32)
        actions = 0.3 * torch.randn((2, B, env.action_size), generator=g)
    st = env.reset(start_frame=start_frame, noise=noise, clip_id=clip_id)
    for a in actions:
        st = env.step(st, a.to(dev))
    return st


def reset_done(env, st, mask, env_offset=0, logs=()):
    """RodentTracking.reset_done at (SEED, STEP_BASE + STEP_OFFSET) with records; returns the records (CPU).  Rows the
    kernel does not write keep the fill values -7 / NaN."""
    B, dev, nq = env.num_envs, env.device, int(env.dims.nq)
    rec = {"start_frame": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "clip_id": torch.full((B,), -7, dtype=torch.int32, device=dev),
           "noise": torch.full((B, nq), float("nan"), dtype=env._dtype, device=dev)}
    base = torch.tensor([STEP_BASE], dtype=torch.int64, device=dev)
    env.reset_done(st, mask.to(dev), seed=SEED, step_base=base, step_offset=STEP_OFFSET, env_offset=env_offset, logs=logs,
                   record=rec)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert int(base) == STEP_BASE  # the kernel only reads the counter
    return {k: v.cpu() for k, v in rec.items()}


def start_hi(env) -> int:
    return max(env._clip_length - env._sub_clip_length - env._ref_traj_length, 1)


def check_draws(env, rec: dict, mask: torch.Tensor, env_offset=0) -> None:
    """item 1: the recorded draws of the masked envs against philox.reset_draws; unmasked record rows untouched"""
    B, nq, scale = env.num_envs, int(env.dims.nq), env._reset_noise_scale
    m = mask.bool().cpu()
    sf, clip, nz = philox.reset_draws(SEED, STEP_BASE + STEP_OFFSET, torch.arange(B) + env_offset, nq, start_hi(env),
                                      env._num_clips, scale)
    assert torch.equal(rec["start_frame"][m].long(), sf[m]) and torch.equal(rec["clip_id"][m].long(), clip[m])
    assert bool(((sf >= 0) & (sf < start_hi(env))).all()) and bool(((clip >= 0) & (clip < env._num_clips)).all())
    err = float((rec["noise"][m].double() - nz[m].double()).abs().max())
    print(f"[fresh reset draws] B={B} masked={int(m.sum())} max |noise - reference| = {err:.3e} (bound {1e-5 * scale:.1e})")
    assert err <= 1e-5 * scale
    assert bool((rec["start_frame"][~m] == -7).all()) and bool((rec["clip_id"][~m] == -7).all())
    assert bool(torch.isnan(rec["noise"][~m]).all())


def check_is_the_existing_reset(env, after: dict, rec: dict, mask: torch.Tensor) -> None:
    """item 2: vnl_env_reset fed the recorded draws gives the same bits in every field a reset writes"""
    m = mask.bool().cpu()
    sf = torch.where(m, rec["start_frame"], torch.zeros_like(rec["start_frame"]))
    clip = torch.where(m, rec["clip_id"], torch.zeros_like(rec["clip_id"]))
    nz = torch.where(m[:, None], rec["noise"], torch.zeros_like(rec["noise"]))
    ref = snapshot(env.reset(start_frame=sf, noise=nz, clip_id=clip))
    same_rows(after, ref, m, WRITTEN)
    assert torch.equal(after["cur_frame"][m], rec["start_frame"][m]) and torch.equal(after["clip_id"][m], rec["clip_id"][m])
    assert bool((after["sub_clip_frame"][m] == 0).all())


def check_nothing_else_moves(before: dict, after: dict, mask: torch.Tensor) -> None:
    """item 3: every row of an unmasked env, and reward / done / metrics of every env, bit for bit"""
    m = mask.bool().cpu()
    same_rows(before, after, ~m, tuple(before))
    same_rows(before, after, torch.ones_like(m), KEPT)
    assert float(before["reward"].abs().min()) > 0 and float(before["metrics"].abs().sum(1).min()) > 0
    assert bool((before["done"][m] != 0).all())


def check_items_1_to_3(env, mask: torch.Tensor, mask2: torch.Tensor, seed: int = 3) -> None:
    """Items 1-3 on one env batch: two reset_done launches (mask, then mask2 on a second state for the independence of the
    draws from the mask), one all-zero launch, one vnl_env_reset."""
    dev = env.device
    st = stepped_state(env, seed)
    st.done.copy_(mask.to(device=dev, dtype=st.done.dtype))
    before = snapshot(st)
    rec0 = reset_done(env, st, torch.zeros_like(mask))
    same_rows(before, snapshot(st), torch.ones(env.num_envs, dtype=torch.bool), tuple(before))  # all-zero mask: nothing at all
    assert bool((rec0["start_frame"] == -7).all())
    rec = reset_done(env, st, mask)
    after = snapshot(st)
    check_draws(env, rec, mask)
    check_nothing_else_moves(before, after, mask)
    assert not torch.equal(before["qpos"][mask.bool()], after["qpos"][mask.bool()])  # .. and the masked envs did move
    st2 = stepped_state(env, seed + 1)
    rec2 = reset_done(env, st2, mask2)
    check_draws(env, rec2, mask2)
    both = mask.bool() & mask2.bool()
    same_rows(rec, rec2, both, ("start_frame", "clip_id", "noise"))  # an env's draws do not depend on who else resets
    check_is_the_existing_reset(env, after, rec, mask)
