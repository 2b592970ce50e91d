"""Prioritised start frames for fresh auto-resets (include/vnl.h: vnl_start_priority, vnl_start_priority_update).

A cell is `clip * start_hi + start_frame`.  The reset kernel counts, per cell, the episodes that ended and those that ended
before their sub-clip did (`ended`, `failed`), and draws the next start from the table `cdf`; `update()` turns the counters
into a new table: a cell's weight is its smoothed failure rate plus a uniform floor.  Everything stays on the device."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib


class StartPriority:
    """The table and counters of one env batch: int32 tensors of `ncell = num_clips * start_hi` 32-bit words (unsigned
    values; `ppo_imitation.philox.words_u32` reads them) on the env's device.

    `prior`: pseudo-count a of the rate (f + a) / (n + 2 a); `floor_q16`: the weight every cell has on top of its rate, in
    units of 2^-16 (6554 = 0.1); `decay_shift`: the counters are shifted right by it at each update (1 halves them: an
    exponential window; 0 keeps accumulating).

    `ended` / `failed` are what `update()` reads.  `count_ended` / `count_failed` are where the reset kernel counts: the same
    tensors, or -- `per_rank_deltas=True`, for runs of several ranks -- delta counters of this rank's own that
    `fold_counters` all-reduces into the accumulators, which are then the same on every rank, and so is the table."""

    def __init__(self, env, prior: int = 1, floor_q16: int = 6554, decay_shift: int = 1, per_rank_deltas: bool = False):
        base = getattr(env, "unwrapped", env)
        if not hasattr(base, "reset_done"):
            raise ValueError(f"{type(base).__name__} has no reset_done: start priorities need a tracking env of this library")
        if not (int(prior) >= 1 and 1 <= int(floor_q16) <= 65536 and 0 <= int(decay_shift) <= 31):
            raise ValueError("prior must be at least 1, floor_q16 in 1..65536, decay_shift in 0..31")
        self._base = base
        self.prior, self.floor_q16, self.decay_shift = int(prior), int(floor_q16), int(decay_shift)
        self.start_hi, self.num_clips = int(base._start_hi()), int(base._num_clips)
        self.ncell = self.start_hi * self.num_clips
        if self.ncell > _lib.PRIORITY_MAX_CELLS:
            raise ValueError(f"{self.num_clips} clips x {self.start_hi} start frames = {self.ncell} cells: more than the "
                             f"{_lib.PRIORITY_MAX_CELLS} the table holds")
        zeros = lambda: torch.zeros(self.ncell, dtype=torch.int32, device=base.device)  # noqa: E731
        self.cdf, self.ended, self.failed = zeros(), zeros(), zeros()
        self.count_ended, self.count_failed = (zeros(), zeros()) if per_rank_deltas else (self.ended, self.failed)
        self.update()  # zero counters: the uniform table

    def update(self) -> None:
        """counters -> table, counters decayed: one launch on the env's stream (vnl_start_priority_update)"""
        L = self._base._L
        _lib.check(L, L.vnl_start_priority_update(self.ended.data_ptr(), self.failed.data_ptr(), self.cdf.data_ptr(), self.ncell,
                                                  self.prior, self.floor_q16, self.decay_shift, self._base._stream()))

    def fold(self, group=None) -> None:
        """per-rank deltas -> the accumulators every rank shares (fold_counters); nothing to do without deltas"""
        if self.count_ended is not self.ended:
            fold_counters((self.count_ended, self.count_failed), (self.ended, self.failed), group)

    def probabilities(self) -> torch.Tensor:
        """float64 (num_clips, start_hi): each cell's width / 2^32, for logging (reads the table back)"""
        from ..ppo_imitation.philox import words_u32

        edges = torch.cat((torch.zeros(1, dtype=torch.int64), words_u32(self.cdf)[:-1], torch.tensor([1 << 32])))
        return ((edges[1:] - edges[:-1]).double() / float(1 << 32)).reshape(self.num_clips, self.start_hi)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: getattr(self, k).detach().cpu().clone() for k in ("cdf", "ended", "failed")}

    def load_state_dict(self, sd) -> None:
        for k in ("cdf", "ended", "failed"):
            v = torch.as_tensor(sd[k])
            if v.dtype != torch.int32 or tuple(v.shape) != (self.ncell,):
                raise ValueError(f"start priority {k}: expected int32 ({self.ncell},), got {v.dtype} {tuple(v.shape)}")
            getattr(self, k).copy_(v)


def fold_counters(delta, acc, group: Optional[object] = None) -> None:
    """delta, acc: tuples of int32 counter tensors (32-bit words).  All-reduces (SUM) the deltas over `group`, adds the
    sums to the accumulators -- identical on every rank before, identical after -- and zeroes the deltas.  The sum is
    formed in int64 so that no rank's partial sum wraps; the accumulators keep the low 32 bits, as the kernel's adds do."""
    import torch.distributed as dist

    for d, a in zip(delta, acc):
        wide = d.to(torch.int64) & 0xFFFFFFFF
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(wide, op=dist.ReduceOp.SUM, group=group)
        total = (a.to(torch.int64) & 0xFFFFFFFF) + wide
        a.copy_(((total + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32))
        d.zero_()
