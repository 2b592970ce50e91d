"""Worker for tests/test_start_priority.py::test_fold_counters_two_ranks: 2 ranks, gloo.  Each rank holds delta counters of
its own and accumulators equal on both; fold_counters must leave equal accumulators = old + the sum of the deltas."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import start_priority_cases as S  # noqa: E402
from vnl_brax_imitation_amd.envs.start_priority import fold_counters  # noqa: E402
from vnl_brax_imitation_amd.ppo_imitation.philox import words_u32  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    delta = (S.as_words([1, 2, 3] if rank == 0 else [11, 12, 13]), S.as_words([1, 0, 0] if rank == 0 else [1, 0, 1]))
    acc = (S.as_words([7, 0, (1 << 32) - 6]), S.as_words([0, 0, 0]))
    fold_counters(delta, acc)
    out = dict(rank=rank, ended=words_u32(acc[0]).tolist(), failed=words_u32(acc[1]).tolist(),
               delta_zero=bool(int(delta[0].abs().sum()) == 0 and int(delta[1].abs().sum()) == 0))
    print("RESULT " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
