"""Cost of the acting policy's noise: ms per control step of a captured 20-step unroll (acting.GraphedUnroll) of 4096 rodent
envs with noise="generator" (three torch RNG launches per step, five logging ops in vnl_rollout_post) and with noise="device"
(the policy kernel draws its own counter-based noise and writes the unroll's log rows itself; one counter add per unroll).

    python tools/policy_noise_bench.py [--envs 4096] [--unroll 20] [--replays 10] [--warmup 3] [--rounds 5]

The two modes are measured in turn, `rounds` times each (W untimed + K timed graph replays between two events), and the
medians and the spread (max - min over the rounds) are reported.  Prints one JSON line, with the policy kernels' resource
lines.  For the kernels' own times and the launch count per step take a trace in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/policy_noise_bench.py --rounds 1 --mode device      (or generator)
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def resource_lines() -> dict:
    from vnl_brax_imitation_amd.csrc import build as hip_build

    path = os.path.join(os.path.dirname(hip_build.__file__), "libvnl.so.resources.txt")
    keep = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")
    out = {}
    for line in open(path):
        name, _, rest = line.strip().partition(" ")
        m = re.search(r"vnl_policy_kernel_tILi(\d)E", name)
        if m:
            kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
            out["MODE " + m.group(1)] = {k: int(v) for k, v in kv.items() if k in keep}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "generator", "device"), default="both")
    args = ap.parse_args()

    import numpy as np
    import torch

    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    dev = torch.device("cuda:0")
    B, T = args.envs, args.unroll
    modes = ("generator", "device") if args.mode == "both" else (args.mode,)
    unrolls = {}
    for mode in modes:
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
        env = AutoResetWrapper(EpisodeWrapper(base, episode_length=150, action_repeat=1))
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                        decoder_layer_sizes=(128, 256))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
        norm = running_statistics.init_state(base.observation_size, device=dev)
        policy = ppo_networks.make_inference_fn(nets)((norm, flat), noise=mode)
        state = env.reset(torch.Generator().manual_seed(1))
        key = torch.Generator(device=dev).manual_seed(2)
        unrolls[mode] = acting.GraphedUnroll(env, state, policy, key, T, extra_fields=("truncation", "traj"))

    def time_replays(g) -> float:
        for _ in range(args.warmup):
            g()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.replays):
            state, _ = g()
        e1.record()
        torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(state.obs).all())
        return e0.elapsed_time(e1) / (args.replays * T)

    ms = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:  # in turn: drift of the clocks hits both alike
            ms[m].append(time_replays(unrolls[m]))
    out = {"envs": B, "unroll": T, "replays": args.replays, "rounds": args.rounds,
           "ms_per_control_step": {m: round(float(np.median(v)), 5) for m, v in ms.items()},
           "spread_ms": {m: round(max(v) - min(v), 5) for m, v in ms.items()},
           "ms_all_rounds": {m: [round(x, 5) for x in v] for m, v in ms.items()}}
    if len(modes) == 2:
        med = out["ms_per_control_step"]
        out["device_minus_generator_ms"] = round(med["device"] - med["generator"], 5)
    out["resources"] = resource_lines()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
