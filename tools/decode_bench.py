"""Cost of latent-driven acting: ms per control step of a captured 20-step unroll (acting.GraphedUnroll) of 4096 rodent envs
(CG 6/6, device noise) with the full intention policy (vnl_policy_forward_noise: encoder, latent heads, decoder) and with the
decoder policy in prior mode (vnl_policy_decode_noise: z ~ N(0, I) drawn in the kernel, decoder alone).

    python tools/decode_bench.py [--envs 4096] [--unroll 20] [--replays 10] [--warmup 3] [--rounds 5] [--report FILE]

The two policies are measured in turn, `rounds` times each (W untimed + K timed graph replays between two events); medians
and the spread (max - min over the rounds) are reported.  Then the decode kernel's tile-shape candidates: the same captured
unroll of the decoder policy with 256, 512 and 1024 threads per 16-env workgroup (vnl_policy_decode_threads_), alternated over
the rounds likewise.  Prints one JSON line; `--report FILE` also writes the figures as text (profiles/latent_policy_bench.txt).

For the two policy kernels' own times take a trace of each in a run of its own (no --pmc), then hand the two
kernel-stats files to a last run, which appends the policy kernels' lines to the report:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o full -- python tools/decode_bench.py --rounds 1 --mode full
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o dec -- python tools/decode_bench.py --rounds 1 --mode decoder
    python tools/decode_bench.py --kernel-stats <full kernel_stats.csv> <dec kernel_stats.csv> --report FILE   (no GPU work)
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

THREADS = (256, 512, 1024)


def policy_kernel_lines(path: str) -> list:
    """the vnl_policy_* rows of a rocprofv3 kernel_stats csv: name (shortened), calls, average and total time"""
    out = []
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        if "vnl_policy" in name:
            short = name.split("(")[0].replace("void ", "")
            out.append(f"  {short}: calls {row.get('Calls')}, average {float(row.get('AverageNs', 'nan')) / 1e3:.2f} us, "
                       f"total {float(row.get('TotalDurationNs', 'nan')) / 1e6:.3f} ms, {row.get('Percentage')} % of the kernel time")
    return out


def commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "full", "decoder"), default="both")
    ap.add_argument("--no-candidates", action="store_true", help="skip the thread-count comparison of the decode kernel")
    ap.add_argument("--report", default=None, help="write (or, with --kernel-stats, append to) this text file")
    ap.add_argument("--kernel-stats", nargs=2, metavar=("FULL_CSV", "DECODER_CSV"), default=None)
    ap.add_argument("--commit", default=None, help="the commit the measured tree stands on (default: git rev-parse, where there is a .git)")
    args = ap.parse_args()

    if args.kernel_stats:
        lines = ["", "Policy kernels' own times, rocprofv3 --kernel-trace --stats (no --pmc), one run per policy, "
                 f"--rounds 1 ({args.warmup + args.replays} replays of {args.unroll} steps, plus the capture's warm-up unroll):"]
        for label, path in zip(("full policy", "decoder policy, prior mode"), args.kernel_stats):
            lines += [f" {label}:"] + (policy_kernel_lines(path) or ["  (no vnl_policy kernel in the trace)"])
        text = "\n".join(lines) + "\n"
        if args.report:
            with open(args.report, "a") as f:
                f.write(text)
        print(text)
        return

    import numpy as np
    import torch

    import helpers as H
    from vnl_brax_imitation_amd import _lib
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    dev = torch.device("cuda:0")
    B, T = args.envs, args.unroll
    lib = _lib.load_library()

    def capture(kind: str, threads: int | None = None):
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
        env = AutoResetWrapper(EpisodeWrapper(base, episode_length=150, action_repeat=1))
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                        decoder_layer_sizes=(128, 256))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
        norm = running_statistics.init_state(base.observation_size, device=dev)
        if kind == "full":
            policy = ppo_networks.make_inference_fn(nets)((norm, flat), noise="device")
        else:
            policy = ppo_networks.make_decoder_inference_fn(nets)((norm, flat), latent="prior")
            if threads is not None:  # the launch geometry is read at the call: the capture bakes it into the graph
                from vnl_brax_imitation_amd.ppo_imitation.hip_policy import HipIntentionPolicy

                hp = policy.hip_cache[(dev, B)] = HipIntentionPolicy(nets.policy_module, base.action_size, B, dev)
                _lib.check(lib, lib.vnl_policy_decode_threads_(hp.h, threads))
        state = env.reset(torch.Generator().manual_seed(1))
        return acting.GraphedUnroll(env, state, policy, None, T, extra_fields=("truncation", "traj"))

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

    def alternate(unrolls: dict) -> dict:
        ms = {m: [] for m in unrolls}
        for _ in range(args.rounds):
            for m, g in unrolls.items():  # in turn: drift of the clocks hits all alike
                ms[m].append(time_replays(g))
        return {m: {"median_ms": round(float(np.median(v)), 5), "spread_ms": round(max(v) - min(v), 5),
                    "rounds_ms": [round(x, 5) for x in v]} for m, v in ms.items()}

    modes = ("full", "decoder") if args.mode == "both" else (args.mode,)
    out = {"envs": B, "unroll": T, "replays": args.replays, "warmup": args.warmup, "rounds": args.rounds, "commit": args.commit or commit(),
           "ms_per_control_step": alternate({m: capture(m) for m in modes})}
    if len(modes) == 2:
        med = out["ms_per_control_step"]
        out["decoder_minus_full_ms"] = round(med["decoder"]["median_ms"] - med["full"]["median_ms"], 5)
    if args.mode != "full" and not args.no_candidates:
        out["decode_threads_ms_per_control_step"] = alternate({str(t): capture("decoder", t) for t in THREADS})
    print(json.dumps(out))
    if args.report:
        r = out["ms_per_control_step"]
        lines = [f"Latent-driven acting: captured {T}-step unroll (acting.GraphedUnroll), {B} rodent envs, CG 6/6, device noise, MI355X.",
                 f"Measured on: {out['commit']}.",
                 "Both policies are that tree's: the full policy is its acting kernel (vnl_policy_forward_noise), the decoder",
                 "policy its decode kernel in prior mode (vnl_policy_decode_noise, latent NULL).  No speed is promised.",
                 f"ms per control step (policy + env step kernel with its epilogue), {args.rounds} rounds alternated, "
                 f"{args.warmup} untimed + {args.replays} timed replays each:"]
        for m in modes:
            lines.append(f"  {m:8s} median {r[m]['median_ms']:.5f}  spread (max - min) {r[m]['spread_ms']:.5f}  rounds {r[m]['rounds_ms']}")
        if "decoder_minus_full_ms" in out:
            lines.append(f"  decoder - full: {out['decoder_minus_full_ms']:+.5f} ms per control step")
        c = out.get("decode_threads_ms_per_control_step")
        if c:
            lines += ["", "Decode kernel, threads per 16-env workgroup (the same unroll of the decoder policy, alternated likewise):"]
            for t in THREADS:
                lines.append(f"  {t:5d} threads  median {c[str(t)]['median_ms']:.5f}  spread {c[str(t)]['spread_ms']:.5f}  "
                             f"rounds {c[str(t)]['rounds_ms']}")
            lines.append("  (16 envs x 1024 threads is the acting kernel's shape; two 16-env tiles sharing one pass over the decoder's")
            lines.append("  weights: not built, unmeasured)")
        with open(args.report, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
