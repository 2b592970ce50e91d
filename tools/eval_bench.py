"""Wall time of ONE evaluation (acting.Evaluator.run_evaluation, synchronised) by its three routes, alternated in one process:

  generic   the wrappers stepped in torch ops through acting.generate_unroll -- what every evaluation was before the scoring
            moved onto the device (a couple of dozen small launches per step and a Transition log nobody reads)
  eager     acting.evaluate_unroll: per step the policy, vnl_env_step_post_eval and, in fresh mode, vnl_env_reset_done
  graphed   the same launches, `--graph-steps` of them captured once and replayed (acting.GraphedEval)

on the rodent with episodes of `--episode-length` steps, for each of `--envs` eval envs and the two settings K = 1 from the
first state (the default evaluation) and K = 4 with the fresh auto-reset.  Prints one JSON line with the median and the
max - min spread of `--rounds` rounds per route and writes it as the section "tools/eval_bench.py" of `--out`
(profiles/eval_epilogue_bench.txt; text before the section -- the bench.py series of the training path -- is kept).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MARK = "## tools/eval_bench.py\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[128, 4096])
    ap.add_argument("--episode-length", type=int, default=200)
    ap.add_argument("--graph-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_epilogue_bench.txt"))
    args = ap.parse_args()

    import functools

    import numpy as np
    import torch

    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import wrap
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    dev = torch.device("cuda:0")
    routes = {"generic": dict(fused=False), "eager": dict(fused=True, graphed=False), "graphed": dict(fused=True, graphed=True)}
    settings = {"K1_first_state": dict(K=1, mode="first_state"), "K4_fresh": dict(K=4, mode="fresh")}

    def evaluator(B, K, mode, route):
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
        env = wrap(base, episode_length=args.episode_length, auto_reset=mode, auto_reset_seed=7)
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                        decoder_layer_sizes=(128, 256))
        params = (running_statistics.init_state(base.observation_size, device=dev),
                  nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev))
        fn = functools.partial(ppo_networks.make_inference_fn(nets), noise="device", seed=1,
                               counter=torch.zeros(1, dtype=torch.int64, device=dev))
        ev = acting.Evaluator(env, fn, num_eval_envs=B, episode_length=args.episode_length, action_repeat=1,
                              key=torch.Generator().manual_seed(2), episodes_per_env=K, graph_steps=args.graph_steps, **routes[route])
        return ev, params

    def timed(ev, params) -> float:
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        ev.run_evaluation(params, {})  # (synchronises before it reads the records)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t

    out = {"episode_length": args.episode_length, "graph_steps": args.graph_steps, "rounds": args.rounds, "seconds": {}}
    for B in args.envs:
        for name, s in settings.items():
            evs = {r: evaluator(B, s["K"], s["mode"], r) for r in routes}
            for ev, params in evs.values():  # warm-up: kernels loaded, the graph captured
                timed(ev, params)
            secs = {r: [] for r in routes}
            for _ in range(args.rounds):
                for r, (ev, params) in evs.items():  # in turn: drift of the clocks hits all alike
                    secs[r].append(timed(ev, params))
            scored = {r: int(ev.records.shape[0]) for r, (ev, _) in evs.items()}
            out["seconds"][f"envs{B}_{name}"] = {
                r: {"median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4), "all": [round(x, 4) for x in v],
                    "episodes_scored": scored[r]} for r, v in secs.items()}
            del evs
    line = json.dumps(out)
    print(line)
    head = ""
    if os.path.exists(args.out):
        head = open(args.out).read().split(MARK)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + MARK + line + "\n")


if __name__ == "__main__":
    main()
