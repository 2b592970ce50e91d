"""Cost of recorded rollouts: wall time of acting.Evaluator.run_evaluation on the rodent, 128 eval envs, episodes of 200
steps, device-noise policy (the reference's network sizes), K = 1 from the first state --

    without a recorder, with record_envs 1 and 128, by the fused eager route and by the graphed route
        (vnl_env_record: one more launch per step, rows written on the device, one copy to the host at the end),
    and what a user could do before: the generic loop (wrappers in torch ops) with every recorded tensor cloned after every
        step, beside that loop without the clones.

    python tools/record_bench.py [--envs 128] [--episode 200] [--rounds 5] [--warmup 1]

The legs are measured in turn, `rounds` times each (the evaluators are built once; `warmup` untimed evaluations each, which
also capture the graphs); medians and the spread (max - min over the rounds) are reported, the cost of each recorder leg
against the SAME tree's recorder-free evaluation by the same route, RolloutRecorder.result() alone (the copy to the host and
the split into columns that end a recorded evaluation) and the new kernel's resource line.  Prints one JSON
line."""
from __future__ import annotations

import argparse
import functools
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def resource_line() -> dict:
    from vnl_brax_imitation_amd.csrc import build as hip_build

    path = os.path.join(os.path.dirname(hip_build.__file__), "libvnl.so.resources.txt")
    keep = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")
    if os.path.exists(path):
        for line in open(path):
            name, _, rest = line.strip().partition(" ")
            if "vnl_record_kernel" in name:
                kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
                return {k: int(v) for k, v in kv.items() if k in keep}
    return {}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=128)
    ap.add_argument("--episode", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch

    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import EvalWrapper, wrap
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    dev = torch.device("cuda:0")
    B, T = args.envs, args.episode

    def setup():
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                        decoder_layer_sizes=(128, 256))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
        norm = running_statistics.init_state(base.observation_size, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        fn = functools.partial(ppo_networks.make_inference_fn(nets), noise="device", seed=9, counter=counter)
        return base, wrap(base, episode_length=T), fn, (norm, flat)

    routes = {"eager": dict(fused=True, graphed=False), "graphed": dict(fused=True, graphed=True), "generic": dict(fused=False)}
    legs, recorders = {}, {}

    def evaluator_leg(route, record_envs):
        base, env, fn, params = setup()
        ev = acting.Evaluator(env, fn, num_eval_envs=B, episode_length=T, action_repeat=1, key=torch.Generator().manual_seed(11),
                              record_envs=record_envs, **routes[route])
        if record_envs:
            recorders[f"{route}_rec{record_envs}"] = ev._recorder
        return lambda: ev.run_evaluation(params, {})

    for route in ("eager", "graphed"):
        for n in (0, 1, B):
            legs[f"{route}_rec{n}" if n else f"{route}_none"] = evaluator_leg(route, n)
    legs["generic_none"] = evaluator_leg("generic", 0)

    def clone_leg():
        base, env, fn, params = setup()
        env = EvalWrapper(env)

        def run():
            policy = fn(params)
            st = env.reset(torch.Generator().manual_seed(11))
            rows = []
            for _ in range(T):
                a, pex = policy(st.info["traj"], st.obs, None)
                st = env.step(st, a)
                raw = st.info["_raw"]
                rows.append([t.clone() for t in (raw["cur_frame"], raw["clip_id"], st.info["steps"], st.done, st.reward,
                                                 raw["termination_error"], raw["metrics"], st.pipeline_state.raw("qpos"),
                                                 st.pipeline_state.raw("qvel"), a, pex["logits"], pex["log_prob"],
                                                 pex["rand_log_prob"])])
            out = [torch.stack(c).cpu() for c in zip(*rows)]  # (the copy to the host, as RolloutRecorder.result makes one)
            torch.cuda.synchronize(dev)
            return out

        return run

    legs["generic_clone_loop"] = clone_leg()

    def timed(fn) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():  # in turn: drift of the clocks hits all alike
            ms[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # `run_evaluation` ends with RolloutRecorder.result(): the copy of the rows to the host and their split into columns, once
    # per evaluation -- timed alone here, so that the launches' share of a recorder leg's cost can be told from it
    result_ms = {k: round(float(np.median([timed(r.result) for _ in range(args.rounds)])), 2) for k, r in recorders.items()}
    out = {"envs": B, "episode_length": T, "rounds": args.rounds,
           "run_evaluation_ms": {k: round(v, 2) for k, v in med.items()},
           "spread_ms": {k: round(max(v) - min(v), 2) for k, v in ms.items()},
           "ms_all_rounds": {k: [round(x, 2) for x in v] for k, v in ms.items()},
           "cost_ms_against_the_same_route_without_recorder": {
               k: round(med[k] - med[k.split("_")[0] + "_none"], 2) for k in med if not k.endswith("_none")},
           "cost_us_per_step": {k: round((med[k] - med[k.split("_")[0] + "_none"]) * 1e3 / T, 2)
                                for k in med if not k.endswith("_none")},
           "result_alone_ms": result_ms,
           "cost_without_result_us_per_step": {k: round((med[k] - med[k.split("_")[0] + "_none"] - result_ms[k]) * 1e3 / T, 2)
                                               for k in result_ms},
           "resources": {"vnl_record_kernel": resource_line()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
