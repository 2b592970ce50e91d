"""Cost of domain randomisation (RodentTracking.with_domain, with_body_domain): ms per control step of env.step at 4096 envs for the rodent
with CG 6 / 6 (the kernel specialised for the rodent) and Newton 6 / 6 (generic kernel, tree-sparse Hessian), each without a
domain, with the identity domain (the compiled values: the randomised instantiation on the unrandomised numbers) and with a
random domain (friction x U[0.4, 1.6], gain x U[0.7, 1.3], damping and armature x U[0.5, 2]), with the identity and a random
body domain (mass x U[0.7, 1.3], moments x that x U[0.8, 1.25], ipos + U[-0.2, 0.2] |ipos|) and with both random parts; then
the compiler's resource lines of the env kernels (VGPRs, SGPR spill, scratch, LDS).

    python tools/domain_bench.py [--envs 4096] [--steps 50] [--warmup 10] [--rounds 3]

Timing as tools/newton_bench.py: W untimed + K timed steps of env.step behind the auto-reset wrappers, random actions; the
three cases of a solver are measured in turn, `rounds` times, and the median is reported.  Prints one JSON line."""
from __future__ import annotations

import argparse
import copy
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SOLVERS = {"cg_6_6": 0, "newton_6_6": 1}


def resource_lines() -> dict:
    from vnl_brax_imitation_amd.csrc import build as hip_build

    path = os.path.join(os.path.dirname(hip_build.__file__), "libvnl.so.resources.txt")
    keep = ("VGPRs", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    out = {}
    for line in open(path):
        name, _, rest = line.strip().partition(" ")
        if not any(k in name for k in hip_build.ENV_KERNELS):
            continue
        kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
        out[name] = {k: int(v) for k, v in kv.items() if k in keep}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    import body_domain_cases as BD
    import domain_cases as D
    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper

    dev = torch.device("cuda:0")
    B = args.envs
    rng = np.random.default_rng(0)
    acts = torch.from_numpy(np.clip(0.5 * rng.standard_normal((args.warmup + args.steps, B, 30)), -1, 1).astype(np.float32)).to(dev)

    def time_steps(env) -> float:
        wenv = AutoResetWrapper(EpisodeWrapper(env, episode_length=150, action_repeat=1))
        ws = wenv.reset(torch.Generator().manual_seed(1))
        for k in range(args.warmup):
            ws = wenv.step(ws, acts[k])
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(args.steps):
            ws = wenv.step(ws, acts[args.warmup + k])
        e1.record()
        torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(ws.pipeline_state.qvel).all())
        return e0.elapsed_time(e1) / args.steps

    out = {"envs": B, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "solvers": {}}
    for name, newton in SOLVERS.items():
        m = copy.deepcopy(H.model())
        m.scalars.update(solver_newton=newton, iterations=6, ls_iterations=6)
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **dict(H.env_kwargs(), model=m))
        envs = {"none": base, "identity": base.with_domain(D.identity(m, B)), "random": base.with_domain(D.random_domain(m, B, 0)),
                "body_identity": base.with_body_domain(BD.identity(m, B)),
                "body_random": base.with_body_domain(BD.random_body_domain(m, B, 0))}
        envs["both_random"] = envs["random"].with_body_domain(BD.random_body_domain(m, B, 0))
        ms = {k: [] for k in envs}
        for _ in range(args.rounds):
            for k, env in envs.items():
                ms[k].append(time_steps(env))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out["solvers"][name] = dict(
            kernel_specialised=int(base.dims.kernel_specialised),
            ms_per_step={k: round(v, 4) for k, v in med.items()},
            ms_per_step_all_rounds={k: [round(x, 4) for x in v] for k, v in ms.items()},
            ratio_to_none={k: round(v / med["none"], 4) for k, v in med.items()})
    out["resources"] = resource_lines()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
