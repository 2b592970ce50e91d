"""Rodent rollout with the Newton solver next to CG: ms per control step of env.step (random actions, no policy), LDS per env
and occupancy, and how close each configuration's one-step result is to a CONVERGED solve.

    python tools/newton_bench.py [--envs 4096] [--steps 50] [--warmup 10] [--quality-envs 256]

Timing: W untimed + K timed steps of env.step behind the auto-reset wrappers, random actions.  Three configurations: CG 6 / 6 (the kernel specialised for the rodent), Newton 6 / 6 and Newton 1 / 4 (generic kernel,
tree-sparse Hessian).  Quality: from the same reset states and actions, one control step of each configuration on the device
against the float64 oracle run with Newton 100 / 50 (converged); per-env scaled error of qvel and qacc_warmstart (median and
90 % quantile).  Prints one JSON line."""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CONFIGS = {"cg_6_6": (0, 6, 6), "newton_6_6": (1, 6, 6), "newton_1_4": (1, 1, 4)}


def model_for(newton: int, iterations: int, ls_iterations: int):
    import helpers as H

    m = copy.deepcopy(H.model())
    m.scalars.update(solver_newton=newton, iterations=iterations, ls_iterations=ls_iterations)
    return m


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quality-envs", type=int, default=256)
    args = ap.parse_args()

    import numpy as np
    import torch

    import helpers as H
    from oracle.oracle import Oracle
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.model import blob

    dev = torch.device("cuda:0")
    B, Q = args.envs, args.quality_envs
    rng = np.random.default_rng(0)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((B, 74))).astype(np.float32)
    acts = torch.from_numpy(np.clip(0.5 * rng.standard_normal((args.warmup + args.steps, B, 30)), -1, 1).astype(np.float32)).to(dev)

    # converged reference for the quality figures: the float64 oracle, Newton 100 / 50, from the first Q envs' reset states
    conv = model_for(1, 100, 50)
    out = {"envs": B, "steps": args.steps, "warmup": args.warmup, "quality_envs": Q, "configs": {}}
    ref = None
    for name, (newton, it, ls) in CONFIGS.items():
        env = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **dict(H.env_kwargs(), model=model_for(newton, it, ls)))
        st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
        # quality: one control step from the reset state
        env.step(st, acts[0])
        torch.cuda.synchronize(dev)
        after = {k: getattr(st.pipeline_state, k)[:Q].double().cpu().numpy() for k in ("qvel", "qacc_warmstart")}
        if ref is None:
            o = Oracle(blob.to_blob(conv), "f64")
            m = env.sys
            o.bind_env(env.env_spec(), env.clip_arrays(0), int(m.scalars["nbody"]), int(m.scalars["nq"]), int(m.scalars["nv"]),
                       int(m.scalars["nu"]))
            ost = o.env_reset(sf[:Q], noise[:Q].astype(np.float64))
            ref = o.env_step(ost, acts[0][:Q].double().cpu().numpy())
        quality = {}
        for k in ("qvel", "qacc_warmstart"):
            e = np.array([H.scaled_err(after[k][i], ref[k][i]) for i in range(Q)])
            quality[k] = dict(median=float(np.median(e)), q90=float(np.quantile(e, 0.9)))
        # timing: W untimed + K timed steps of the rollout with auto-reset (as bench.py runs it: an env that ended starts
        # again, so the timed steps see live envs, not fallen ones)
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
        ms = e0.elapsed_time(e1) / args.steps
        finite = float(torch.isfinite(ws.pipeline_state.qvel).all(1).float().mean())
        d = env.dims
        out["configs"][name] = dict(iterations=it, ls_iterations=ls, solver="newton" if newton else "cg", ms_per_step=round(ms, 4),
                                    env_steps_per_s=round(B / (ms * 1e-3)), lds_bytes_per_env=int(d.workspace_floats_per_env) * 4,
                                    workgroups_per_cu=int(d.workgroups_per_cu), kernel_specialised=int(d.kernel_specialised),
                                    finite_env_fraction_after_rollout=finite, one_step_error_vs_converged=quality)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
