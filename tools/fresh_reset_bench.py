"""Cost of fresh starts on auto-reset: ms per control step of a captured 20-step unroll (acting.GraphedUnroll) of 4096 rodent
envs, CG 6 / 6, device-noise policy, with AutoResetWrapper(mode="first_state") (a done env is copied back to its cached
first state by vnl_rollout_post) and with mode="fresh" (vnl_env_reset_done after every step: a new start frame, clip and
reset noise and one forward pass for the envs that finished, a mask read and two row copies for the others).

    python tools/fresh_reset_bench.py [--envs 4096] [--unroll 20] [--replays 10] [--warmup 3] [--rounds 5] [--mode both]

The modes are measured in turn, `rounds` times each (W untimed + K timed graph replays between two events); medians and the
spread (max - min over the rounds) are reported, with the share of envs that finished per control step in the last timed
replay of every round (the mean of 1 - discount; read after the timed span) and the new kernel's resource lines.  Prints one JSON line.  With the reference's
10-frame sub-clips every env finishes at step 10 of the first unroll, and only the envs that terminate early fall out of
step afterwards: --per-step times the reset launch of every step of one eager fused unroll (event pairs) with the share of
envs it reset, and then the launch alone with 0, 1/64, 1/8 and all of the envs masked, which tells the launch of idle
workgroups from the reset envs' forward pass.

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fresh_reset_bench.py --rounds 1 --mode fresh

--start-priority: the legs are fresh mode without and with a StartPriority (envs/start_priority.py: start frame and clip
drawn from a table by a wave-wide search, the ended episodes counted by atomics; `update()` after every replay, as train()
runs it after every unroll), alternated in this one process; and the update kernel alone at 15,040 cells (64 clips x 235
frames; median of 20 launches between event pairs).

--domain-ranges: the legs are fresh mode on an identity-domain env (with_domain of the compiled values: the randomised
kernels, the tables never written) without and with ranges on all four fields (with_domain_ranges: every reset env draws its
friction, gain, damping and armature anew inside the reset launch), alternated in this one process; with --per-step the
reset launch of every step and the launch alone at fixed shares, for both.  --mode fresh_domain is the first of these legs on
its own (no new entry point is called: it also runs against an older library, for the comparison of the default paths).

--body-ranges: the legs are fresh mode on an identity-BODY-domain env (with_body_domain of the compiled values) without and
with body ranges (with_body_domain_ranges of body_domain_ranges_scaled: mass and moments x [0.7, 1.3] on the mass's uniform,
ipos -/+ 0.2 |ipos|: every reset env draws its bodies anew and folds its welded bodies in float64 inside the reset launch),
alternated in this one process; with --per-step the reset launch of every step and the launch alone at fixed shares (none,
64, 512, all envs), for both.
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
    if os.path.exists(path):
        for line in open(path):
            name, _, rest = line.strip().partition(" ")
            if "vnl_priority_kernel" in name:
                kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
                out["vnl_priority_kernel"] = {k: int(v) for k, v in kv.items() if k in keep}
            if "vnl_redraw_domain_kernel" in name:
                kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
                out["redraw_" + re.sub(r"^_Z\d+vnl_redraw_domain_kernelI|EvPK.*$", "", name)] = {k: int(v) for k, v in kv.items() if k in keep}
            if "vnl_reset_done_kernel" in name:
                kv = dict(re.findall(r"(\S[^=]*?)=(-?\d+)(?=\s|$)", rest))
                out[re.sub(r"^_Z\d+vnl_reset_done_kernelI|EvPK.*$", "", name)] = {k: int(v) for k, v in kv.items() if k in keep}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--unroll", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "first_state", "fresh", "fresh_domain"), default="both")
    ap.add_argument("--per-step", action="store_true", help="also time every control step of one eager fused unroll in fresh mode")
    ap.add_argument("--start-priority", action="store_true", help="legs: fresh mode without and with a StartPriority")
    ap.add_argument("--domain-ranges", action="store_true", help="legs: fresh mode on an identity-domain env without and with ranges")
    ap.add_argument("--body-ranges", action="store_true", help="legs: fresh mode on an identity-body-domain env without and with body ranges")
    args = ap.parse_args()

    import numpy as np
    import torch

    import helpers as H
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking
    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

    dev = torch.device("cuda:0")
    B, T = args.envs, args.unroll
    modes = ("first_state", "fresh") if args.mode == "both" else (args.mode,)
    if args.start_priority:
        modes = ("fresh", "fresh_priority")
    if args.domain_ranges:
        modes = ("fresh_domain", "fresh_ranges")
    if args.body_ranges:
        modes = ("fresh_body", "fresh_body_ranges")
    priorities = {}

    def setup(mode):
        base = RodentTracking(H.reference_clip(), num_envs=B, device=dev, **H.env_kwargs())
        if mode in ("fresh_domain", "fresh_ranges"):
            import domain_cases as D

            base = base.with_domain(D.identity(base.sys, B))
            if mode == "fresh_ranges":
                from vnl_brax_imitation_amd.envs.rodent import domain_ranges_scaled

                base = base.with_domain_ranges(domain_ranges_scaled(base.sys, friction=(0.5, 1.5), gain=(0.7, 1.3),
                                                                    damping=(0.5, 2.0), armature=(0.5, 2.0)))
        if mode in ("fresh_body", "fresh_body_ranges"):
            import body_domain_cases as BD

            base = base.with_body_domain(BD.identity(base.sys, B))
            if mode == "fresh_body_ranges":
                from vnl_brax_imitation_amd.envs.rodent import body_domain_ranges_scaled

                base = base.with_body_domain_ranges(body_domain_ranges_scaled(base.sys, mass=(0.7, 1.3), ipos=(-0.2, 0.2)),
                                                    inertia_with_mass=True)
        ep = EpisodeWrapper(base, episode_length=150, action_repeat=1)
        # (the default mode is constructed as before the keyword existed: this file also runs against an older library)
        if mode == "fresh_priority":
            from vnl_brax_imitation_amd.envs.start_priority import StartPriority

            priorities[mode] = StartPriority(base)
            env = AutoResetWrapper(ep, mode="fresh", seed=7, start_priority=priorities[mode])
        else:
            env = AutoResetWrapper(ep) if mode == "first_state" else AutoResetWrapper(ep, mode="fresh", seed=7)
        nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                        preprocess_observations_fn=running_statistics.normalize,
                                                        intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                        decoder_layer_sizes=(128, 256))
        flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(dev)
        norm = running_statistics.init_state(base.observation_size, device=dev)
        policy = ppo_networks.make_inference_fn(nets)((norm, flat), noise="device")
        return env, policy, env.reset(torch.Generator().manual_seed(1))

    unrolls = {}
    for mode in modes:
        env, policy, state = setup(mode)
        unrolls[mode] = acting.GraphedUnroll(env, state, policy, None, T, extra_fields=("truncation", "traj"))

    done_share = {m: [] for m in modes}

    def time_replays(mode) -> float:
        g, prio = unrolls[mode], priorities.get(mode)
        for _ in range(args.warmup):
            g()
            if prio is not None:
                prio.update()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        share = torch.zeros((), device=dev)
        e0.record()
        for _ in range(args.replays):
            state, data = g()
            if prio is not None:
                prio.update()
        e1.record()
        share += (1 - data.discount).mean()  # (outside the timed span) the share of envs that finished per step, last replay
        torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(state.obs).all())
        done_share[mode].append(float(share))
        return e0.elapsed_time(e1) / (args.replays * T)

    ms = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:  # in turn: drift of the clocks hits both alike
            ms[m].append(time_replays(m))
    out = {"envs": B, "unroll": T, "replays": args.replays, "rounds": args.rounds,
           "ms_per_control_step": {m: round(float(np.median(v)), 5) for m, v in ms.items()},
           "spread_ms": {m: round(max(v) - min(v), 5) for m, v in ms.items()},
           "ms_all_rounds": {m: [round(x, 5) for x in v] for m, v in ms.items()},
           "share_of_envs_reset_per_step": {m: round(float(np.mean(v)), 5) for m, v in done_share.items()}}
    med = out["ms_per_control_step"]
    if args.start_priority:
        out["priority_minus_fresh_ms"] = round(med["fresh_priority"] - med["fresh"], 5)
        prio = priorities["fresh_priority"]
        out["episodes_counted_in_window"] = int(prio.ended.sum())
        out["largest_cell_probability_times_ncell"] = round(float(prio.probabilities().max()) * prio.ncell, 3)
        # the update kernel alone at 64 clips x 235 frames
        from vnl_brax_imitation_amd import _lib

        L, n = _lib.load_library(), 64 * 235
        gen = torch.Generator(device=dev).manual_seed(3)
        ended = torch.randint(0, 1000, (n,), generator=gen, device=dev, dtype=torch.int32)
        failed = (ended.float() * torch.rand(n, generator=gen, device=dev)).to(torch.int32)
        cdf = torch.zeros_like(ended)
        us = []
        for k in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L, L.vnl_start_priority_update(ended.data_ptr(), failed.data_ptr(), cdf.data_ptr(), n, 1, 6554, 0,
                                                      torch.cuda.current_stream(dev).cuda_stream))
            e1.record()
            torch.cuda.synchronize(dev)
            us.append(e0.elapsed_time(e1) * 1e3)
        out["update_kernel_us_at_15040_cells"] = round(float(np.median(us[3:])), 1)
    elif args.body_ranges:
        out["body_ranges_minus_body_domain_ms"] = round(med["fresh_body_ranges"] - med["fresh_body"], 5)
    elif args.domain_ranges:
        out["ranges_minus_domain_ms"] = round(med["fresh_ranges"] - med["fresh_domain"], 5)
    elif len(modes) == 2:
        out["fresh_minus_first_state_ms"] = round(med["fresh"] - med["first_state"], 5)
    for leg in [m for m in modes if m != "first_state" and m != "fresh_priority"] if args.per_step else ():
        # where the time goes: one eager fused unroll, an event pair around the reset launch of every step -- steps on which
        # (nearly) nobody resets show the launch of empty workgroups, the others the reset envs' forward pass
        env, policy, state = setup(leg)
        tag = "" if leg == "fresh" else "_" + leg
        base = env.unwrapped
        real = base.reset_done
        spans = []

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(*a, **kw)
            e1.record()
            spans.append((e0, e1))
            return r

        base.reset_done = timed
        for _ in range(2):  # the second unroll is the one reported (kernels loaded, envs past their first sub-clip)
            spans.clear()
            state, data = acting.generate_unroll(env, state, policy, None, T, extra_fields=("truncation", "traj"), fused=True)
            torch.cuda.synchronize(dev)
            rows = [(round(a.elapsed_time(b) * 1e3, 1), round(float((1 - data.discount[t]).mean()), 4))
                    for t, (a, b) in enumerate(spans)]
        base.reset_done = real
        out["reset_launch_us_and_share_by_step" + tag] = rows
        # .. and the launch alone at fixed shares (median of 20 launches, the two logs of the unroll): share 0 is the cost of
        # 4096 workgroups that read a mask word and copy two rows
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        logs = [(state.obs, torch.empty_like(state.obs)), (state.info["traj"], torch.empty_like(state.info["traj"]))]
        alone = {}
        for share in (0.0, 64.0 / B, 512.0 / B, 1.0) if args.body_ranges else (0.0, 1.0 / 64, 0.125, 1.0):
            mask = (torch.arange(B, device=dev) < round(share * B)).float()
            us = []
            for k in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                base.reset_done(state, mask, seed=7, step_base=counter, step_offset=k, logs=logs)
                e1.record()
                torch.cuda.synchronize(dev)
                us.append(e0.elapsed_time(e1) * 1e3)
            alone[f"{share:.4f}"] = round(float(np.median(us[3:])), 1)
        out["reset_launch_alone_us_by_share" + tag] = alone
    out["resources"] = resource_lines()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
