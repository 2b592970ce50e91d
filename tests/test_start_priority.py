"""Prioritised start frames on the host builds of the product source: the weighted draws and the outcome counters of
vnl_env_reset_done_weighted, the table update, sharding, the eager wrapper against the fused unroll, the checkpoint and the
fold of per-rank counters.  (In the host build the update entry is a serial loop: this tier tests its arithmetic, the GPU
tier the kernel.)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import fresh_reset_cases as F
import helpers as H
import start_priority_cases as S
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.start_priority import StartPriority, fold_counters
from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper, wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, checkpoint, philox, ppo_networks, running_statistics

B = 8
MASK = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.float32)


def _env(num_envs=B, real="float", **over):
    return H.hostsim_env(num_envs, real, reference_clip=F.three_clips(), **over)


def test_weighted_draws_reset_and_null_descriptor():
    """Checks 1, 2 and 4 at 8 envs, three clips: 705 cells."""
    env = _env()
    assert S.ncells(env) == 705
    S.check_draws_and_reset(env, MASK)


def test_ant_cells_are_clips():
    """AntTracking starts every episode at frame 0: start_hi == 1, a cell is a clip (checks 1 to 4)."""
    env = S.ant_env(B)
    assert env._start_hi() == 1 and S.ncells(env) == 3
    S.check_draws_and_reset(env, MASK)
    S.check_counters(env)


def test_counters_equal_the_bincounts():
    """Check 3: 8 envs on 4 cells, sub_clip_length 2."""
    S.check_counters(_env(sub_clip_length=2))


def test_update_equals_its_integer_restatement():
    """Check 5 (the host build's serial loop)."""
    S.check_update(H.hostsim_library(), "cpu")


def test_restatement_by_hand():
    """philox.start_priority_table against numbers worked out by hand: two cells, prior 1, floor 1, no decay."""
    # cell 0: n = 2, f = 0 -> s = (1 << 16) // 4 = 16384, t = 16385; cell 1: n = 2, f = 2 -> s = (3 << 16) // 4 = 49152, t = 49153
    cdf, e, f = philox.start_priority_table(torch.tensor([2, 2]), torch.tensor([0, 2]), prior=1, floor_q16=1, decay_shift=0)
    assert cdf.tolist() == [(16385 << 32) // 65538, 0xFFFFFFFF] and e.tolist() == [2, 2] and f.tolist() == [0, 2]
    cells = philox.weighted_cells(1, 2, torch.arange(2000), S.as_words(cdf))
    share = float((cells == 1).double().mean())
    assert abs(share - 49153 / 65538) < 4 * (0.75 * 0.25 / 2000) ** 0.5  # three quarters of the draws go to the failing cell


def test_argument_errors_launch_nothing():
    """Check 6: every malformed call returns the stated code and leaves state, table and counters as they were."""
    env = _env(4)
    st = F.stepped_state(env, 1)
    before = F.snapshot(st)
    L, p = env._L, env._ptrs(st)
    mask, base = torch.ones(4), torch.zeros(1, dtype=torch.int64)
    n = S.ncells(env)
    cdf = S.tables(n)["uniform"]
    ended, failed = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    big = torch.zeros(32769, dtype=torch.int32)

    def call(**kw):
        nz = _lib.ResetNoise(seed=1, step_base=base.data_ptr(), step_offset=0, env_offset=0, start_hi=235, noise_scale=1e-3)
        d = dict(cdf=cdf.data_ptr(), ncell=n, ended=ended.data_ptr(), failed=failed.data_ptr(), truncation=None)
        d.update(kw)
        pr = _lib.StartPriorityDesc(**d)
        return L.vnl_env_reset_done_weighted(env._env_h, mask.data_ptr(), C.byref(nz), C.byref(pr), C.byref(p), None, 0, None)

    bad = [(dict(cdf=None), -1), (dict(ncell=n - 1), -1), (dict(ncell=n + 1), -1), (dict(ncell=0), -1), (dict(ended=None), -1),
           (dict(failed=None), -1), (dict(cdf=big.data_ptr(), ncell=32769), -5)]
    for kw, code in bad:
        assert call(**kw) == code, kw
        assert L.vnl_last_error()
    F.same_rows(before, F.snapshot(st), torch.ones(4, dtype=torch.bool), tuple(before))
    assert int(ended.abs().sum()) == 0 and int(failed.abs().sum()) == 0
    assert call() == 0 and call(ended=None, failed=None) == 0  # .. and the well-formed calls launch
    assert not torch.equal(before["qpos"], F.snapshot(st)["qpos"]) and int(ended.sum()) == 4
    S.check_update_argument_errors(L, "cpu")
    with pytest.raises(ValueError, match="start_priority needs mode='fresh'"):
        AutoResetWrapper(EpisodeWrapper(env, 3, 1), start_priority=StartPriority(env))
    with pytest.raises(ValueError, match="start_priority needs mode='fresh'"):
        wrap(env, episode_length=3, start_priority=StartPriority(env))
    assert wrap(env, episode_length=3, auto_reset="fresh", start_priority=StartPriority(env)).start_priority is not None
    with pytest.raises(ValueError, match="needs auto_reset='fresh'"):
        from vnl_brax_imitation_amd.ppo_imitation import train as ppo

        ppo.train(environment=env, num_timesteps=1, episode_length=3, num_envs=4, start_priority=True)


def test_sharding_does_not_change_draws_or_counters():
    """Check 7: one env of 8 at env_offset 0 == two envs of 4 at offsets 0 and 4: the draws, and the counters summed."""
    whole = _env(B, sub_clip_length=2)
    n = S.ncells(whole)
    cdf = S.tables(n, 5)["min_width"]
    st, mask, trunc, ended, failed = S.counter_case(whole)
    raw = {k: st.info["_raw"][k].clone() for k in ("cur_frame", "sub_clip_frame", "clip_id")}
    prio = S.priority(whole, cdf)
    rec = S.reset_done(whole, st, mask, prio, trunc)
    total_e, total_f = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    for lo in (0, 4):
        part, sl = _env(4, sub_clip_length=2), slice(lo, lo + 4)
        sp = F.stepped_state(part, 1)
        for k, v in raw.items():  # (the counters read these three rows of the old episode and nothing else)
            sp.info["_raw"][k].copy_(v[sl])
        pp = S.priority(part, cdf)
        rp = S.reset_done(part, sp, mask[sl], pp, trunc[sl], env_offset=lo)
        F.same_rows({k: v[sl] for k, v in rec.items()}, rp, mask[sl].bool(), tuple(rp))
        total_e += pp.count_ended
        total_f += pp.count_failed
    assert torch.equal(total_e, prio.count_ended) and torch.equal(total_f, prio.count_failed)
    assert torch.equal(prio.count_ended.long(), ended) and torch.equal(prio.count_failed.long(), failed)


def _setup(episode_length=4, seed=77):
    base = _env(sub_clip_length=3)
    prio = StartPriority(base, decay_shift=0)
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1), mode="fresh", seed=seed,
                           start_priority=prio)
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0))
    norm = running_statistics.init_state(base.observation_size)
    return env, prio, ppo_networks.make_inference_fn(nets)((norm, flat))


def test_eager_wrapper_equals_fused_unroll_with_a_priority():
    """Check 8, after test_eager_wrapper_equals_fused_unroll_in_fresh_mode: T = 7, update(), T = 3; episodes end at the
    sub-clip's 3 frames (counted) and, for the envs that begin with two steps on their clock, at the wrapper's 4 steps
    (truncated: not counted)."""
    extra = ("truncation", "traj", "cur_frame", "sub_clip_frame", "clip_id")
    out = []
    for fused in (False, True):
        env, prio, policy = _setup()
        uniform = prio.cdf.clone()
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        state.info["steps"].copy_((torch.arange(B) % 3).to(state.info["steps"].dtype))
        key = torch.Generator().manual_seed(11)
        state, data = acting.generate_unroll(env, state, policy, key, 7, extra_fields=extra, fused=fused)
        mid = (prio.ended.clone(), prio.failed.clone())
        prio.update()
        table = prio.cdf.clone()
        state, data2 = acting.generate_unroll(env, state, policy, key, 3, extra_fields=extra, fused=fused)
        out.append((state, data, data2, mid, table, prio))
        assert int(mid[0].sum()) > 0 and not torch.equal(table, uniform)
        # the first unroll's draws follow the uniform table, the second one's the updated one
        sx, ended = data.extras["state_extras"], (data.discount == 0)
        for t in range(7):
            cells = philox.weighted_cells(77, t, torch.arange(B), uniform)
            m = ended[t]
            assert torch.equal(sx["cur_frame"][t][m].long(), (cells % prio.start_hi)[m])
            assert torch.equal(sx["clip_id"][t][m].long(), (cells // prio.start_hi)[m])
        sx, ended = data2.extras["state_extras"], (data2.discount == 0)
        for t in range(3):
            cells = philox.weighted_cells(77, 7 + t, torch.arange(B), table)
            m = ended[t]
            assert torch.equal(sx["cur_frame"][t][m].long(), (cells % prio.start_hi)[m])
    (s0, d0, e0, m0, t0, p0), (s1, d1, e1, m1, t1, p1) = out
    for a, b in zip(acting._leaves(d0) + acting._leaves(e0), acting._leaves(d1) + acting._leaves(e1)):
        assert a.shape == b.shape and torch.equal(a, b)
    F.same_rows(F.snapshot(s0), F.snapshot(s1), torch.ones(B, dtype=torch.bool), F.WRITTEN + F.KEPT)
    for a, b in zip(m0 + (t0, p0.ended, p0.failed, p0.cdf), m1 + (t1, p1.ended, p1.failed, p1.cdf)):
        assert torch.equal(a, b)
    # truncated ends are not counted: fewer counted episodes than ended ones
    n_ended = int((d0.discount == 0).sum() + (e0.discount == 0).sum())
    n_trunc = int(d0.extras["state_extras"]["truncation"].sum() + e0.extras["state_extras"]["truncation"].sum())
    assert n_trunc > 0 and int(p0.ended.sum()) == n_ended - n_trunc


def test_probabilities_and_state_dict():
    env = _env(2)
    prio = StartPriority(env)
    p = prio.probabilities()
    assert p.shape == (3, 235) and p.dtype == torch.float64 and abs(float(p.sum()) - 1.0) < 1e-12
    assert float((p - 1 / 705).abs().max()) < 2.0 ** -31
    prio.ended[5], prio.failed[5] = 9, 9
    prio.update()
    assert int(prio.probabilities().argmax()) == 5 and int(prio.ended[5]) == 4  # (decay_shift 1)
    other = StartPriority(env)
    other.load_state_dict(prio.state_dict())
    for k in ("cdf", "ended", "failed"):
        assert torch.equal(getattr(other, k), getattr(prio, k))
    with pytest.raises(ValueError):
        other.load_state_dict({k: v[:-1] for k, v in prio.state_dict().items()})


def test_checkpoint_round_trip(tmp_path):
    """Check 9: the three tensors come back bit for bit (words above 2^31 included)."""
    nets = ppo_networks.make_intention_ppo_networks(10, 12, 3, intention_latent_size=4, encoder_layer_sizes=(8,),
                                                    decoder_layer_sizes=(8,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0))
    ended, failed = S.update_counters(705, 2)
    sd = {"cdf": S.tables(705)["min_width"], "ended": ended, "failed": failed}
    assert int(sd["cdf"].min()) < 0 and int(ended.min()) < 0
    path = checkpoint.save_params(str(tmp_path / "ck"), (running_statistics.init_state(12), flat), nets, start_priority=sd)
    back = checkpoint.load_params(path, nets)["start_priority"]
    for k, v in sd.items():
        assert back[k].dtype == torch.int32 and torch.equal(back[k], v), k
    assert "start_priority" not in checkpoint.load_params(
        checkpoint.save_params(str(tmp_path / "ck2"), (running_statistics.init_state(12), flat), nets), nets)


def test_fold_counters_single_process():
    delta = (S.as_words([1, 2, 3]), S.as_words([0, 1, 0]))
    acc = (S.as_words([10, (1 << 32) - 1, 1 << 31]), S.as_words([5, 5, 5]))
    fold_counters(delta, acc)
    assert philox.words_u32(acc[0]).tolist() == [11, 1, (1 << 31) + 3] and acc[1].tolist() == [5, 6, 5]
    assert int(delta[0].abs().sum()) == 0 and int(delta[1].abs().sum()) == 0


def test_fold_counters_two_ranks():
    """Check 10: two gloo processes; both end with equal accumulators that are the sum, and zero deltas."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29613", os.path.join(H.ROOT, "tests", "start_priority_fold_worker.py")]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = [json.loads(m) for m in re.findall(r"RESULT (\{.*?\})(?=\s|RESULT|$)", p.stdout)]
    assert len(res) == 2 and {r["rank"] for r in res} == {0, 1}
    want_e = [7 + 1 + 11, 0 + 2 + 12, (-6 + 3 + 13) % (1 << 32)]  # (32-bit words: the last one wraps)
    for r in res:
        assert r["ended"] == want_e and r["failed"] == [1 + 1, 0, 1] and r["delta_zero"]
