"""Fresh starts on auto-reset (vnl_env_reset_done, AutoResetWrapper(mode="fresh")) on the host builds of the product source:
the in-kernel counter-based draws against ppo_imitation/philox.py, the reset against vnl_env_reset, sharding, the eager wrapper
against the fused unroll, and the argument checks of the entry point."""
import ctypes as C

import pytest
import torch

import fresh_reset_cases as F
import helpers as H
from model_cases import humanoid_env
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper, wrap
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics

B = 8
MASK = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.float32)
MASK2 = torch.tensor([0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.float32)


def _env(num_envs=B, real="float", **over):
    return H.hostsim_env(num_envs, real, reference_clip=F.three_clips(), **over)


def test_draws_reset_and_untouched_rows():
    """Items 1-3: draws == philox.reset_draws (exact integers, noise within 1e-5 noise_scale, the same whatever the mask);
    the reset == vnl_env_reset of the recorded draws, bit for bit; unmasked rows and reward / done / metrics unchanged."""
    env = _env()
    assert F.start_hi(env) == 235 and env._num_clips == 3
    F.check_items_1_to_3(env, MASK, MASK2)


def test_logs_copy_rows_of_every_env():
    env = _env()
    st = F.stepped_state(env, 5)
    obs_log, frame_log = torch.zeros_like(st.obs), torch.full_like(st.info["cur_frame"], -1)
    F.reset_done(env, st, MASK, logs=[(st.obs, obs_log), (st.info["cur_frame"], frame_log)])
    assert torch.equal(obs_log, st.obs) and torch.equal(frame_log, st.info["cur_frame"])  # post-reset values, reset or not


def test_sharding_does_not_change_the_draws_or_the_reset():
    """Item 4: one env of 8 at env_offset 0 == two envs of 4 at offsets 0 and 4, every field, bit for bit."""
    g = torch.Generator().manual_seed(9)
    sf = torch.randint(0, 200, (B,), generator=g, dtype=torch.int32)
    nz = 1e-3 * torch.randn((B, 74), generator=g)
    clip = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
    act = 0.3 * torch.randn((2, B, 30), generator=g)
    whole = _env(B)
    st = F.stepped_state(whole, 0, clip, sf, nz, act)
    rec = F.reset_done(whole, st, MASK)
    full = F.snapshot(st)
    for lo in (0, 4):
        part = _env(4)
        sl = slice(lo, lo + 4)
        sp = F.stepped_state(part, 0, clip[sl], sf[sl], nz[sl], act[:, sl])
        rp = F.reset_done(part, sp, MASK[sl], env_offset=lo)
        snap = F.snapshot(sp)
        every = torch.ones(4, dtype=torch.bool)
        F.same_rows({k: v[sl] for k, v in full.items()}, snap, every, tuple(snap))
        F.same_rows({k: v[sl] for k, v in rec.items()}, rp, MASK[sl].bool(), tuple(rp))


def _setup(make_env, device, episode_length=3, seed=77):
    base = make_env()
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1), mode="fresh", seed=seed)
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(device)
    norm = running_statistics.init_state(base.observation_size, device=device)
    return env, ppo_networks.make_inference_fn(nets)((norm, flat))


def test_eager_wrapper_equals_fused_unroll_in_fresh_mode():
    """Item 5, after tests/test_fused_rollout.py::_compare: episodes of 3 steps that end on different steps, T = 7 then 3."""
    extra = ("truncation", "traj", "cur_frame", "sub_clip_frame", "clip_id")
    dev, out = torch.device("cpu"), []
    for fused in (False, True):
        env, policy = _setup(_env, dev)
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        state.info["steps"].copy_((torch.arange(B) % 3).to(state.info["steps"].dtype))
        first = (state.info["cur_frame"].clone(), state.info["clip_id"].clone())
        key = torch.Generator(device=dev).manual_seed(11)
        state, data = acting.generate_unroll(env, state, policy, key, 7, extra_fields=extra, fused=fused)
        state, data2 = acting.generate_unroll(env, state, policy, key, 3, extra_fields=extra, fused=fused)
        out.append((state, data, data2))
    (s0, d0, e0), (s1, d1, e1) = out
    for a, b in zip(acting._leaves(d0) + acting._leaves(e0), acting._leaves(d1) + acting._leaves(e1)):
        assert a.shape == b.shape and torch.equal(a, b)
    F.same_rows(F.snapshot(s0), F.snapshot(s1), torch.ones(B, dtype=torch.bool), F.WRITTEN + F.KEPT)
    for k in ("steps", "truncation", "reset_step"):
        assert torch.equal(s0.info[k], s1.info[k]), k
    assert int(s1.info["reset_step"]) == 10
    # the episode ends are where the wrapper says, and the frame an env shows right after one is the DRAWN start frame
    sx, ended = d1.extras["state_extras"], (d1.discount == 0)
    assert ended.any(dim=1).sum() >= 3 and not bool(ended.all())  # on different steps
    for t in range(7):
        sf, clip, _ = philox.reset_draws(77, t, torch.arange(B), 74, 235, 3, 1e-3)
        m = ended[t]
        assert torch.equal(sx["cur_frame"][t][m].long(), sf[m]) and torch.equal(sx["clip_id"][t][m].long(), clip[m])
        assert bool((sx["sub_clip_frame"][t][m] == 0).all())
    assert not torch.equal(sx["cur_frame"][6], first[0] + 7)  # not the first episode carried on ..
    assert bool((sx["clip_id"][6] != first[1]).any())         # .. and at least one env changed its clip


def test_argument_errors_launch_nothing():
    """Item 6: every malformed call returns VNL_ERR_ARG and leaves the state bit-identical."""
    env = _env(4)
    st = F.stepped_state(env, 1)
    before = F.snapshot(st)
    L, p = env._L, env._ptrs(st)
    mask = torch.ones(4)
    base = torch.zeros(1, dtype=torch.int64)
    obs_log = torch.zeros_like(st.obs)  # (kept alive: the one valid call below writes it)
    log = _lib.ResetLog(st.obs.data_ptr(), obs_log.data_ptr(), st.obs.shape[1], 0)

    def call(mask_p=mask.data_ptr(), desc=True, state=True, num_logs=0, **kw):
        nz = _lib.ResetNoise(seed=1, step_base=base.data_ptr(), step_offset=0, env_offset=0, start_hi=235, noise_scale=1e-3)
        for k, v in kw.items():
            setattr(nz, k, v)
        return L.vnl_env_reset_done(env._env_h, mask_p, C.byref(nz) if desc else None, C.byref(p) if state else None,
                                    C.byref(log), num_logs, None)

    bad = [dict(mask_p=None), dict(desc=False), dict(state=False), dict(step_base=None), dict(start_hi=0), dict(start_hi=-3),
           dict(step_offset=-1), dict(env_offset=-1), dict(env_offset=(1 << 32) - 1 - 4), dict(num_logs=-1), dict(num_logs=9)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.vnl_last_error()
    assert L.vnl_env_reset_done(None, mask.data_ptr(), None, None, None, 0, None) == -1
    F.same_rows(before, F.snapshot(st), torch.ones(4, dtype=torch.bool), tuple(before))
    assert call(env_offset=(1 << 32) - 2 - 4, num_logs=1) == 0  # the largest offset allowed, one log: launched
    assert not torch.equal(before["qpos"], F.snapshot(st)["qpos"])
    assert torch.equal(obs_log, st.obs)
    with pytest.raises(ValueError, match="reset_info_on_autoreset"):
        AutoResetWrapper(EpisodeWrapper(env, 3, 1), reset_info_on_autoreset=True, mode="fresh")
    with pytest.raises(ValueError, match="unknown auto-reset mode"):
        AutoResetWrapper(EpisodeWrapper(env, 3, 1), mode="sometimes")
    with pytest.raises(ValueError, match="unknown auto-reset mode"):
        wrap(env, episode_length=3, auto_reset="sometimes")
    assert wrap(env, episode_length=3, auto_reset="fresh").mode == "fresh" and wrap(env, episode_length=3).mode == "first_state"


def test_integer_map_covers_the_reference_range():
    """Item 7, on philox.py alone: 235 = the reference's 250 - 10 - 5 start frames, over 4096 envs x 4 steps."""
    sf = torch.cat([philox.reset_draws(3, t, torch.arange(4096), 4, 235, 3, 0.0)[0] for t in range(4)])
    assert sf.dtype == torch.int64 and int(sf.min()) == 0 and int(sf.max()) == 234
    assert torch.unique(sf).numel() == 235
    n, var = sf.numel(), (235 ** 2 - 1) / 12.0  # discrete uniform on 0..234: mean 117
    assert abs(float(sf.double().mean()) - 117.0) < 4.0 * (var / n) ** 0.5


def test_fresh_reset_is_the_existing_reset_in_the_double_build():
    """Item 8: the check of item 2 with the float64 host build (draws and noise scaling in float32, stored as float64)."""
    env = _env(4, "double")
    mask = torch.tensor([1, 0, 1, 1], dtype=torch.float32)
    st = F.stepped_state(env, 2)
    rec = F.reset_done(env, st, mask)
    assert rec["noise"].dtype == torch.float64
    F.check_draws(env, rec, mask)
    F.check_is_the_existing_reset(env, F.snapshot(st), rec, mask)


def test_humanoid_and_ant_draw_from_the_range_of_their_own_reset():
    """The start frames of a fresh reset are those of the env's OWN reset: the humanoid's U[0, clip_length - episode_length -
    ref_traj_length) (its sub-clip term is off), the ant's frame 0; neither adds reset noise."""
    env = humanoid_env(8)
    assert env._start_hi() == 60 - 20 - 5
    st = env.reset(start_frame=torch.zeros(8, dtype=torch.int32))
    st = env.step(st, torch.zeros(8, env.action_size))
    rec = F.reset_done(env, st, torch.ones(8))
    sf, _, _ = philox.reset_draws(F.SEED, F.STEP_BASE + F.STEP_OFFSET, torch.arange(8), int(env.dims.nq), 35, 1, 0.0)
    assert torch.equal(rec["start_frame"].long(), sf) and torch.equal(st.info["cur_frame"].long(), sf) and int(sf.max()) > 0
    assert bool((rec["noise"] == 0).all())
    assert _env(2)._start_hi() == 235


def test_offset_near_int64_max_is_refused():
    env = _env(2)
    st = F.stepped_state(env, 1)
    before = F.snapshot(st)
    base, p = torch.zeros(1, dtype=torch.int64), env._ptrs(st)
    nz = _lib.ResetNoise(seed=1, step_base=base.data_ptr(), step_offset=0, env_offset=(1 << 63) - 1, start_hi=235, noise_scale=0.0)
    assert env._L.vnl_env_reset_done(env._env_h, torch.ones(2).data_ptr(), C.byref(nz), C.byref(p), None, 0, None) == -1
    F.same_rows(before, F.snapshot(st), torch.ones(2, dtype=torch.bool), tuple(before))


def test_checkpoint_carries_the_reset_counter(tmp_path):
    from vnl_brax_imitation_amd.ppo_imitation import checkpoint

    nets = ppo_networks.make_intention_ppo_networks(10, 12, 3, intention_latent_size=4, encoder_layer_sizes=(8,),
                                                    decoder_layer_sizes=(8,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0))
    path = checkpoint.save_params(str(tmp_path / "ck"), (running_statistics.init_state(12), flat), nets,
                                  reset_step=torch.tensor([(1 << 33) + 40]))
    assert int(checkpoint.load_params(path, nets)["reset_step"]) == (1 << 33) + 40
