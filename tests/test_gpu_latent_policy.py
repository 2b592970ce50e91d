"""Latent-driven acting on the device (vnl_policy_decode / vnl_policy_decode_noise, the decode kernels of csrc/vnl_policy.hip):
the decoder against its float64 restatement, row independence, the same function as the full forward pass, the drawn noise and
the prior draw against the acting kernel's and the torch restatement's, the ABI's argument errors, the two backends of
make_decoder_inference_fn, and the unroll, graph and evaluator routes of acting.py with the decoder policy."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_policy_cases as LC
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.ppo_imitation import acting, philox, ppo_networks, running_statistics

pytestmark = pytest.mark.gpu

B = 33  # two full 16-env tiles and a one-row tile
SEED, STEP, OFFSET = LC.SEED, LC.STEP, LC.OFFSET
OUTS = ("action", "raw_action", "log_prob", "rand_log_prob", "logits")


class Case(LC.Net):
    def __init__(self, name):
        from vnl_brax_imitation_amd.ppo_imitation.hip_policy import HipIntentionPolicy

        super().__init__(name)
        self.dev = dev = torch.device("cuda:0")
        self.host = {k: getattr(self, k) for k in ("flat", "traj", "obs", "z", "eps_action", "rand_action")}
        self.d_flat, self.d_mean, self.d_std = self.flat.to(dev), self.norm.mean.to(dev), self.norm.std.to(dev)
        self.d_traj, self.d_obs, self.d_z = self.traj.to(dev), self.obs.to(dev), self.z.to(dev)
        self.d_eps, self.d_rand = self.eps_action.to(dev), self.rand_action.to(dev)
        self.hp = HipIntentionPolicy(self.nets.policy_module, self.act, LC.ROWS, dev)

    def decode(self, rows=slice(0, B), z=None, eps=None, rand="given", deterministic=False):
        """one vnl_policy_decode call on the case's rows -> outputs incl. action"""
        z = self.d_z[rows] if z is None else z
        eps = self.d_eps[rows] if eps is None else eps
        rand = self.d_rand if isinstance(rand, str) else rand
        a, ex = self.hp.decode(self.d_flat, self.d_mean, self.d_std, z, self.d_obs[rows], None if deterministic else eps,
                               deterministic, rand_action=None if deterministic else rand)
        return {"action": a, **ex}

    def noise(self, rows=slice(0, B), latent="given", counter=STEP, step_offset=0, env_offset=OFFSET, deterministic=False,
              record=True):
        """one vnl_policy_decode_noise call -> (outputs incl. action, recorded draws, the counter tensor); latent=None: prior"""
        nb = self.d_obs[rows].shape[0]
        ctr = torch.tensor([counter], dtype=torch.int64, device=self.dev)
        rec = None
        if record:
            rec = {"eps_latent": torch.full((nb, self.latent), 9.0, device=self.dev),
                   "eps_action": torch.full((nb, self.act), 9.0, device=self.dev),
                   "rand_action": torch.full((self.act,), 9.0, device=self.dev)}
        z = self.d_z[rows] if isinstance(latent, str) else latent
        a, ex = self.hp.decode_noise(self.d_flat, self.d_mean, self.d_std, z, self.d_obs[rows], ctr, step_offset=step_offset,
                                     seed=SEED, env_offset=env_offset, deterministic=deterministic, eps_out=rec)
        return {"action": a, **ex}, rec, ctr

    def forward_noise(self, rows=slice(0, B)):
        """the ACTING kernel's draws at the same key: (outputs, records)"""
        nb = self.d_obs[rows].shape[0]
        ctr = torch.tensor([STEP], dtype=torch.int64, device=self.dev)
        rec = {"eps_latent": torch.full((nb, self.latent), 9.0, device=self.dev),
               "eps_action": torch.full((nb, self.act), 9.0, device=self.dev),
               "rand_action": torch.full((self.act,), 9.0, device=self.dev)}
        a, ex = self.hp.forward_noise(self.d_flat, self.d_mean, self.d_std, self.d_traj[rows], self.d_obs[rows], ctr, seed=SEED,
                                      env_offset=OFFSET, eps_out=rec)
        return {"action": a, **ex}, rec


@pytest.fixture(scope="module", params=list(LC.NETS))
def case(request):
    c = Case(request.param)
    c.out = c.decode()  # the B = 33 call several tests compare against: computed once, left unchanged
    c.f64 = c.decoder_f64(c.z.numpy(), c.obs.numpy())  # all 48 rows
    return c


def _equal(a, b, keys=OUTS):
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("nb", [1, 15, 16, 17, 33])
def test_decode_against_float64(case, nb):
    """a lone row, a tile short of one row, one tile, one tile plus a row, two tiles plus a row.  Logits <= 2e-5 absolute of
    the float64 restatement (the bound of tests/test_gpu_policy.py, whose accumulation depth K <= 1027 exceeds the decoder's
    K <= 296); raw_action / action 1e-5 and log_prob 2e-6 of its scale, in float64 on the kernel's own logits, as there."""
    rows = slice(0, nb)
    out = case.out if nb == B else case.decode(rows)
    lg = out["logits"].cpu()
    err = float(np.abs(lg.double().numpy() - case.f64[rows]).max())
    dist = case.nets.parametric_action_distribution
    raw = dist.sample_no_postprocessing(lg, case.eps_action[rows])
    e_raw = float((out["raw_action"].cpu() - raw).abs().max())
    e_act = float((out["action"].cpu() - torch.tanh(raw)).abs().max())
    lp_ref = dist.log_prob(lg.double(), out["raw_action"].cpu().double())
    e_lp = float((out["log_prob"].cpu().double() - lp_ref).abs().max() / lp_ref.abs().max())
    rlp_ref = dist.log_prob(lg.double(), case.rand_action.double().expand(nb, case.act))
    e_rlp = float((out["rand_log_prob"].cpu().double() - rlp_ref).abs().max() / rlp_ref.abs().max())
    det = case.decode(rows, deterministic=True)
    e_det = float((det["action"].cpu() - torch.tanh(lg[:, :case.act])).abs().max())
    print(f"{case.name} B={nb}: logits vs float64 {err:.2e}, raw_action {e_raw:.2e}, action {e_act:.2e}, log_prob rel "
          f"{e_lp:.2e}, rand_log_prob rel {e_rlp:.2e}, deterministic action {e_det:.2e}")
    assert err < 2e-5, err
    assert e_raw <= 1e-5 and e_act <= 1e-5, (e_raw, e_act)
    assert e_lp < 2e-6 and e_rlp < 2e-6, (e_lp, e_rlp)
    assert e_det <= 1e-5, e_det
    assert set(det) == {"action", "logits"} and torch.equal(det["logits"], out["logits"])


def test_rows_are_independent(case):
    """rows 16 and 32 of the B = 33 call == B = 1 calls on those rows with the same latent and noise rows, on every output"""
    for r in (16, 32):
        one = case.decode(slice(r, r + 1))
        _equal({k: case.out[k][r:r + 1] for k in OUTS}, one)
    assert not torch.equal(case.out["action"][16], case.out["action"][32])


def test_same_function_as_the_full_forward(case):
    """decode fed z = latent_mean + eps_latent * exp(latent_logvar / 2), in float32 torch ops from vnl_policy_forward's own
    outputs: logits within 2e-5 of that call's (the two differ by the rounding of z alone)"""
    g = torch.Generator().manual_seed(11)
    eps_l = torch.randn((B, case.latent), generator=g).to(case.dev)
    sl = slice(0, B)
    a, ex = case.hp.forward(case.d_flat, case.d_mean, case.d_std, case.d_traj[sl], case.d_obs[sl], eps_l, case.d_eps[sl],
                            False, rand_action=case.d_rand)
    z = ex["latent_mean"] + eps_l * torch.exp(0.5 * ex["latent_logvar"])
    out = case.decode(sl, z=z)
    diff = {k: float((out[k] - v).abs().max()) for k, v in (("logits", ex["logits"]), ("action", a))}
    print(f"{case.name}: decode(z of the full forward) vs vnl_policy_forward: max |d logits| = {diff['logits']:.2e}, "
          f"max |d action| = {diff['action']:.2e}")
    assert diff["logits"] <= 2e-5, diff


@pytest.mark.parametrize("deterministic", [False, True])
def test_drawn_noise_is_the_acting_kernels(case, deterministic):
    """decode_noise with a given latent: every output == decode fed the recorded draws; the records == those a forward_noise
    call leaves at the same (seed, step, env_offset); stream 0 is not drawn"""
    out, rec, ctr = case.noise(deterministic=deterministic)
    assert float(rec["eps_latent"].min()) == 9.0 == float(rec["eps_latent"].max())  # left alone
    if deterministic:
        assert float(rec["eps_action"].min()) == 9.0 and float(rec["rand_action"].min()) == 9.0
        ref = case.decode(deterministic=True)
        _equal(out, ref, ("action", "logits"))
        assert set(out) == {"action", "logits"}
    else:
        ref = case.decode(eps=rec["eps_action"], rand=rec["rand_action"])
        _equal(out, ref)
        _, frec = case.forward_noise()
        assert torch.equal(rec["eps_action"], frec["eps_action"]) and torch.equal(rec["rand_action"], frec["rand_action"])
    assert int(ctr) == STEP
    bare = case.noise(deterministic=deterministic, record=False)[0]  # the optional records null: the same outputs
    _equal(out, bare, ("action", "logits") if deterministic else OUTS)


def test_prior_draw(case):
    """latent == NULL: the recorded z == the eps_latent forward_noise records at the same key, bit for bit, and lies within
    1e-5 of philox.normal(stream 0) (the bound and derivation of test_emitted_draws_match_the_restatement: |x| <= 5.9, logf,
    sqrtf, sinf, cosf each within ~2 ulp is under ~8 ulp of 5.9 = 5.6e-6; a wrong Philox bit misses by O(1)); the outputs ==
    decode fed that z and the recorded draws"""
    out, rec, ctr = case.noise(latent=None)
    _, frec = case.forward_noise()
    for k in ("eps_latent", "eps_action", "rand_action"):
        assert torch.equal(rec[k], frec[k]), k
    ref = philox.normal(SEED, STEP, OFFSET + torch.arange(B), case.latent, philox.STREAM_LATENT)
    err = float((rec["eps_latent"].cpu().double() - ref.double()).abs().max())
    print(f"{case.name}: prior z: max |kernel - restatement| = {err:.2e}")
    assert err <= 1e-5, err
    _equal(out, case.decode(z=rec["eps_latent"], eps=rec["eps_action"], rand=rec["rand_action"]))
    assert int(ctr) == STEP
    _equal(out, case.noise(latent=None, record=False)[0])
    det, drec, _ = case.noise(latent=None, deterministic=True)  # stream 0 only
    assert torch.equal(drec["eps_latent"], rec["eps_latent"]) and float(drec["eps_action"].min()) == 9.0
    _equal(det, case.decode(z=rec["eps_latent"], deterministic=True), ("action", "logits"))


def test_prior_mode_is_independent_of_batch_size_row_and_step_split(case):
    big = case.noise(rows=slice(0, 48), latent=None, env_offset=0)[0]
    part, _, ctr = case.noise(rows=slice(32, 48), latent=None, env_offset=32)
    _equal({k: big[k][32:48] for k in OUTS}, part)
    assert not torch.equal(big["action"][:16], part["action"])
    a, _, ctr_a = case.noise(latent=None, counter=7, step_offset=3)
    b, _, ctr_b = case.noise(latent=None, counter=10, step_offset=0)
    _equal(a, b)
    assert int(ctr_a) == 7 and int(ctr_b) == 10 and int(ctr) == STEP  # the kernel leaves the counter unwritten
    assert not torch.equal(a["action"], case.noise(latent=None)[0]["action"])  # another step, other draws


def test_abi_errors(case):
    lib, hp, dev = case.hp.lib, case.hp, case.dev
    f32 = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    action = torch.full((LC.ROWS, case.act), 7.0, device=dev)
    raw, lp, logits, rlp = f32(LC.ROWS, case.act), f32(LC.ROWS), f32(LC.ROWS, 2 * case.act), f32(LC.ROWS)

    def decode(latent=case.d_z, mean=case.d_mean, std=case.d_std, batch=B):
        return lib.vnl_policy_decode(hp.h, p(case.d_flat), p(mean), p(std), p(latent), p(case.d_obs), p(case.d_eps), batch, 0,
                                     p(action), p(raw), p(lp), p(logits), p(case.d_rand), p(rlp), C.c_void_p(0))

    def decode_noise(step_base=ctr, step_offset=0, env_offset=0, mean=case.d_mean, std=case.d_std, batch=B, latent=None):
        nz = _lib.PolicyNoise()
        nz.seed, nz.step_base, nz.step_offset, nz.env_offset = 1, p(step_base), step_offset, env_offset
        return lib.vnl_policy_decode_noise(hp.h, p(case.d_flat), p(mean), p(std), p(latent), p(case.d_obs), C.byref(nz), batch,
                                           0, p(action), p(raw), p(lp), p(logits), p(rlp), C.c_void_p(0))

    bad = [(decode, dict(latent=None), "latent"), (decode, dict(mean=None), "obs_mean"), (decode, dict(std=None), "obs_std"),
           (decode, dict(batch=0), "batch"), (decode, dict(batch=LC.ROWS + 1), "batch"),
           (decode_noise, dict(std=None), "obs_std"), (decode_noise, dict(mean=None), "obs_mean"),
           (decode_noise, dict(batch=0), "batch"), (decode_noise, dict(batch=LC.ROWS + 1), "batch"),
           (decode_noise, dict(step_base=None), "step_base"), (decode_noise, dict(step_offset=-1), "negative"),
           (decode_noise, dict(env_offset=-1), "negative"), (decode_noise, dict(env_offset=2 ** 32 - 1 - B), "2^32")]
    for fn, kw, word in bad:
        rc = fn(**kw)
        msg = lib.vnl_last_error().decode()
        assert rc == -1 and word in msg, (fn.__name__, kw, rc, msg)  # VNL_ERR_ARG
    torch.cuda.synchronize()
    assert float(action.min()) == 7.0  # nothing was launched
    assert decode_noise(env_offset=2 ** 32 - 2 - B) == 0  # the largest env index allowed
    assert decode_noise(latent=case.d_z) == 0 and decode() == 0
    torch.cuda.synchronize()
    assert float(action[:B].abs().max()) <= 1.0 and float(action[B:].min()) == 7.0
    with pytest.raises(_lib.VnlError):
        case.noise(env_offset=-1)
    with pytest.raises(ValueError):
        case.hp.decode(case.d_flat, case.d_mean, case.d_std, None, case.d_obs[:B], case.d_eps[:B])


def test_backends_of_the_decoder_policy():
    """hip against torch in prior mode at B = 64 on the reference net: logits and action within 2e-4, log_prob and
    rand_log_prob within 2e-5 of their scale -- the bounds and the reasoning of test_make_policy_uses_hip_kernel_on_gpu (two
    float32 implementations of the network: the logits differ by ~5e-6, and the log-prob's sensitivity to them is
    |d log_prob / d logits| ~ z / scale, up to ~1e2 for a random action five standard deviations out)"""
    dev = torch.device("cuda:0")
    n = ppo_networks.make_intention_ppo_networks(795, 232, 30, preprocess_observations_fn=running_statistics.normalize,
                                                 intention_latent_size=64, encoder_layer_sizes=(256, 128),
                                                 decoder_layer_sizes=(128, 256))
    g = torch.Generator().manual_seed(0)
    flat = n.policy_network.init(g).to(dev)
    st = running_statistics.init_state(232, device=dev)
    mk = ppo_networks.make_decoder_inference_fn(n)
    z_hip, z_torch = torch.zeros((64, 64), device=dev), torch.zeros((64, 64), device=dev)
    pol_hip = mk((st, flat), seed=3, env_offset=100, latent_out=z_hip)
    pol_torch = mk((st, flat), seed=3, env_offset=100, backend="torch", latent_out=z_torch)
    assert pol_hip.use_hip and not pol_torch.use_hip and pol_hip.noise == pol_torch.noise == "device"
    traj = (torch.randn((64, 795), generator=g) * 0.1).to(dev)
    obs = torch.randn((64, 232), generator=g).to(dev)
    a1, e1 = pol_hip(traj, obs)
    a2, e2 = pol_torch(traj, obs)
    assert int(pol_hip.counter) == 1 == int(pol_torch.counter)
    assert set(e1) == set(e2) == {"log_prob", "rand_log_prob", "raw_action", "logits"}
    ez = float((z_hip - z_torch).abs().max())
    el, ea = float((e1["logits"] - e2["logits"]).abs().max()), float((a1 - a2).abs().max())
    print(f"hip vs torch, prior mode: z {ez:.2e}, logits {el:.2e}, action {ea:.2e}")
    assert ez <= 1e-5 and el <= 2e-4 and ea <= 2e-4, (ez, el, ea)
    for k in ("rand_log_prob", "log_prob"):
        err = float((e1[k] - e2[k]).abs().max()) / max(float(e2[k].abs().max()), 1.0)
        print(f"{k}: hip vs torch max error relative to its scale: {err:.2e}")
        assert err < 2e-5, (k, err)
    # a tensor latent is read live: rewritten in place between two calls it changes the action
    live = torch.zeros((64, 64), device=dev)
    pol = mk((st, flat), latent=live, seed=3)
    b0, _ = pol(traj, obs, advance=False)
    b0 = b0.clone()
    live.copy_(z_hip)
    b1, _ = pol(traj, obs, advance=False)
    assert not torch.equal(b0, b1) and int(pol.counter) == 0
    # a callable latent receives (traj, obs); its result drives the kernel as the same tensor given directly does
    seen = []

    def controller(t, o):
        seen.append((t, o))
        return z_hip * 0.5

    c1, ce = mk((st, flat), latent=controller, seed=3)(traj, obs)
    assert len(seen) == 1 and seen[0][0] is traj and seen[0][1] is obs
    c2, ce2 = mk((st, flat), latent=z_hip * 0.5, seed=3)(traj, obs)
    assert torch.equal(c1, c2) and torch.equal(ce["logits"], ce2["logits"])


def test_unroll_routes():
    """rodent, 64 envs, episodes of 4 steps, T = 5, decoder policy in prior mode: the generic actor_step loop, the fused eager
    loop and GraphedUnroll replayed twice give the same Transition and state leaves, bit for bit; the counter is 0 after the
    capture and 10 after two replays"""
    T, extra = 5, ("truncation", "traj")
    runs = {}
    for mode in ("fused", "generic", "graphed"):
        env, policy, state, _, _ = LC.rodent_setup(64, "cuda:0")
        assert policy.use_hip
        g = acting.GraphedUnroll(env, state, policy, None, T, extra_fields=extra) if mode == "graphed" else None
        assert int(policy.counter) == 0  # building the graph consumes no noise
        datas = []
        for _ in range(2):
            state, data = g() if g else acting.generate_unroll(env, state, policy, None, T, extra_fields=extra,
                                                               fused=mode == "fused")
            datas.append([x.clone() for x in acting._leaves(data)])
        assert int(policy.counter) == 10
        runs[mode] = (datas, [x.clone() for x in LC.state_leaves(state)])
    d0, s0 = runs["fused"]
    i_trunc = [i for i, x in enumerate(acting._leaves(data)) if x is data.extras["state_extras"]["truncation"]][0]
    assert float(d0[0][i_trunc].sum()) > 0  # episodes of 4 steps did end inside the unroll
    assert not torch.equal(d0[0][1], d0[1][1])  # the second unroll drew other actions
    for other in ("generic", "graphed"):
        d1, s1 = runs[other]
        for a_, b_ in zip(d0, d1):
            assert len(a_) == len(b_)
            for a, b in zip(a_, b_):
                assert a.shape == b.shape and torch.equal(a, b), other
        for a, b in zip(s0, s1):
            assert torch.equal(a, b), other


def test_evaluator_takes_the_decoder_policy():
    """one Evaluator.run_evaluation at 64 eval envs, episode_length 8, by the fused route (GraphedEval underneath)"""
    env, policy, _, nets, params = LC.rodent_setup(64, "cuda:0", episode_length=8)
    mk = ppo_networks.make_decoder_inference_fn(nets)
    made = []

    def policy_fn(p):
        made.append(mk(p, seed=2))
        return made[-1]

    ev = acting.Evaluator(env, policy_fn, num_eval_envs=64, episode_length=8, action_repeat=1,
                          key=torch.Generator().manual_seed(3), fused=True)
    m = ev.run_evaluation(params, {})
    assert ev._fused and ev._graph is not None  # the captured evaluation ran
    assert np.isfinite(m["eval/episode_reward"]) and m["eval/avg_episode_length"] > 0
    assert int(made[-1].counter) == 8
