"""Newton solver with the tree-sparse Hessian (EnvWaveT::newton_hessian / newton_solve, csrc/vnl_body.h), the one Newton
solver of the library: the rodent (nv 73, nefc 303), the ant and the humanoid.

CPU tier: the float64 host build of the product source against the dense float64 oracle (whose Newton branch has no size
limit), the assembled Hessian against a NumPy one, the ant and the humanoid.  GPU tier: the rodent on the device against the
float64 / float32 oracles following the product's decisions, determinism, graph capture and a short training run (the ant's
Newton on the device: tests/test_ant_env.py::test_ant_env_newton_on_gpu)."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import hostsim_cases as HP
import model_cases as M
import parity as P
from model_cases import newton_model
from model_cases import rodent_env as _rodent
from vnl_brax_imitation_amd import configs, envs

CONFIGS = [(6, 6), (1, 4)]  # CG's counts, and the reference's Newton counts (configs/env_config.yaml:16-21)


def _sections(env):
    env.debug(True)
    return env


# ------------------------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("it,ls", CONFIGS)
def test_rodent_newton_float64_build_matches_oracle(it, ls):
    B = 16
    env = _rodent(B, newton_model(it, ls))
    sf, noise, acts = HP.parity_inputs(B)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    o = H.make_oracle(env, "f64")
    ost = o.env_reset(sf, noise)
    e = HP.parity_errors(st, ost, B)
    assert max(e.values()) < 1e-11, e
    st = env.step(st, torch.from_numpy(acts[0]))
    o.env_step(ost, acts[0])
    e = HP.parity_errors(st, ost, B)
    assert max(e.values()) < 1e-8, e  # the bound the CG route is held to (test_hostsim_parity)
    assert np.array_equal(st.done.numpy(), ost["done"])
    m = np.stack([st.metrics[k].numpy() for k in st.metrics], 1)
    assert np.abs(m - ost["metrics"]).max() < 1e-10
    # a different algorithm than CG with the same counts, not a no-op
    env_cg = H.hostsim_env(B, "double", iterations=it, ls_iterations=ls)
    sc = env_cg.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    sc = env_cg.step(sc, torch.from_numpy(acts[0]))
    assert float((sc.pipeline_state.qvel - st.pipeline_state.qvel).abs().max()) > 1e-6


def test_rodent_newton_takes_the_tree_sparse_route():
    env = _sections(_rodent(1, newton_model(1, 4)))
    env.reset(0)
    assert env.scratch("newton_LD").shape == (1, 1119) and env.scratch("newton_LDiagInv").shape == (1, 73)  # nM, nv
    with pytest.raises(Exception):
        env.scratch("newton_efc_J")  # no dense Jacobian
    lds = int(env.dims.workspace_floats_per_env) * 4
    assert lds <= 32 * 1024, lds  # five workgroups per CU (160 KiB of LDS)


def test_rodent_newton_tree_hessian_assembly():
    """The Hessian the kernel factorised, rebuilt from its inverted L'DL factor in the debug image, against NumPy's
    qM + J' diag(D * (Jaref < 0)) J with qM / efc_J from the oracle at the same state and efc_D / Jaref from the image."""
    env = _sections(_rodent(1, newton_model(6, 6)))
    sf, noise, _ = HP.parity_inputs(1, seed=7)
    env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    o = H.make_oracle(env, "f64")
    c = env.clip_arrays(0)
    f = int(sf[0])
    o.set(qpos=np.concatenate([c["position"][f], c["quaternion"][f], c["joints"][f]]) + noise[0],
          qvel=np.concatenate([c["velocity"][f], c["angular_velocity"][f], c["joints_velocity"][f]]),
          act=np.zeros(30), ctrl=np.zeros(30), qacc_warmstart=np.zeros(73))
    o.call("forward")
    nv, ne = 73, 303
    M, J = o.field("qM").reshape(nv, nv), o.field("efc_J").reshape(ne, nv)
    D = np.abs(env.scratch("efc_D")[0].numpy())  # limit rows carry the Jacobian's sign on D
    Jaref = env.scratch("Jaref")[0].numpy()
    act = (D != 0) & (Jaref < 0)
    assert act.sum() >= 4  # contacts are active: the contact part of the assembly is exercised
    Href = M + (J.T * (D * act)) @ J
    # the image holds N = L^-1 (unit lower, ancestor pattern) and 1/D of H = L' D L
    par = env.sys.dof_parentid
    LD, dinv = env.scratch("newton_LD")[0].numpy(), env.scratch("newton_LDiagInv")[0].numpy()
    N, k = np.eye(nv), 0
    for i in range(nv):
        j = i
        while j >= 0:
            if j != i:
                N[i, j] = LD[k]
            k += 1
            j = par[j]
    assert k == len(LD)
    L = np.linalg.inv(N)
    Hk = L.T @ np.diag(1.0 / dinv) @ L
    err = np.abs(Hk - Href).max() / np.abs(Href).max()
    assert err < 1e-12, err
    # qM kept beside it for M * search
    Mk = env.scratch("newton_qM")[0].numpy()
    k = 0
    for i in range(nv):
        j = i
        while j >= 0:
            assert abs(Mk[k] - M[i, j]) <= 1e-12 * np.abs(M).max()
            k += 1
            j = par[j]


def _ant_env(B):
    return M.ant_env(B, "double", params=M.NEWTON)


def _humanoid_env(B):
    return M.humanoid_newton_env(B, "double")


@pytest.mark.parametrize("which", ["ant", "humanoid"])
def test_small_models_newton_float64_build_matches_oracle(which):
    """The ant (its welded bodies folded) and the humanoid (eulerdamp off) with Newton 1 / 4: four control steps against the
    oracle, whose dense Cholesky is the independent check of the tree-sparse factorisation."""
    B = 6
    env = (_ant_env if which == "ant" else _humanoid_env)(B)
    env.debug(True)
    nu, nq = env.action_size, int(env.sys.scalars["nq"])
    sf = np.random.default_rng(5).integers(0, 30, B).astype(np.int32)
    st = env.reset(start_frame=torch.from_numpy(sf))
    o = H.make_oracle(env)
    ost = o.env_reset(sf, np.zeros((B, nq)))
    rng = np.random.default_rng(4)
    moved = 0.0
    for _ in range(4):
        a = np.clip(0.5 * rng.standard_normal((B, nu)), -1, 1)
        st = env.step(st, torch.from_numpy(a))
        o.env_step(ost, a)
        for k in ("qpos", "qvel", "qacc_warmstart"):
            x = getattr(st.pipeline_state, k).numpy()
            assert H.scaled_err(x, ost[k]) < 1e-9, (k, H.scaled_err(x, ost[k]))
        assert np.array_equal(st.done.numpy(), ost["done"])
        moved = max(moved, float(np.abs(st.pipeline_state.qvel.numpy()).max()))
    assert moved > 1e-2


def test_public_constructors_accept_newton_for_the_rodent():
    """solver="newton" without model=: the packaged compiled model through _load_model, as the reference's keyword."""
    from vnl_brax_imitation_amd.envs.rodent import RodentMultiClipTracking, RodentTracking

    B = 2
    kw = dict(configs.RODENT_ENV_ARGS, solver="newton", iterations=1, ls_iterations=4)
    with H.hostsim_backend("double"):
        a = RodentTracking(H.reference_clip(), num_envs=B, device="cpu", **kw)
        b = envs.get_environment("rodent", reference_clip=H.reference_clip(), num_envs=B, device="cpu", **kw)
        c = RodentMultiClipTracking(H.reference_clip(), num_envs=B, device="cpu", **kw)
    assert int(a.sys.scalars["solver_newton"]) == 1 and int(a.sys.scalars["iterations"]) == 1
    ref = _rodent(B, newton_model(1, 4))
    act = torch.from_numpy(np.clip(0.3 * np.random.default_rng(0).standard_normal((B, 30)), -1, 1))
    outs = []
    for env in (a, b, c, ref):
        s = env.reset(start_frame=torch.tensor([3, 40], dtype=torch.int32), noise=torch.zeros(B, 74, dtype=torch.float64))
        s = env.step(s, act)
        outs.append(s.pipeline_state.qvel.clone())
    assert torch.isfinite(outs[0]).all() and all(torch.equal(outs[0], o) for o in outs[1:])


def test_small_models_newton_takes_the_tree_sparse_hessian():
    """The ant and the humanoid run Newton on the tree-sparse Hessian: its factor and pivots in the debug image, no dense
    Jacobian."""
    for make in (_ant_env, _humanoid_env):
        env = make(1)
        env.debug(True)
        env.reset(start_frame=torch.zeros(1, dtype=torch.int32))
        nv, par, nM = int(env.sys.scalars["nv"]), env.sys.dof_parentid, 0
        for i in range(nv):  # qM's tree-sparse entries: one per ancestor of each dof, itself included
            j = i
            while j >= 0:
                nM, j = nM + 1, par[j]
        assert env.scratch("newton_LD").shape == (1, nM) and env.scratch("newton_LDiagInv").shape == (1, nv)
        with pytest.raises(Exception):
            env.scratch("newton_efc_J")  # no dense Jacobian


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _device_inputs(B, seed=0):
    rng = np.random.default_rng(seed)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((B, 74))).astype(np.float32)
    act = np.clip(0.3 * rng.standard_normal((B, 30)), -1, 1).astype(np.float32)
    return sf, noise, act


@pytest.mark.gpu
@pytest.mark.parametrize("B", [256, 4096])
@pytest.mark.parametrize("it,ls", CONFIGS)
def test_rodent_newton_on_gpu(it, ls, B):
    env = _rodent(B, newton_model(it, ls), device="cuda:0")
    assert int(env.dims.kernel_specialised) == 0
    sf, noise, act = _device_inputs(B)
    o64, o32 = H.make_oracle(env, "f64"), H.make_oracle(env, "f32")
    st, err, dev, rep, ost = P.control_step_follow(env, o64, o32, sf, noise, act)
    print(f"\n[rodent, Newton {it}/{ls}, control step, {B} envs] " +
          ", ".join(f"{k}: max {v.max():.2e} median {np.median(v):.2e}" for k, v in err.items()))
    nflip = P.check_control_step(err, dev, rep, max_flipped=B // 8)
    causes = P.flip_causes(rep)
    print(f"   flipped {nflip}: row presence {int(causes['row_presence'].sum())}, active set "
          f"{int(causes['active_set'].sum())}, other {int(causes['other'].sum())}")
    assert int(causes["other"].sum()) <= max(2, B // 50), causes
    print("   vs the natural oracle:", P.natural_check(st, o64, o32, act))
    assert np.abs(st.reward.cpu().numpy() - ost["reward"]).max() < 2e-4 or nflip > 0
    assert torch.isfinite(st.obs).all()


# (the rollout, graph and training tests run Newton 6 / 6: with ONE iteration the rodent's solve is far from converged, and
# under random actions both this kernel and the float64 oracle take the fallen envs to non-finite states within a few control
# steps -- DESIGN section 3, "Newton solver")
@pytest.mark.gpu
def test_rodent_newton_rollout_deterministic_on_gpu():
    B = 512
    sf, noise, _ = _device_inputs(B, seed=1)
    rng = np.random.default_rng(2)
    acts = [torch.from_numpy(np.clip(0.5 * rng.standard_normal((B, 30)), -1, 1).astype(np.float32)).cuda() for _ in range(20)]
    outs = []
    for _ in range(2):
        env = _rodent(B, newton_model(6, 6), device="cuda:0")
        s = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
        for a in acts:
            s = env.step(s, a)
        torch.cuda.synchronize()
        outs.append([s.pipeline_state.qpos.clone(), s.pipeline_state.qvel.clone(), s.obs.clone(), s.reward.clone()])
    for x, y in zip(*outs):
        assert torch.isfinite(x).all() and torch.equal(x, y)


@pytest.mark.gpu
def test_rodent_newton_graphed_unroll_equals_eager_on_gpu():
    from vnl_brax_imitation_amd.ppo_imitation import acting

    dev = torch.device("cuda:0")
    make_env = lambda B: _rodent(B, newton_model(6, 6), device=dev)  # noqa: E731
    B, T, extra = 130, 6, ("truncation", "traj")
    out = []
    for graphed in (False, True):
        env, policy = H.unroll_setup(B, False, 4, make_env, dev)
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        key = torch.Generator(device=dev).manual_seed(11)
        g = acting.GraphedUnroll(env, state, policy, key, T, extra_fields=extra) if graphed else None
        datas = []
        for _ in range(2):
            if graphed:
                state, data = g()
            else:
                state, data = acting.generate_unroll(env, state, policy, key, T, extra_fields=extra, fused=True)
            datas.append([x.clone() for x in acting._leaves(data)])
        out.append((state, datas))
    (s0, d0), (s1, d1) = out
    for a_, b_ in zip(d0, d1):
        for a, b in zip(a_, b_):
            assert a.shape == b.shape and torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n


@pytest.mark.gpu
def test_rodent_newton_short_training_on_gpu():
    from vnl_brax_imitation_amd.ppo_imitation import ppo_networks
    from vnl_brax_imitation_amd.ppo_imitation import train as ppo

    env = _rodent(64, newton_model(6, 6), device="cuda:0")
    nf = functools.partial(ppo_networks.make_intention_ppo_networks, intention_latent_size=60,
                           encoder_layer_sizes=(128, 128), decoder_layer_sizes=(128, 128))
    log = []
    _, (norm, flat), _ = ppo.train(
        environment=env, num_timesteps=2 * 64 * 5, episode_length=150, num_envs=64, learning_rate=1e-3,
        entropy_cost=1e-2, discounting=0.95, unroll_length=5, batch_size=16, num_minibatches=4,
        num_updates_per_batch=2, num_evals=1, normalize_observations=True, network_factory=nf, num_eval_envs=0,
        eval_env=None, seed=3, progress_fn=lambda s, m: log.append(m))
    m = log[-1]
    for k in ("training/total_loss", "training/v_loss", "training/policy_loss"):
        assert np.isfinite(m[k]), (k, m[k])
    assert torch.isfinite(flat).all()
