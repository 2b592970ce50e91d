"""Cross-lane glue of the step kernel in fewer issue slots (csrc/vnl_body.h, vnl_rows_join / VNL_WAVE_SUMS / VNL_SCAN6: each
row_bcast step of a wave sum or scan one masked v_add_f32_dpp, several values through that stage together; dof_prefix: the last
trip of at most 16 dofs as two in-row scans): the product library against the regression build with the former forms
(csrc/build.py --xlaneplain).  The same adds on the same operands in the same order: every output bit for bit."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import test_gpu_sgpr_plain as G
import test_gpu_solver_staging as S
import test_humanoid as Hu
import test_solver_tail as T
from vnl_brax_imitation_amd.envs import wrappers as W
from vnl_brax_imitation_amd.ppo_imitation import acting, ppo_networks, running_statistics

pytestmark = pytest.mark.gpu
DEV = G.DEV
STEPS = G.STEPS
N = G.N  # 128 envs: the rodent's 73 dofs take both trips of every carried scan, the second one in the tail form
TRACE_ROWS = 8 + 64 * 8  # csrc/vnl_types.h VNL_TRACE_ROWS: then 16 ints, bit r set = constraint row r exists (D != 0)
FEW = 16  # the line search's short path: at most this many existing rows, one per lane of a DPP row


def _old():
    return G._variant("xlaneplain")


def _existing_rows(env):
    """(envs, solver calls of the last reset / step): number of existing constraint rows, from the debug trace's row bits."""
    bits = env.solver_trace()[..., TRACE_ROWS:TRACE_ROWS + 16].numpy().astype(np.uint32)
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=-1).sum(-1)


@functools.lru_cache(maxsize=None)
def _rows_of_the_rodent_inputs():
    """Existing rows per env and solver call over the rollout of G._rollout, from a debug run of the regression build."""
    env = G._rodent(N, _old())
    env.debug(True)
    sf, noise, acts = S._inputs(N)
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    rows = [_existing_rows(env)[:, :1]]
    for a in acts[:STEPS]:
        st = env.step(st, torch.from_numpy(a))
        rows.append(_existing_rows(env))
    return np.concatenate(rows, axis=1)


def test_the_inputs_take_both_line_search_paths():
    """The short path (at most 16 existing rows: the in-row butterfly alone) and the long one (more: the nine sums through
    vnl_rows_join) are both taken by the solver calls of the rollout the tests below compare."""
    rows = _rows_of_the_rodent_inputs()
    print(f"existing rows per env and solver call: min {rows.min()} max {rows.max()}; envs with a call of <= {FEW}: "
          f"{int((rows <= FEW).any(1).sum())}, of more: {int((rows > FEW).any(1).sum())}")
    assert ((rows <= FEW) & (rows > 0)).any(1).sum() >= 1 and (rows > FEW).any(1).sum() >= 1


@pytest.mark.parametrize("domain", [None, G._damping_armature], ids=["plain", "with_domain"])
def test_cross_lane_forms_change_no_bit_on_the_rodent(domain):
    """128 envs, the specialised kernels (CG 6 / 6) and their randomised instantiation (VnlSpecDom): both trips of every
    carried scan, the tail form as a compile-time fact."""
    new, old = G._rodent(N, None, domain), G._rodent(N, _old(), domain)
    assert int(new.dims.kernel_specialised) == 1 and int(old.dims.kernel_specialised) == 1
    G._same(G._rollout(new, N), G._rollout(old, N), "plain" if domain is None else "with_domain")


def test_generic_kernels_with_the_new_forms_equal_the_former_specialised_ones():
    """The shipped `nospec` library has the new forms (only -DVNL_XLANE_PLAIN switches them off): the generic kernels, where the
    tail form of dof_prefix is a wave-uniform branch at run time, against the former forms in the specialised kernel."""
    gen, old = G._rodent(N, G._variant("nospec")), G._rodent(N, _old())
    assert int(gen.dims.kernel_specialised) == 0 and int(old.dims.kernel_specialised) == 1
    G._same(G._rollout(gen, N), G._rollout(old, N), "nospec")


def test_cross_lane_forms_change_no_bit_on_the_humanoid():
    """64 envs, nv = 27: a single trip of every scan and no tail form -- the one-instruction row_bcast steps alone."""
    n = 64
    outs = []
    for lib in (None, _old()):
        with H.backend(lib):
            env = Hu._env(n, device=DEV)
        rng = np.random.default_rng(3)
        st = env.reset(5)
        snaps = [T._outputs(st)]
        for _ in range(STEPS):
            st = env.step(st, torch.from_numpy(np.clip(0.3 * rng.standard_normal((n, 21)), -1, 1).astype(np.float32)))
            snaps.append(T._outputs(st))
        outs.append(snaps)
    G._same(outs[0], outs[1], "humanoid")


def test_graphed_unroll_equals_the_eager_unroll_of_the_regression_build():
    """One 20-step replay of a captured unroll with the product library, 128 envs (the step kernel inside a graph, resets
    included), against the eager fused unroll of the regression build."""
    steps = 20
    out = []
    for lib, graphed in ((None, True), (_old(), False)):
        base = G._rodent(N, lib)
        with H.backend(lib):
            env = W.AutoResetWrapper(W.EpisodeWrapper(base, episode_length=8, action_repeat=1))
            nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                            preprocess_observations_fn=running_statistics.normalize,
                                                            intention_latent_size=16, encoder_layer_sizes=(32,),
                                                            decoder_layer_sizes=(32,))
            flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(DEV)
            policy = ppo_networks.make_inference_fn(nets)((running_statistics.init_state(base.observation_size, device=DEV), flat))
            torch.manual_seed(123)
            state = env.reset(torch.Generator().manual_seed(5))
            key = torch.Generator(device=DEV).manual_seed(11)
            if graphed:
                state, data = acting.GraphedUnroll(env, state, policy, key, steps, extra_fields=("truncation",))()
            else:
                state, data = acting.generate_unroll(env, state, policy, key, steps, extra_fields=("truncation",), fused=True)
        out.append((state, [x.clone() for x in acting._leaves(data)]))
    (s0, d0), (s1, d1) = out
    assert len(d0) == len(d1)
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n
    q = s0.pipeline_state.raw("qpos")
    assert torch.isfinite(q).all() and any(not torch.equal(x[0], x[-1]) for x in d0 if x.dim() > 1 and x.shape[0] == steps)
