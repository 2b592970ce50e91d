"""The tiled prediction_corr kernels (csrc/vnl_ppo.hip: row means, partial Gram matrices over chunks of B, a finish that
adds them in a fixed order) against float64 np.corrcoef of the same float32 inputs.

Bound 2e-6: a float32 two-pass NumPy emulation with chunked Gram accumulation stays below 6e-8 on every shape used here;
2e-6 is 30 x that, for the kernels' other summation order.  (A one-pass raw-moment form errs by 4e-6 .. 1.4e-4 on these
inputs: the `vs` rows have mean / std = 50.)"""
import numpy as np
import pytest
import torch

import prediction_corr_cases as PC

pytestmark = pytest.mark.gpu

BOUND = 2e-6
DEV = "cuda:0"


def _run(T, B, scaling, route):
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    vs, reward = PC.rows(T, B)
    out = hip_update.prediction_corr(torch.tensor(vs, device=DEV), torch.tensor(reward, device=DEV), scaling, route=route)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0], PC.reference(vs, reward, scaling)


def _chunk_cols(T, B):
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    return int(hip_update.prediction_corr_plan(T, B, 2).chunk_cols)


@pytest.mark.parametrize("T,B", [(1, 2), (1, 3), (5, 9), (3, 65), (7, 257), (33, 300), (20, 420), (20, 1024)])
@pytest.mark.parametrize("scaling", [1.0, 2.5])
def test_tiled_route_matches_float64_corrcoef(T, B, scaling):
    got, ref = _run(T, B, scaling, 2)
    print(f"\n[prediction_corr tiled T={T} B={B} scaling={scaling}] got {got:.9f} ref {ref:.9f} err {abs(got - ref):.2e}")
    assert np.isfinite(got) and abs(got - ref) <= BOUND, (got, ref)


@pytest.mark.parametrize("which", ["chunk_cols-1", "chunk_cols", "chunk_cols+1", "2*chunk_cols+1"])
def test_tiled_route_at_the_chunk_boundaries(which):
    T = 20
    cc = _chunk_cols(T, 64)  # (the plan's smallest chunk: every B up to 32 of them has this width)
    B = {"chunk_cols-1": cc - 1, "chunk_cols": cc, "chunk_cols+1": cc + 1, "2*chunk_cols+1": 2 * cc + 1}[which]
    assert _chunk_cols(T, B) == cc
    for scaling in (1.0, 2.5):
        got, ref = _run(T, B, scaling, 2)
        print(f"\n[prediction_corr tiled T={T} B={B} ({which}, chunk_cols {cc}) scaling={scaling}] err {abs(got - ref):.2e}")
        assert np.isfinite(got) and abs(got - ref) <= BOUND, (B, got, ref)


@pytest.mark.parametrize("T,B,chunks,chunk_cols", [(20, 2049, 22, 96), (20, 2 * 1024 + 33, 22, 96), (200, 900, 15, 64)])
def test_tiled_route_with_several_slabs_per_chunk(T, B, chunks, chunk_cols):
    """Beyond 32 x 32 columns a workgroup loops over the 32-column slabs of its chunk (LDS reused behind a barrier, sums
    carried across slabs), the last slab ragged; with R = 400 the plan allows fewer than 32 chunks (32 R x R matrices would
    exceed its 16 MB) and there are 28 pairs of row tiles.  Same bound: the float32 two-pass emulation with this chunking
    stays below 4e-8 on these shapes too."""
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    plan = hip_update.prediction_corr_plan(T, B, 0)
    assert (plan.route, plan.chunks, plan.chunk_cols) == (2, chunks, chunk_cols)
    assert chunk_cols > 32 and B % 32 != 0
    got, ref = _run(T, B, 2.5, 2)
    print(f"\n[prediction_corr tiled T={T} B={B}, {chunks} chunks of {chunk_cols}] got {got:.9f} ref {ref:.9f} err {abs(got - ref):.2e}")
    assert np.isfinite(got) and abs(got - ref) <= BOUND, (got, ref)


@pytest.mark.parametrize("T,B", [(20, 128), (5, 9)])
def test_both_routes_agree(T, B):
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    assert hip_update.prediction_corr_plan(T, B, 0).route == 1
    for scaling in (1.0, 2.5):
        one, ref = _run(T, B, scaling, 1)
        tiled, _ = _run(T, B, scaling, 2)
        auto, _ = _run(T, B, scaling, 0)
        print(f"\n[prediction_corr T={T} B={B} scaling={scaling}] one workgroup err {abs(one - ref):.2e}, tiled err "
              f"{abs(tiled - ref):.2e}, difference {abs(one - tiled):.2e}")
        assert abs(one - ref) <= BOUND and abs(tiled - ref) <= BOUND, (one, tiled, ref)
        assert abs(float(one) - float(tiled)) <= 1e-6
        assert auto.tobytes() == one.tobytes()  # route 0 is the one-workgroup kernel where the rows fit


def test_tiled_route_is_deterministic():
    a, _ = _run(20, 1024, 1.0, 2)
    b, _ = _run(20, 1024, 1.0, 2)
    assert a.tobytes() == b.tobytes()


def test_constant_row_gives_nan_on_both_routes():
    """A row without variance: jnp.corrcoef gives NaN there, and so does the mean (the existing kernel passes it through)."""
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    vs, reward = (torch.tensor(a, device=DEV) for a in PC.rows(5, 9))
    vs[2] = 5.0
    for route in (1, 2):
        out = hip_update.prediction_corr(vs, reward, 1.0, route=route)
        assert torch.isnan(out).all(), route


def test_through_the_update_handle():
    """T = 20, B = 1024 (the reference's minibatch proportions) on the small-odd network: metrics[8] is a number, agrees with
    the float64 autograd path, and is what vnl_prediction_corr gives on the handle's own `vs`."""
    from vnl_brax_imitation_amd.ppo_imitation import hip_update, running_statistics

    T, B = 20, 1024
    nets, flat, data, norm, noise = PC.make_update_case(T, B)
    m_ref, _ = PC.loss_float64(nets, flat, data, norm, noise)
    dev = torch.device(DEV)
    upd = hip_update.HipPPOUpdate(nets, T, B, dev, **PC.HP)
    to = lambda t: t.to(dev)  # noqa: E731
    grads = torch.empty(flat.numel(), device=dev)
    ndev = running_statistics.RunningStatisticsState(to(norm.count), to(norm.mean), to(norm.summed_variance), to(norm.std))
    mt = upd.grad(to(flat).contiguous(), ndev, data.map(to), {k: to(v) for k, v in noise.items()}, grads)
    torch.cuda.synchronize()
    got = mt.cpu().numpy()[8]
    ref = float(m_ref["prediction_corr"])
    print(f"\n[prediction_corr through the handle, T={T} B={B}] got {got:.9f} float64 autograd path {ref:.9f}")
    assert np.isfinite(got)
    assert abs(got - ref) < 2e-5, (got, ref)
    assert hip_update.prediction_corr_plan(T, B, 0).route == 2
    alone = hip_update.prediction_corr(upd.buffer("vs").view(T, B), to(data.reward), PC.HP["reward_scaling"], route=0)
    torch.cuda.synchronize()
    assert alone.cpu().numpy()[0].tobytes() == got.tobytes()


def test_tiled_route_in_a_captured_graph():
    from vnl_brax_imitation_amd.ppo_imitation import hip_update

    T, B = 20, 1024
    vs, reward = (torch.tensor(a, device=DEV) for a in PC.rows(T, B))
    eager = hip_update.prediction_corr(vs, reward, 2.5, route=2)
    torch.cuda.synchronize()
    eager = eager.cpu().numpy().tobytes()
    plan = hip_update.prediction_corr_plan(T, B, 2)
    ws = torch.zeros(int(plan.workspace_floats), dtype=torch.float32, device=DEV)
    out = torch.zeros(1, dtype=torch.float32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        hip_update.prediction_corr(vs, reward, 2.5, route=2, out=out, workspace=ws)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == eager
