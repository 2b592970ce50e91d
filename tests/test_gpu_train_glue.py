"""The glue kernels of a training step on the device, each against a plain reference of its own (tests/train_glue_cases.py,
which the host simulation is put through as well):
  vnl_gather_rows   exact words of src[:, idx], guard words around every destination;
  vnl_adam_step     one step from a given state within derived rounding bounds, past the 2048-block cap into the grid-stride loop;
  vnl_ppo_head      every output element by element against float64 autograd: action widths beyond one 32-lane group, T around
                    the 8-step trip of the GAE loop, B beyond its 256 columns, more samples than one launch's groups;
  vnl_ppo_minibatch_grad_part   parts 1 and 2 (the data-parallel form of the step) against the whole step: the value segment
                    final after part 1 and left alone by part 2, the policy segment filled by part 2."""
import numpy as np
import pytest
import torch

import train_glue_cases as G
from ppo_update_cases import HP
from ppo_update_cases import make as _make
from vnl_brax_imitation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("N,M,permutation,all_ops", [(37, 11, False, False), (16, 16, True, False), (5, 16, False, False),
                                                     (37, 11, False, True)],
                         ids=["37-11", "16-16-permutation", "5-16-repeats", "37-11-all-24-ops"])
def test_gather_equals_index_select(N, M, permutation, all_ops):
    G.check_gather(_lib.load_library(), DEV, N, M, permutation, all_ops)


@pytest.mark.parametrize("n,count,hyper", G.ADAM_CASES, ids=[f"n{n}-t{c}-lr{h['lr']}" for n, c, h in G.ADAM_CASES])
def test_adam_within_the_rounding_bounds(n, count, hyper):
    G.check_adam(_lib.load_library(), DEV, n, count, hyper)


def test_adam_in_two_segments_equals_one_call():
    G.check_adam_segments(None, DEV)  # (FlatAdam finds the product library itself on a HIP device)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw-advantages"])
@pytest.mark.parametrize("shape", G.HEAD_SHAPES, ids=["x".join(map(str, s)) for s in G.HEAD_SHAPES])
def test_head_matches_float64_autograd(shape, normalize):
    G.check_head(_lib.load_library(), DEV, *shape, normalize)


def test_head_with_other_min_std_and_var_scale():
    G.check_head(_lib.load_library(), DEV, 9, 5, 33, 3, True, min_std=0.01, var_scale=0.5)


def test_head_all_truncated_leaves_the_entropy_term():
    G.check_head(_lib.load_library(), DEV, 9, 5, 33, 3, False, all_truncated=True)


# configurations that tests/test_gpu_ppo_update.py passes as whole steps; the last takes the transposed-input route, whose
# arena is split "value part | policy part"
SPLIT_CONFIGS = {
    "small-odd": dict(traj=45, obs=19, act=5, latent=6, enc=(40, 24), dec=(24, 40), val=(72, 56), T=5, B=9),
    "reference-sizes": dict(traj=795, obs=232, act=30, latent=64, enc=(256, 128), dec=(128, 256), val=(1024, 1024), T=20, B=128),
    "large-minibatch-wide-value": dict(traj=45, obs=19, act=5, latent=6, enc=(40, 24), dec=(24, 40), val=(512, 512), T=20, B=420),
}


def _tensors(nets):
    """(name, first, end) of every parameter tensor in the flat [policy | value] buffer, and the policy segment's size."""
    n_pol = nets.policy_network.layout.size
    out = []
    for seg, lay, off0 in (("policy", nets.policy_network.layout, 0), ("value", nets.value_network.layout, n_pol)):
        for name, (off, shape) in lay.entries.items():
            out.append((seg, name, off0 + off, off0 + off + int(np.prod(shape))))
    return out, n_pol


def _worst(a, b, tensors, seg):
    """The largest per-tensor difference of a from b, relative to the tensor's largest entry in b, over one segment."""
    worst = 0.0
    for s, name, lo, hi in tensors:
        if s == seg:
            worst = max(worst, np.abs(a[lo:hi] - b[lo:hi]).max() / max(np.abs(b[lo:hi]).max(), 1e-12))
    return worst


@pytest.mark.parametrize("name", list(SPLIT_CONFIGS))
def test_minibatch_grad_in_two_parts_keeps_its_promises(name):
    """include/vnl.h, vnl_ppo_minibatch_grad_part: after part 1 the value segment is final, part 2 fills the policy segment,
    and the caller's all-reduce may rewrite the value segment in between."""
    from vnl_brax_imitation_amd.ppo_imitation import hip_update, intention_losses, running_statistics

    cfg = dict(SPLIT_CONFIGS[name])
    T, B = cfg["T"], cfg["B"]
    nets, flat, data, norm, noise = _make(**cfg)
    tensors, n_pol = _tensors(nets)
    dev = torch.device(DEV)
    to = lambda t: t.to(dev)  # noqa: E731
    ndev = running_statistics.RunningStatisticsState(to(norm.count), to(norm.mean), to(norm.summed_variance), to(norm.std))
    fl, dd, nn = to(flat).contiguous(), data.map(to), {k: to(v) for k, v in noise.items()}
    upd = hip_update.HipPPOUpdate(nets, T, B, dev, **HP)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    # part 0: the whole step
    g0 = torch.full((flat.numel(),), float("nan"), device=dev)
    m0 = upd.grad(fl, ndev, dd, nn, g0)
    torch.cuda.synchronize()
    g0, m0 = f64(g0), f64(m0)
    assert np.isfinite(g0).all()
    # part 1: the value segment is final
    g = torch.full((flat.numel(),), float("nan"), device=dev)
    m1 = upd.grad(fl, ndev, dd, nn, g, part=1)
    torch.cuda.synchronize()
    g1, m1 = f64(g), f64(m1)
    e_value = _worst(g1, g0, tensors, "value")
    assert np.isfinite(g1[n_pol:]).all() and e_value <= 1e-5, e_value
    assert np.array_equal(np.isnan(m1), np.isnan(m0)), (m1, m0)
    ok = ~np.isnan(m0)
    e_metrics = (np.abs(m1 - m0)[ok] / np.maximum(1.0, np.abs(m0[ok]))).max()
    assert e_metrics <= 2e-6, (m1, m0)
    # the caller's all-reduce, as an in-place mean, rewrites the value segment
    g[n_pol:].mul_(0.5)
    written = g[n_pol:].clone()
    # part 2: the policy segment, and nothing else
    upd.grad(fl, ndev, dd, nn, g, part=2)
    torch.cuda.synchronize()
    assert torch.equal(g[n_pol:].view(torch.int32), written.view(torch.int32))
    g2 = f64(g)
    assert np.isfinite(g2[:n_pol]).all()
    e_policy = _worst(g2, g0, tensors, "policy")
    assert e_policy <= 1e-5, e_policy
    print(f"\n[grad parts, {name}] part 1 value segment vs whole step {e_value:.2e}, metrics {e_metrics:.2e}; part 2 policy "
          f"segment vs whole step {e_policy:.2e}")
    if name != "small-odd":
        return
    # the assembled gradient against float64 autograd through the op-by-op loss, the bound of
    # tests/test_gpu_ppo_update.py::test_hip_update_matches_autograd_and_numpy
    p64 = flat.double().requires_grad_(True)
    n64 = running_statistics.RunningStatisticsState(norm.count.double(), norm.mean.double(), norm.summed_variance.double(),
                                                    norm.std.double())
    loss, _ = intention_losses.compute_ppo_intention_loss(
        intention_losses.PPONetworkParams(policy=p64[:n_pol], value=p64[n_pol:]), n64, data.map(lambda x: x.double()), None,
        ppo_network=nets, noise={k: v.double() for k, v in noise.items()}, head="torch", time_major=True, **HP)
    loss.backward()
    g_ref = p64.grad.numpy()
    assembled = np.concatenate([g2[:n_pol], 2.0 * g2[n_pol:]])  # (the halving undone: exact)
    e_ref = max(_worst(assembled, g_ref, tensors, "policy"), _worst(assembled, g_ref, tensors, "value"))
    print(f"[grad parts, {name}] assembled gradient vs float64 autograd {e_ref:.2e}")
    assert e_ref < 2e-5 * max(1.0, np.sqrt(T * B / 2560.0)), e_ref
