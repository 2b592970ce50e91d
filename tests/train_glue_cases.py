"""The small kernels that hold a training step together -- vnl_gather_rows, vnl_adam_step, vnl_ppo_head (csrc/vnl_lib.hip) --
called through the C-ABI on raw tensors and compared with plain references: exact words for the gather, float64 arithmetic
on the same float32 state for Adam, float64 autograd through the op-by-op formulas of intention_losses.py for the head.
Shared by tests/test_gpu_train_glue.py (the device) and tests/test_train_glue.py (the host simulation): every `check_*`
takes the library and the device.

Output buffers of the gather and Adam cases are slices of larger buffers filled with a sentinel word, starting one element
in (so the base pointer is only 4-byte aligned); a write outside the slice, which no allocator would fault, shows in them."""
import ctypes as C
import functools

import torch

from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.ppo_imitation import intention_losses
from vnl_brax_imitation_amd.ppo_imitation.distribution import NormalTanhDistribution

SENTINEL = 0x5A5A5A5A
U = 2.0 ** -24  # unit roundoff of float32


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    cuda = torch.device(dev).type == "cuda"
    return C.c_void_p(torch.cuda.current_stream(torch.device(dev)).cuda_stream) if cuda else C.c_void_p(0)


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _guarded(words, dev, tail):
    """`words` (int32, CPU) on `dev` as the slice [1 : 1 + n] of a sentinel-filled buffer with `tail` guard words behind."""
    buf = torch.full((1 + words.numel() + tail,), SENTINEL, dtype=torch.int32, device=dev)
    out = buf[1:1 + words.numel()]
    out.copy_(words.reshape(-1))
    return buf, out


def _guards_intact(buf, n):
    b = buf.cpu()
    return int(b[0]) == SENTINEL and bool((b[1 + n:] == SENTINEL).all())


# ---- vnl_gather_rows ------------------------------------------------------------------------------------------------------
# (T, width) of the ops of one descriptor: widths below, at and above one pass of the 256 threads, the bootstrap row (an op
# with fewer time steps than its neighbours), and the op with the most time steps LAST (the grid's height comes from it)
GATHER_OPS = [(5, 1), (5, 3), (5, 255), (5, 256), (5, 257), (5, 795), (1, 232), (5, 9), (7, 30)]
GATHER_INT_OP = 7  # this op holds int32 words, NaN payloads and -0.0 among them
GATHER_SPECIAL = [0x7FC00001, 0xFFFFFFFF, 0x80000000]


def _i32(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


def gather_index(N, M, permutation, g):
    if permutation:
        assert N == M
        idx = torch.randperm(N, generator=g)
        while bool((idx[1:] > idx[:-1]).all()):
            idx = torch.randperm(N, generator=g)
        return idx.to(torch.int64)
    idx = torch.randint(0, N, (M,), generator=g)
    idx[0], idx[1], idx[2], idx[M - 1] = N - 1, 0, N - 1, min(3, N - 1)  # both ends, a duplicate, unsorted
    assert int(idx.min()) == 0 and int(idx.max()) == N - 1 and idx.unique().numel() < M
    assert not bool((idx[1:] >= idx[:-1]).all())
    return idx.to(torch.int64)


def check_gather(lib, dev, N, M, permutation=False, all_ops=False):
    g = torch.Generator().manual_seed(1000 * N + M)
    ops = list(GATHER_OPS)
    if all_ops:  # every slot of the descriptor in use
        ops = ops[:-1] + [(1 + k % 5, 2 + 3 * k) for k in range(_lib.POST_MAX_OPS - len(ops))] + ops[-1:]
        assert len(ops) == _lib.POST_MAX_OPS
    idx = gather_index(N, M, permutation, g)
    srcs, want = [], []
    for k, (T, w) in enumerate(ops):
        if k == GATHER_INT_OP:
            s = torch.randint(-(1 << 31), (1 << 31) - 1, (T, N, w), generator=g, dtype=torch.int64).to(torch.int32)
            s.view(-1)[:len(GATHER_SPECIAL)] = _i32(GATHER_SPECIAL)
            s[T - 1, N - 1, w - len(GATHER_SPECIAL):] = _i32(GATHER_SPECIAL)
            s[:, 0, 0] = _i32(GATHER_SPECIAL[:1])[0]
        else:
            s = torch.randn(T, N, w, generator=g).view(torch.int32)
        srcs.append(s)
        want.append(s[:, idx].contiguous())
    d_idx = idx.to(dev)
    d_src = [s.to(dev) for s in srcs]
    d_dst = [_guarded(torch.full((T * M * w,), SENTINEL, dtype=torch.int32), dev, tail=w + 1) for (T, w) in ops]
    d = _lib.GatherDesc()
    d.idx, d.N, d.M, d.num_ops = _ptr(d_idx), N, M, len(ops)
    for k, (T, w) in enumerate(ops):
        d.ops[k].dst, d.ops[k].src, d.ops[k].T, d.ops[k].width = _ptr(d_dst[k][1]), _ptr(d_src[k]), T, w
        assert d_dst[k][1].data_ptr() % 8 == 4
    _lib.check(lib, lib.vnl_gather_rows(C.byref(d), _stream(dev)))
    _sync(dev)
    assert torch.equal(d_idx.cpu(), idx)
    for k, (T, w) in enumerate(ops):
        assert torch.equal(d_dst[k][1].cpu().view(T, M, w), want[k]), (k, T, w)
        assert _guards_intact(d_dst[k][0], T * M * w), (k, T, w)
        assert torch.equal(d_src[k].cpu(), srcs[k]), (k, T, w)


# ---- vnl_adam_step --------------------------------------------------------------------------------------------------------
ADAM_DEFAULT = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8)  # optax.adam as the reference builds it
ADAM_OTHER = dict(lr=1e-2, b1=0.8, b2=0.99, eps=1e-5)
# n = 2048 * 256 + 1 is one element into the grid-stride loop behind the 2048-block cap; count 10^6: both corrections are 1
ADAM_CASES = [(1, 1, ADAM_DEFAULT), (1, 10 ** 6, ADAM_DEFAULT), (255, 2, ADAM_DEFAULT), (256, 1000, ADAM_DEFAULT),
              (257, 1, ADAM_DEFAULT), (257, 2, ADAM_OTHER), (257, 10 ** 6, ADAM_DEFAULT), (524289, 1, ADAM_DEFAULT),
              (524289, 2, ADAM_DEFAULT), (524289, 1000, ADAM_OTHER)]


def _f32(x):
    """A Python double rounded to float32, as a double."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32).double())


def _ulp(x):
    """Spacing of float32 at |x| (float64 tensor), normal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def adam_state(n, count, g):
    """(p0, grads, mu0, nu0) float32: |g| log-uniform over 1e-6 .. 10 with exact zeros, moments as a run of such gradients
    would leave them (zero before the first step), and some elements at rest (mu = nu = g = 0)."""
    sign = lambda: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1  # noqa: E731
    mag = lambda: 10.0 ** (torch.rand(n, generator=g) * 7 - 6)  # noqa: E731
    p0, gr = torch.randn(n, generator=g), sign() * mag()
    if count == 1:
        mu0, nu0 = torch.zeros(n), torch.zeros(n)
    else:
        mu0, nu0 = 0.5 * sign() * mag(), (0.3 * mag()) ** 2
    i = torch.arange(n)
    if n > 1:
        gr[i % 7 == 3] = 0.0
        rest = i % 13 == 5
        gr[rest], mu0[rest], nu0[rest] = 0.0, 0.0, 0.0
    assert (gr != 0).any() and float(gr.abs().max()) <= 10 and float(gr[gr != 0].abs().min()) >= 1e-6
    return p0, gr, mu0, nu0


def check_adam(lib, dev, n, count, hyper):
    g = torch.Generator().manual_seed(n + count)
    p0, gr, mu0, nu0 = adam_state(n, count, g)
    iv = lambda t: t.view(torch.int32)  # noqa: E731
    bufs = {k: _guarded(iv(v), dev, tail=3) for k, v in (("p", p0), ("mu", mu0), ("nu", nu0))}
    d_g, d_count = gr.to(dev), torch.tensor([count], dtype=torch.int64, device=dev)
    assert bufs["p"][1].data_ptr() % 8 == 4
    _lib.check(lib, lib.vnl_adam_step(_ptr(bufs["p"][1]), _ptr(d_g), _ptr(bufs["mu"][1]), _ptr(bufs["nu"][1]), _ptr(d_count),
                                      n, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], _stream(dev)))
    _sync(dev)
    for k, (buf, _) in bufs.items():
        assert _guards_intact(buf, n), k
    assert torch.equal(iv(d_g.cpu()), iv(gr)) and int(d_count.cpu()) == count
    p, mu, nu = (bufs[k][1].cpu().view(torch.float32) for k in ("p", "mu", "nu"))
    # float64 on the same float32 inputs, the constants formed as include/vnl.h says
    b1, b2, omb1, omb2 = _f32(hyper["b1"]), _f32(hyper["b2"]), _f32(1.0 - hyper["b1"]), _f32(1.0 - hyper["b2"])
    lr, eps = _f32(hyper["lr"]), _f32(hyper["eps"])
    bc1, bc2 = _f32(1.0 - hyper["b1"] ** count), _f32(1.0 - hyper["b2"] ** count)
    P0, G, M0, V0 = p0.double(), gr.double(), mu0.double(), nu0.double()
    m_ref, v_ref = b1 * M0 + omb1 * G, b2 * V0 + omb2 * G * G
    m_bound = 3 * U * ((b1 * M0).abs() + (omb1 * G).abs())  # three roundings
    v_bound = 4 * U * v_ref                                 # four roundings
    # the update from the kernel's OWN moments, so that the bounds do not compound
    upd = lr * ((mu.double() / bc1) / ((nu.double() / bc2).sqrt() + eps))
    p_ref = P0 - upd
    p_bound = 0.5 * _ulp(torch.maximum(P0.abs(), p_ref.abs())) + 16 * U * upd.abs()
    worst = {}
    for name, got, ref, bound in (("mu", mu, m_ref, m_bound), ("nu", nu, v_ref, v_bound), ("p", p, p_ref, p_bound)):
        err = (got.double() - ref).abs()
        assert torch.isfinite(got).all(), name
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                                 torch.zeros_like(err)))
        worst[name] = float(ratio.max())
    print(f"\n[adam n={n} count={count} lr={hyper['lr']}] worst error / bound: mu {worst['mu']:.3f} nu {worst['nu']:.3f} "
          f"p {worst['p']:.3f}")
    assert worst["mu"] <= 1.0 and worst["nu"] <= 1.0 and worst["p"] <= 1.0, worst
    rest = (gr == 0) & (mu0 == 0) & (nu0 == 0)
    assert n == 1 or rest.any()
    assert torch.equal(iv(p)[rest], iv(p0)[rest]) and not (mu[rest] != 0).any() and not (nu[rest] != 0).any()
    assert (gr != 0).any() and (torch.equal(p_ref.float(), p0) or not torch.equal(p, p0))


def check_adam_segments(lib, dev, n=1537, k=511):
    """FlatAdam.update on the whole buffer and as two segment calls [0:k], [k:n], k odd: the same bits, the count once."""
    from vnl_brax_imitation_amd.ppo_imitation import train as ppo

    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g)
    grads = [(0.1 * torch.randn(n, generator=g)).to(dev) for _ in range(2)]
    out = []
    for split in (False, True):
        opt = ppo.FlatAdam(3e-3, lib=lib)
        p = p0.clone().to(dev)
        st = opt.init(p)
        for gr in grads:
            if split:
                opt.update(gr, st, p, segment=slice(0, k), bump=True)
                opt.update(gr, st, p, segment=slice(k, n), bump=False)
            else:
                opt.update(gr, st, p)
        _sync(dev)
        out.append((p.cpu(), st["mu"].cpu(), st["nu"].cpu(), int(st["count"].cpu())))
    whole, parts = out
    assert whole[3] == parts[3] == len(grads)
    for a, b, name in zip(whole[:3], parts[:3], ("params", "mu", "nu")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert not torch.equal(whole[0], p0)


# ---- vnl_ppo_head ---------------------------------------------------------------------------------------------------------
HEAD_HP = dict(entropy_cost=1e-2, discounting=0.97, reward_scaling=2.0, gae_lambda=0.9, clipping_epsilon=0.3, kl_weight=3e-3)
# (T, B, act, latent): the lane group is 32 action components wide, the GAE loop takes 8 time steps a trip and 256 columns a
# pass, a launch covers 2048 samples and 65,536 latent entries, 256 blocks of partial sums
HEAD_SHAPES = [(1, 2, 1, 1), (9, 5, 33, 3), (8, 31, 32, 1), (7, 257, 5, 6), (16, 255, 30, 64), (3, 300, 70, 17),
               (20, 128, 30, 64)]
HEAD_SEED = 0  # for which the references alone meet every condition asserted in head_case, at every case below
HEAD_METRICS = ("total_loss", "policy_loss", "v_loss", "entropy_loss", "kl_loss_intention", "explained_variance",
                "advantage_mean", "advantage_std")
HEAD_TENSORS = ("g_logits", "g_baseline", "g_lat_mean", "g_lat_logvar", "vs", "advantages")
CLIP_EDGE = 1e-4   # a sample whose float64 rho is this close (relative) to 1 +- epsilon may take the other branch in float32
D32_MAX = 2e-5     # float32 torch may itself deviate this much from float64, per quantity, and no more
TOL_FLOOR, TOL_FACTOR = 2e-5, 8.0  # the bound: max(2e-5, 8 x d32): at most 1.6e-4


def head_inputs(T, B, act, latent, seed, min_std, var_scale, all_truncated):
    """float32 inputs that look like a rollout: the stored raw action is a sample of the current policy, the behaviour
    log-prob the current one plus noise, ~15 % truncated and ~10 % zero-discount steps; two planted edges take both branches
    of vnl_softplus at 20 (one sample's scale logits at 25, one raw action at -11)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    N = T * B
    dist = NormalTanhDistribution(act, min_std=min_std, var_scale=var_scale)
    logits = torch.cat([0.5 * r(N, act), 1.0 * r(N, act)], dim=1)
    logits[(N - 1) // 2, act:] = 25.0
    # (the planted action stays a plausible draw: its component's mean lies next to it, or |log_prob| runs into the thousands)
    logits[N - 1, act - 1], logits[N - 1, 2 * act - 1] = -10.5, 0.0
    logits = logits.float()
    raw = dist.sample_no_postprocessing(logits.double(), r(N, act))
    raw[N - 1, act - 1] = -11.0
    raw = raw.float()
    behaviour = (dist.log_prob(logits.double(), raw.double()) + 0.3 * r(N)).float()
    trunc = torch.ones(N) if all_truncated else (torch.rand(N, generator=g) < 0.15).float()
    inp = dict(logits=logits, baseline=r(N).float(), bootstrap=r(B).float(), lat_mean=r(N, latent).float(),
               lat_logvar=(0.5 * r(N, latent)).float(), raw_action=raw, behaviour_log_prob=behaviour,
               reward=(0.1 * r(N).abs()).float(), truncation=trunc,
               discount=(torch.rand(N, generator=g) >= 0.1).float(), eps_entropy=r(N, act).float())
    return inp


def head_formulas(inp, T, B, dtype, normalize, min_std, var_scale):
    """The op-by-op loss of intention_losses.py after the network forward passes, in `dtype` on the CPU: every output of
    vnl_ppo_head (gradients by autograd), and rho."""
    x = {k: v.to(dtype) for k, v in inp.items()}
    leaves = {k: x[k].clone().requires_grad_(True) for k in ("logits", "baseline", "lat_mean", "lat_logvar")}
    act = x["raw_action"].shape[1]
    dist = NormalTanhDistribution(act, min_std=min_std, var_scale=var_scale)
    hp = HEAD_HP
    tb = lambda v: v.view(T, B)  # noqa: E731
    rewards = tb(x["reward"]) * hp["reward_scaling"]
    trunc = tb(x["truncation"])
    termination = (1 - tb(x["discount"])) * (1 - trunc)
    baseline = tb(leaves["baseline"])
    vs, adv = intention_losses.compute_gae(truncation=trunc, termination=termination, rewards=rewards, values=baseline.detach(),
                                           bootstrap_value=x["bootstrap"], lambda_=hp["gae_lambda"], discount=hp["discounting"])
    adv_mean, adv_std = adv.mean(), adv.std(unbiased=False)
    a = (adv - adv_mean) / (adv_std + 1e-8) if normalize else adv
    target = dist.log_prob(leaves["logits"], x["raw_action"])
    rho = torch.exp(target - x["behaviour_log_prob"])
    s1 = tb(rho) * a
    s2 = tb(rho.clamp(1 - hp["clipping_epsilon"], 1 + hp["clipping_epsilon"])) * a
    policy_loss = -torch.mean(torch.minimum(s1, s2))
    v_err = vs - baseline
    v_loss = torch.mean(v_err * v_err) * 0.5 * 0.5
    entropy_loss = hp["entropy_cost"] * -torch.mean(dist.entropy(leaves["logits"], x["eps_entropy"]))
    kl = hp["kl_weight"] * intention_losses.kl_divergence(leaves["lat_mean"], leaves["lat_logvar"])
    total = policy_loss + v_loss + entropy_loss + kl
    total.backward()
    ev = 1.0 - v_loss / rewards.var(unbiased=False)
    out = {"g_" + k: leaves[k].grad.double() for k in leaves}
    out.update(vs=vs.reshape(-1).double(), advantages=adv.reshape(-1).double(), rho=rho.detach().double(),
               metrics=torch.stack([total, policy_loss, v_loss, entropy_loss, kl, ev, adv_mean, adv_std]).detach().double())
    return out


def _tensor_dev(got, ref, keep=None):
    """max |got - ref| relative to the reference tensor's largest entry (rows outside `keep` left out of both); a reference
    that is zero throughout admits only zeros."""
    if keep is not None:
        got, ref = got[keep], ref[keep]
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def _metric_scales(m):
    """Each loss term relative to max(|term|, |total|) (as tests/test_gpu_ppo_update.py); explained variance = 1 - a ratio,
    relative to max(|.|, 1); the advantages' mean and std relative to max(|mean|, std), the size of what was summed."""
    total, s_adv = abs(float(m[0])), max(abs(float(m[6])), float(m[7]))
    return [max(abs(float(m[i])), total) for i in range(5)] + [max(abs(float(m[5])), 1.0), s_adv, s_adv]


def _metric_dev(got, ref):
    out = []
    for i, s in enumerate(_metric_scales(ref)):
        err = abs(float(got[i]) - float(ref[i]))
        out.append(err / s if s > 0 else (0.0 if err == 0 else float("inf")))
    return out


@functools.lru_cache(maxsize=None)
def head_case(T, B, act, latent, normalize, min_std=0.001, var_scale=1.0, all_truncated=False):
    """Inputs, the float64 reference and the bound per quantity, computed once and shared by both tiers.  Everything asserted
    here is a property of the references alone."""
    inp = head_inputs(T, B, act, latent, HEAD_SEED, min_std, var_scale, all_truncated)
    ref = head_formulas(inp, T, B, torch.float64, normalize, min_std, var_scale)
    f32 = head_formulas(inp, T, B, torch.float32, normalize, min_std, var_scale)
    N, eps = T * B, HEAD_HP["clipping_epsilon"]
    rho = ref["rho"]
    edge = ((rho / (1 - eps) - 1).abs() <= CLIP_EDGE) | ((rho / (1 + eps) - 1).abs() <= CLIP_EDGE)
    assert int(edge.sum()) <= 0.01 * N, (int(edge.sum()), N)
    keep = {"g_logits": ~edge}
    d32 = {k: _tensor_dev(f32[k], ref[k], keep.get(k)) for k in HEAD_TENSORS}
    d32.update(zip(HEAD_METRICS, _metric_dev(f32["metrics"], ref["metrics"])))
    for k, v in d32.items():
        assert v <= D32_MAX, (k, v)
    tol = {k: max(TOL_FLOOR, TOL_FACTOR * v) for k, v in d32.items()}
    if N >= 50 and not all_truncated:
        clipped = float(((rho < 1 - eps) | (rho > 1 + eps)).float().mean())
        assert 0.2 <= clipped <= 0.6, clipped
        trunc = inp["truncation"].view(T, B)
        term = (1 - inp["discount"].view(T, B)) * (1 - trunc)
        for name, flag in (("truncated", trunc), ("terminated", term)):
            assert 0 < int(flag.sum()) < N and bool(flag[-1].any()), name
    if all_truncated:  # nothing but the entropy term reaches the logits
        assert not ref["advantages"].any() and float(ref["metrics"][1]) == 0 and ref["g_logits"].any()
    return inp, ref, keep, tol, d32


def check_head(lib, dev, T, B, act, latent, normalize, min_std=0.001, var_scale=1.0, all_truncated=False):
    inp, ref, keep, tol, d32 = head_case(T, B, act, latent, normalize, min_std, var_scale, all_truncated)
    N = T * B
    d_in = {k: v.to(dev) for k, v in inp.items()}
    sizes = dict(g_logits=2 * N * act, g_baseline=N, g_lat_mean=N * latent, g_lat_logvar=N * latent, vs=N, advantages=N,
                 metrics=8)
    guard = 64  # sentinel words behind every output
    d_out = {k: torch.full((n + guard,), SENTINEL, dtype=torch.int32, device=dev) for k, n in sizes.items()}
    work = torch.zeros(_lib.PPO_HEAD_WORKSPACE_FLOATS, dtype=torch.float32, device=dev)
    a = _lib.PPOHeadArgs()
    a.T, a.B, a.act, a.latent = T, B, act, latent
    for k, v in d_in.items():
        setattr(a, k, _ptr(v))
    for k, v in HEAD_HP.items():
        setattr(a, k, v)
    a.min_std, a.var_scale, a.normalize_advantage = min_std, var_scale, int(normalize)
    for k, v in d_out.items():
        setattr(a, k, _ptr(v))
    _lib.check(lib, lib.vnl_ppo_head(C.byref(a), _ptr(work), _stream(dev)))
    _sync(dev)
    for k, v in d_in.items():
        assert torch.equal(v.cpu().view(torch.int32), inp[k].view(torch.int32)), k
    got = {}
    for k, n in sizes.items():
        w = d_out[k].cpu()
        assert bool((w[n:] == SENTINEL).all()), k
        got[k] = w[:n].view(torch.float32).double()
        assert torch.isfinite(got[k]).all(), k
    got["g_logits"] = got["g_logits"].view(N, 2 * act)
    got["g_lat_mean"], got["g_lat_logvar"] = got["g_lat_mean"].view(N, latent), got["g_lat_logvar"].view(N, latent)
    dev_k = {k: _tensor_dev(got[k], ref[k], keep.get(k)) for k in HEAD_TENSORS}
    dev_k.update(zip(HEAD_METRICS, _metric_dev(got["metrics"], ref["metrics"])))
    worst = max(dev_k, key=lambda k: dev_k[k] / tol[k])
    print(f"\n[head T={T} B={B} act={act} latent={latent} norm={int(normalize)} min_std={min_std} var_scale={var_scale}"
          f"{' all truncated' if all_truncated else ''}] worst error / bound {dev_k[worst] / tol[worst]:.3f} ({worst}: "
          f"{dev_k[worst]:.2e}, bound {tol[worst]:.2e}, float32 torch {d32[worst]:.2e}); left out at the clip edge: "
          f"{int((~keep['g_logits']).sum())} of {N}")
    for k in dev_k:
        assert dev_k[k] <= tol[k], (k, dev_k[k], tol[k], d32[k])
    if all_truncated:
        assert float(got["metrics"][1]) == 0 and not got["advantages"].any()
