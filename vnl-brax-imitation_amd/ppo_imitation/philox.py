"""Counter-based noise of the acting policy: Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as
1, 2, 3") restated in torch integer ops.  It is the reference of the device draws of csrc/vnl_policy.hip
(vnl_policy_forward_noise) and what the torch-backend policy draws from with `noise="device"`.

    key     = (seed low 32 bits, seed high 32 bits)
    counter = (block, env, step low 32 bits, (step >> 32) << 2 | stream),  step < 2^62
    stream  = 0 latent draw, 1 action draw, 2 the random action shared by the batch (env = 0xFFFFFFFF),
              3 the fresh episode reset of an env (vnl_env_reset_done): blocks 0.. its reset noise, block 0x80000000 its
              start frame and clip, blocks 0x40000000.. the redraw of its physical domain (domain_draws)

A call yields four words x0..x3; u_i = ((x_i >> 8) + 0.5) 2^-24 lies strictly inside (0, 1).  Normal draws are Box-Muller
pairs, (u0, u1) -> sqrt(-2 ln u0) (cos, sin)(2 pi u1) and (u2, u3) likewise; element j of an env's row is output j % 4 of block
j / 4, the surplus of the last block is dropped.  Stream 2 gives 2 u - 1 per element.  An env's draws depend on
(seed, step, global env index) alone: not on the batch size, not on where the env sits in the batch.

Words are int64 tensors masked to 32 bits; the floating-point part runs in float64 and is cast to float32 last."""
from __future__ import annotations

import math
from typing import Tuple, Union

import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_LATENT, STREAM_ACTION, STREAM_SHARED = 0, 1, 2
STREAM_RESET = 3  # the last one: the stream field is the low two bits of counter word 3
RESET_INT_BLOCK = 0x80000000  # the block of stream 3 whose words x0, x1 give start frame and clip
DOMAIN_BLOCK, DOMAIN_INITIAL, DOMAIN_FIELD_STRIDE = 0x40000000, 0x20000000, 0x00100000  # stream 3: the domain redraw
DOMAIN_FIELDS = ("cg_friction", "act_gain", "dof_damping", "dof_armature")  # field index f, the order of vnl_domain
BODY_DOMAIN_FIELDS = ("body_mass", "body_inertia", "body_ipos")  # field indices 4, 5, 6: the order of vnl_body_domain
SHARED_ENV = 0xFFFFFFFF  # the env word of stream 2: no env may have this index

IntLike = Union[int, torch.Tensor]


def _mulhilo(m: int, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(high, low) 32 bits of the 64-bit product m * x, without leaving the signed 64-bit range: x in 16-bit halves."""
    p0, p1 = m * (x & 0xFFFF), m * (x >> 16)  # both < 2^48
    lo = (((p1 & 0xFFFF) << 16) + p0) & MASK
    hi = (p1 + (p0 >> 16)) >> 16
    return hi, lo


def philox4x32(counter: torch.Tensor, key: Tuple[IntLike, IntLike], rounds: int = 10) -> torch.Tensor:
    """counter: int64 [..., 4] of 32-bit words; key: two 32-bit words (ints or int64 tensors).  Returns int64 [..., 4]."""
    c0, c1, c2, c3 = (counter[..., i] & MASK for i in range(4))
    k0, k1 = key
    for r in range(rounds):
        hi0, lo0 = _mulhilo(M0, c0)
        hi1, lo1 = _mulhilo(M1, c2)
        c0, c1, c2, c3 = (hi1 ^ c1 ^ k0) & MASK, lo1, (hi0 ^ c3 ^ k1) & MASK, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return torch.stack((c0, c1, c2, c3), dim=-1)


def _words(seed: int, step: IntLike, env: torch.Tensor, n: int, stream: int, block0: int = 0) -> torch.Tensor:
    """The (n + 3) // 4 blocks of every env's row, from block `block0` on: int64 [len(env), blocks, 4].  `step` may be an
    int64 tensor on the device (the policy's counter): nothing is read back to the host."""
    dev = env.device
    nb = (n + 3) // 4
    step = torch.as_tensor(step, dtype=torch.int64, device=dev).reshape(())
    shape = (env.shape[0], nb)
    ctr = torch.stack(((block0 + torch.arange(nb, dtype=torch.int64, device=dev)).expand(shape),
                       (env.to(torch.int64) & MASK)[:, None].expand(shape),
                       (step & MASK).expand(shape),
                       (((step >> 32) << 2) | stream).expand(shape)), dim=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32(ctr, (seed & MASK, seed >> 32))


def _unit(x: torch.Tensor) -> torch.Tensor:
    return ((x >> 8).to(torch.float64) + 0.5) * 2.0 ** -24


def normal(seed: int, step: IntLike, env: torch.Tensor, n: int, stream: int) -> torch.Tensor:
    """float32 [len(env), n] standard normal draws of the envs with GLOBAL indices `env` (int64 [B]) at `step`."""
    u = _unit(_words(seed, step, env, n, stream))
    r = torch.sqrt(-2.0 * torch.log(u[..., 0::2]))  # [B, blocks, 2]: from u0, u2
    a = (2.0 * math.pi) * u[..., 1::2]              # from u1, u3
    out = torch.stack((r * torch.cos(a), r * torch.sin(a)), dim=-1)  # [B, blocks, pair, (cos, sin)]
    return out.reshape(env.shape[0], -1)[:, :n].to(torch.float32)


def shared_uniform(seed: int, step: IntLike, n: int, device=None) -> torch.Tensor:
    """float32 [n] in (-1, 1): the ONE pre-tanh random action shared by the batch (reference ppo_networks.py:67-73)."""
    env = torch.full((1,), SHARED_ENV, dtype=torch.int64, device=device)
    u = _unit(_words(seed, step, env, n, STREAM_SHARED))
    return (2.0 * u - 1.0).reshape(-1)[:n].to(torch.float32)


def reset_draws(seed: int, step: IntLike, env: torch.Tensor, nq: int, start_hi: int, num_clips: int,
                noise_scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(start_frame int64 [B], clip_id int64 [B], noise float32 [B, nq]) of a fresh reset (vnl_env_reset_done) of the envs
    with GLOBAL indices `env` at `step`.  The integers are multiply-shift maps of words x0, x1 of block RESET_INT_BLOCK,
    (x * n) >> 32, exact in int64 for n < 2^31 (x < 2^32)."""
    x = _words(seed, step, env, 1, STREAM_RESET, block0=RESET_INT_BLOCK)[:, 0]  # [B, 4]
    assert 0 < int(start_hi) < (1 << 31) and 0 < int(num_clips) < (1 << 31)

    def below(w: torch.Tensor, n: int) -> torch.Tensor:
        return (w * n) >> 32

    u = _unit(_words(seed, step, env, nq, STREAM_RESET))
    r = torch.sqrt(-2.0 * torch.log(u[..., 0::2]))
    a = (2.0 * math.pi) * u[..., 1::2]
    nz = torch.stack((r * torch.cos(a), r * torch.sin(a)), dim=-1).reshape(env.shape[0], -1)[:, :nq]
    return below(x[:, 0], int(start_hi)), below(x[:, 1], int(num_clips)), (nz * float(noise_scale)).to(torch.float32)


def domain_draws(seed: int, step: IntLike, env: torch.Tensor, field: IntLike, lo, hi, shared: bool = False,
                 initial: bool = False) -> torch.Tensor:
    """float64 [len(env), n]: the values a domain redraw (vnl_env_reset_done with ranges, vnl_env_redraw_domain) draws for
    field `field` (index or name of DOMAIN_FIELDS) of the envs with GLOBAL indices `env` at `step`, between the bounds `lo`,
    `hi` (float64 [n]).  Element j takes word j % 4 of block DOMAIN_BLOCK + initial * DOMAIN_INITIAL + f * DOMAIN_FIELD_STRIDE
    + j / 4; a `shared` field word 0 of the first block for every element.  u = (x + 0.5) 2^-32 is exact in float64;
    v = lo + u * (hi - lo) rounds the difference, the product and the sum separately (torch ops do not fuse them): the bits
    of the device.  The tables are v cast to the env's real type, the inverse weight `contact_invweight` of v."""
    f = DOMAIN_FIELDS.index(field) if isinstance(field, str) else int(field)
    lo = torch.as_tensor(lo, dtype=torch.float64).reshape(-1)
    hi = torch.as_tensor(hi, dtype=torch.float64).reshape(-1)
    n = lo.shape[0]
    assert hi.shape[0] == n and 0 <= f < 4 and n <= 4 * DOMAIN_FIELD_STRIDE
    block0 = DOMAIN_BLOCK + (DOMAIN_INITIAL if initial else 0) + f * DOMAIN_FIELD_STRIDE
    x = _words(seed, step, env, 1 if shared else n, STREAM_RESET, block0=block0).reshape(env.shape[0], -1)
    x = x[:, :1].expand(env.shape[0], n) if shared else x[:, :n]
    u = (x.to(torch.float64) + 0.5) * 2.0 ** -32
    w = hi - lo
    p = u.cpu() * w
    return lo + p


def body_domain_draws(seed: int, step: IntLike, env: torch.Tensor, ranges, shared=(), inertia_with_mass: bool = False,
                      initial: bool = False) -> dict:
    """{field: float64 (len(env), nbody[, 3])}: the values a body-domain redraw (vnl_env_reset_done with body ranges,
    vnl_env_redraw_domain; include/vnl.h: vnl_body_domain_ranges) draws for the fields of `ranges` ({field: (lo, hi)} float64
    (nbody,) / (nbody, 3): what RodentTracking.body_domain_ranges returns, further keys ignored) of the envs with GLOBAL indices
    `env` at `step`.  Field indices 4, 5, 6 of the block range of `domain_draws`, the field flattened: element j takes word
    j % 4 of block j / 4, a field in `shared` word 0 of block 0; with `inertia_with_mass` moment (b, k) takes the word of body
    b's mass.  Row 0 (the world body) is never drawn: it holds lo[0], which with_body_domain_ranges sets to the compiled
    values.  The arithmetic is domain_draws': the bits of the device."""
    env = torch.as_tensor(env)
    B, out, u_mass = env.shape[0], {}, None
    if inertia_with_mass and "body_mass" not in ranges:
        raise ValueError("inertia_with_mass needs a range for 'body_mass'")
    for k in BODY_DOMAIN_FIELDS:
        if k not in ranges:
            continue
        f = 4 + BODY_DOMAIN_FIELDS.index(k)
        lo, hi = (torch.as_tensor(x, dtype=torch.float64).cpu() for x in ranges[k])
        shape, n = tuple(lo.shape), lo.numel()
        assert tuple(hi.shape) == shape and n <= 4 * DOMAIN_FIELD_STRIDE
        lo, hi = lo.reshape(-1), hi.reshape(-1)
        if k == "body_inertia" and inertia_with_mass:
            u = u_mass.repeat_interleave(3, dim=1)
        else:
            block0 = DOMAIN_BLOCK + (DOMAIN_INITIAL if initial else 0) + f * DOMAIN_FIELD_STRIDE
            one = k in shared
            x = _words(seed, step, env, 1 if one else n, STREAM_RESET, block0=block0).reshape(B, -1)
            x = x[:, :1].expand(B, n) if one else x[:, :n]
            u = ((x.to(torch.float64) + 0.5) * 2.0 ** -32).cpu()
        if k == "body_mass":
            u_mass = u
        w = hi - lo
        p = u * w
        v = (lo + p).reshape((B,) + shape).clone()
        v[:, 0] = lo.reshape(shape)[0]
        out[k] = v
    return out


def contact_invweight(t, mu, impratio: float):
    """The contact rows' inverse weight from friction `mu`, float64, as the library derives it (csrc/vnl_types.h)."""
    return (t + mu * mu * t) * 2 * mu * mu / impratio


def words_u32(t) -> torch.Tensor:
    """The 32-bit words of an int32 tensor (or of an integer array of values below 2^32) as unsigned values: int64, CPU."""
    return torch.as_tensor(t).detach().cpu().to(torch.int64) & MASK


def weighted_cells(seed: int, step: IntLike, env: torch.Tensor, cdf: torch.Tensor) -> torch.Tensor:
    """The cells (int64 [B], cell = clip * start_hi + start_frame) that a prioritised fresh reset
    (vnl_env_reset_done_weighted) draws for the envs with GLOBAL indices `env` at `step` from the table `cdf` (int32 words
    or unsigned values, [ncell]): #{ c < ncell - 1 : cdf[c] <= x0 } on word x0 of block RESET_INT_BLOCK, the word of
    reset_draws' start frame.  The last entry is not read."""
    x0 = _words(seed, step, env, 1, STREAM_RESET, block0=RESET_INT_BLOCK)[:, 0, 0].cpu().contiguous()
    return torch.searchsorted(words_u32(cdf)[:-1].contiguous(), x0, right=True)


def start_priority_table(ended, failed, prior: int = 1, floor_q16: int = 6554,
                         decay_shift: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """vnl_start_priority_update restated (include/vnl.h): (cdf, ended', failed') as unsigned values, int64 [ncell], from
    counters given as int32 words or unsigned values.  uint64 throughout: (f + a) << 16 < 2^49, P_c << 32 < 2^64 because
    P_c <= S < 2^32 for ncell <= 32768."""
    import numpy as np

    n0, f0 = words_u32(ended).numpy().astype(np.uint64), words_u32(failed).numpy().astype(np.uint64)
    ncell, a = n0.shape[0], int(prior)
    assert 1 <= ncell <= 32768 and 1 <= a < (1 << 32) and 1 <= int(floor_q16) <= 65536 and 0 <= int(decay_shift) <= 31
    n = np.minimum(n0, np.uint64(1 << 20))
    f = np.minimum(f0, n)
    s = ((f + np.uint64(a)) << np.uint64(16)) // (n + np.uint64(2 * a))
    assert int(s.max()) <= 65535
    p = np.cumsum(s + np.uint64(floor_q16), dtype=np.uint64)
    assert int(p[-1]) < (1 << 32)
    cdf = (p << np.uint64(32)) // p[-1]
    cdf[-1] = 0xFFFFFFFF
    back = lambda x: torch.from_numpy(x.astype(np.int64))  # noqa: E731
    return back(cdf), back(n0 >> np.uint64(decay_shift)), back(f0 >> np.uint64(decay_shift))
