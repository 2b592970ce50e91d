"""'A regression build of csrc/build.py VARIANTS gives the product's bits' on the device: the libraries, the envs bound to
them, the inputs, the rollouts and the comparisons that the tests/test_gpu_*.py of the regression builds share.  A test of
a new build names its variant, its sizes and what is specific to it; everything else is here."""
import functools

import numpy as np
import torch

import domain_cases as D
import helpers as H
import model_cases as M
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.ppo_imitation import acting

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def variant(name):
    """The library of a build of csrc/build.py VARIANTS; None: the product (what an env binds to by default)."""
    if name is None:
        return None
    from vnl_brax_imitation_amd.csrc import build as hip_build

    return _lib.load_library(hip_build.build(variant=name))


def rodent(n, lib, domain=None, **kw):
    """RodentTracking bound to `lib`; domain(sys, n) -> the fields of a with_domain, bound to the same library."""
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    with H.backend(lib):
        base = RodentTracking(H.reference_clip(), num_envs=n, device=DEV, **{**H.env_kwargs(), **kw})
        return base if domain is None else base.with_domain(domain(base.sys, n))


def friction(sys, n):
    return {"cg_friction": D.random_domain(sys, n, 21)["cg_friction"]}


def damping_armature(sys, n):
    dom = D.random_domain(sys, n, 22)
    return {"dof_damping": dom["dof_damping"], "dof_armature": dom["dof_armature"]}  # (damping feeds D2, armature both pivots)


@functools.lru_cache(maxsize=None)
def rodent_inputs(n):
    """Start frames, reset noise and three action sets: several envs with contacts, both line-search routes
    (tests/test_gpu_solver_staging.py, tests/test_gpu_xlane_plain.py)."""
    rng = np.random.default_rng(9)
    sf = rng.integers(0, 235, n).astype(np.int32)
    noise = (1e-3 * rng.standard_normal((n, 74))).astype(np.float32)
    acts = np.clip(0.3 * rng.standard_normal((3, n, 30)), -1, 1).astype(np.float32)
    return sf, noise, acts


def outputs(st):
    """Every tensor of a state, cloned."""
    out = {"obs": st.obs, "reward": st.reward, "done": st.done}
    out.update({"ps." + n: st.pipeline_state.raw(n) for n in st.pipeline_state._FIELDS})
    out.update({"info." + k: v for k, v in st.info.items() if torch.is_tensor(v)})
    out.update({"metrics." + k: v for k, v in st.metrics.items()})
    return {k: v.clone() for k, v in out.items()}


def rollout(env, n, steps, each=None):
    """reset + `steps` control steps on rodent_inputs(n); each(env) after the reset and after every step."""
    sf, noise, acts = rodent_inputs(n)
    assert len(acts) >= steps
    st = env.reset(start_frame=torch.from_numpy(sf), noise=torch.from_numpy(noise))
    snaps = [outputs(st)]
    if each:
        each(env)
    for a in acts[:steps]:
        st = env.step(st, torch.from_numpy(a))
        snaps.append(outputs(st))
        if each:
            each(env)
    return snaps


def humanoid_rollout(lib, n, steps):
    with H.backend(lib):
        env = M.humanoid(n, DEV)
    rng = np.random.default_rng(3)
    st = env.reset(5)
    snaps = [outputs(st)]
    for _ in range(steps):
        st = env.step(st, torch.from_numpy(np.clip(0.3 * rng.standard_normal((n, 21)), -1, 1).astype(np.float32)))
        snaps.append(outputs(st))
    return snaps


def same(a_snaps, b_snaps, tag, steps, finite=True):
    """Every output of the reset and of each of the `steps` steps bit for bit, and the state moved."""
    assert len(a_snaps) == len(b_snaps) == steps + 1
    for t, (a, b) in enumerate(zip(a_snaps, b_snaps)):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (tag, t, k)
    assert not torch.equal(a_snaps[-1]["ps.qpos"], a_snaps[0]["ps.qpos"])
    if finite:
        assert all(torch.isfinite(v).all() for k, v in a_snaps[-1].items() if v.is_floating_point()), tag


def small_unroll(lib, n, graphed, steps=20):
    """One unroll of a small intention network over episodes of 8 steps, as a replay of its captured graph or as the eager
    fused unroll: (final state, Transition leaves)."""
    with H.backend(lib):
        env, policy = H.unroll_setup(n, False, 8, lambda b: rodent(b, lib), DEV)
        torch.manual_seed(123)
        state = env.reset(torch.Generator().manual_seed(5))
        key = torch.Generator(device=DEV).manual_seed(11)
        if graphed:
            state, data = acting.GraphedUnroll(env, state, policy, key, steps, extra_fields=("truncation",))()
        else:
            state, data = acting.generate_unroll(env, state, policy, key, steps, extra_fields=("truncation",), fused=True)
    return state, [x.clone() for x in acting._leaves(data)]


def same_unroll(out0, out1, tail=False, steps=20):
    """Every Transition leaf and every carried state tensor bit for bit; tail: and the final state is finite and some logged
    tensor changes between the first and the last of its `steps` steps."""
    (s0, d0), (s1, d1) = out0, out1
    assert len(d0) == len(d1)
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    for n in s0.pipeline_state._FIELDS:
        assert torch.equal(s0.pipeline_state.raw(n), s1.pipeline_state.raw(n)), n
    if tail:
        q = s0.pipeline_state.raw("qpos")
        assert torch.isfinite(q).all() and any(not torch.equal(x[0], x[-1]) for x in d0 if x.dim() > 1 and x.shape[0] == steps)
