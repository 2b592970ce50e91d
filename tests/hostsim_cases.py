"""What the tests of the host builds share (helpers.build_hostsim: the product source and its regression builds compiled by
g++): the inputs and error measures of the float64 parity gate, the model factories, the rollout of a host library, and the
comparison of two rollouts bit for bit."""
import numpy as np
import torch

import domain_cases as D
import helpers as H
import model_cases as M
from variant_cases import outputs

KEYS = ("qpos", "qvel", "act", "qacc_warmstart", "xpos", "qfrc_actuator")


def parity_inputs(B, seed=0):
    rng = np.random.default_rng(seed)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = 1e-3 * rng.standard_normal((B, 74))
    acts = np.clip(0.3 * rng.standard_normal((3, B, 30)), -1, 1)
    return sf, noise, acts


def parity_errors(st, ost, B):
    out = {k: H.scaled_err(getattr(st.pipeline_state, k).reshape(B, -1).numpy(), ost[k]) for k in KEYS}
    out["obs"] = H.scaled_err(st.obs.numpy(), ost["obs"])
    out["traj"] = H.scaled_err(st.info["traj"].numpy(), ost["traj"])
    out["reward"] = H.scaled_err(st.reward.numpy(), ost["reward"]) if np.abs(ost["reward"]).max() > 0 else 0.0
    out["com"] = H.scaled_err(st.pipeline_state.subtree_com_root.numpy(), ost["com1"])
    return out


# ------------------------------------------------------------------------------ make(B) -> (env, action size), no library bound
def _rodent(solver):
    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    def make(B):
        kw = H.env_kwargs()
        if solver == "newton":
            kw["model"] = M.newton_model(1, 4)
        return RodentTracking(H.reference_clip(), num_envs=B, device="cpu", **kw), 30
    return make


def ant_as_rodent_tracking(B):
    return M.ant_as_rodent(B), 8


def rodent_friction(n):
    """A rodent whose envs each have their own friction (the randomised instantiation: friction staged per env)."""
    env, nu = MODELS["rodent_cg_6_6"](n)
    dom = D.random_domain(env.sys, n, 21)
    return env.with_domain({"cg_friction": dom["cg_friction"]}), nu


MODELS = {"rodent_cg_6_6": _rodent("cg"), "rodent_newton_1_4": _rodent("newton"), "ant": lambda B: (M.ant(B), 8),
          "humanoid": lambda B: (M.humanoid(B), 21)}


def host_rollout(library, real, make, B, steps, step_in_backend=False):
    """reset(5) + `steps` control steps (rng seed 3, 0.3 normal clipped to +-1) of make(B) bound to `library`.
    step_in_backend: the whole rollout inside helpers.backend, for a make() whose with_domain binds at every use."""
    dtype = torch.float64 if real == "double" else torch.float32

    def run(env, nu):
        rng = np.random.default_rng(3)
        st = env.reset(5)
        snaps = [outputs(st)]
        for _ in range(steps):
            act = torch.from_numpy(np.clip(0.3 * rng.standard_normal((B, nu)), -1, 1)).to(dtype)
            st = env.step(st, act)
            snaps.append(outputs(st))
        return env, snaps

    with H.backend(library, dtype):
        env, nu = make(B)
        if step_in_backend:
            return run(env, nu)
    return run(env, nu)


def same_rollouts(new, old, tag, equal=torch.equal):
    """Every output of every step `equal`, and the state moved."""
    moved = False
    for t, (a, b) in enumerate(zip(new, old)):
        assert a.keys() == b.keys()
        for k in a:
            assert equal(a[k], b[k]), (*tag, t, k)
        moved = moved or (t > 0 and not torch.equal(a["ps.qpos"], new[0]["ps.qpos"]))
    assert moved


def equal_with_nan(a, b):
    return np.array_equal(a.numpy(), b.numpy(), equal_nan=True)
