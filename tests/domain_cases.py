"""Domain randomisation cases shared by tests/test_domain_randomization.py (host builds) and tests/test_gpu_domain.py:
per-env values of the four raw fields (RodentTracking.with_domain) and the models they stand for."""
import copy

import numpy as np

import helpers as H

FIELDS = ("cg_friction", "act_gain", "dof_damping", "dof_armature")
# the issue's spread: friction x U[0.4, 1.6], gain x U[0.7, 1.3], damping and armature x U[0.5, 2]
SPREAD = {"cg_friction": (0.4, 1.6), "act_gain": (0.7, 1.3), "dof_damping": (0.5, 2.0), "dof_armature": (0.5, 2.0)}


def compiled(m) -> dict:
    """The model's own values of the four fields, one row each (cg_friction: column 0 of the compiled (ncg, 3) array)."""
    return {"cg_friction": np.asarray(m.cg_friction)[:, 0].astype(np.float64), "act_gain": np.asarray(m.act_gain, np.float64),
            "dof_damping": np.asarray(m.dof_damping, np.float64), "dof_armature": np.asarray(m.dof_armature, np.float64)}


def identity(m, B: int) -> dict:
    return {k: np.tile(v, (B, 1)) for k, v in compiled(m).items()}


def random_domain(m, B: int, seed: int = 0) -> dict:
    rng = np.random.default_rng(seed)
    return {k: v * rng.uniform(*SPREAD[k], size=(B, v.size)) for k, v in compiled(m).items()}


def scaled_domain(m, B: int, **scale) -> dict:
    """The compiled values, field k multiplied by scale[k] in every env."""
    return {k: v * scale.get(k, 1.0) for k, v in identity(m, B).items()}


def model_with(m, dom: dict, i: int):
    """Deep copy of CompiledModel `m` with env i's values of the domain in place of the four fields."""
    mi = copy.deepcopy(m)
    fr = np.array(mi.arrays["cg_friction"], dtype=np.float64)
    fr[:, 0] = dom["cg_friction"][i]
    mi.arrays["cg_friction"] = fr
    for k in ("act_gain", "dof_damping", "dof_armature"):
        mi.arrays[k] = np.array(dom[k][i], dtype=np.float64)
    return mi


def row(dom: dict, i: int) -> dict:
    return {k: v[i:i + 1] for k, v in dom.items()}


OUT_KEYS = ("qpos", "qvel", "act", "qacc_warmstart", "xpos", "qfrc_actuator")


def inputs(B, nq=74, nu=30, seed=0):
    rng = np.random.default_rng(seed)
    sf = rng.integers(0, 235, B).astype(np.int32)
    noise = 1e-3 * rng.standard_normal((B, nq))
    acts = np.clip(0.3 * rng.standard_normal((3, B, nu)), -1, 1)
    return sf, noise, acts


def row_err(st, ost, i):
    """Env i of a batch against the oracle state of a one-env batch: scaled errors per output."""
    ps = st.pipeline_state
    out = {k: H.scaled_err(getattr(ps, k).reshape(st.obs.shape[0], -1)[i:i + 1].numpy(), ost[k]) for k in OUT_KEYS}
    out["obs"] = H.scaled_err(st.obs[i:i + 1].numpy(), ost["obs"])
    out["traj"] = H.scaled_err(st.info["traj"][i:i + 1].numpy(), ost["traj"])
    return out


# the ant (generic kernel) as tests/model_cases.py builds it: CG 6 / 6, a seeded gait around the init pose as its clip
ANT_PARAMS = dict(solver="cg", iterations=6, ls_iterations=6)


def ant_clip(m, T=60):
    from vnl_brax_imitation_amd.preprocessing import mjx_preprocess as pp

    t = np.arange(T)[:, None] * 0.02
    q = np.zeros((T, 15))
    q[:, 2], q[:, 3] = 0.55, 1.0
    q[:, 0] = 0.2 * t[:, 0]
    q[:, 7:] = np.array([0.0, 1.0, 0.0, -1.0, 0.0, -1.0, 0.0, 1.0]) + 0.15 * np.sin(2 * np.pi * 1.5 * t + np.arange(8))
    return pp.process_qpos(m, q, max_qvel=20.0, dt=0.02)
