"""Shared test scaffolding: fixtures -> model, clip, oracle, and the host simulation
of the kernels (tests/hostsim) used by the CPU-only tier."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

import vnl_brax_imitation_amd  # noqa: F401  (installs the package alias)
from vnl_brax_imitation_amd import _lib, configs
from vnl_brax_imitation_amd.envs.rodent import packaged_model_path
from vnl_brax_imitation_amd.model import blob, mjcf
from vnl_brax_imitation_amd.preprocessing import mjx_preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BODY_IDXS = [1, 8, 9, 10, 11, 13, 14, 15, 54, 55, 56, 57, 58, 60, 61, 62, 63, 65]


@functools.lru_cache(maxsize=None)
def model() -> mjcf.CompiledModel:
    return mjcf.CompiledModel.load(packaged_model_path())


@functools.lru_cache(maxsize=None)
def golden_clip() -> dict:
    z = np.load(os.path.join(GOLDEN, "groom_clip.npz"))
    return {k: z[k] for k in z.files}


def golden_qpos() -> np.ndarray:
    """(250, 74) qpos rows of the shipped clip."""
    g = golden_clip()
    return np.concatenate([g["position"], g["quaternion"], g["joints"]], axis=1)


@functools.lru_cache(maxsize=None)
def reference_clip() -> pp.ReferenceClip:
    """66-body features rebuilt from the shipped clip's qpos."""
    return pp.process_qpos(model(), golden_qpos())


def model_digest(m: mjcf.CompiledModel) -> str:
    """sha256 over a compiled model's names, scalars and arrays (dtype, shape, bytes), in key order."""
    import hashlib

    h = hashlib.sha256()
    for k in sorted(m.names):
        h.update(f"n {k} {'|'.join(m.names[k])}\n".encode())
    for k in sorted(m.scalars):
        h.update(f"s {k} {float(m.scalars[k])!r}\n".encode())
    for k in sorted(m.arrays):
        a = np.ascontiguousarray(m.arrays[k])
        h.update(f"a {k} {a.dtype.str} {a.shape}\n".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def env_kwargs() -> dict:
    kw = dict(configs.RODENT_ENV_ARGS)
    kw["model"] = model()
    return kw


# the regression builds of csrc/build.py VARIANTS that have a host counterpart: file suffix -> define
HOSTSIM_VARIANTS = {"tail": "VNL_SOLVER_TAIL", "plain": "VNL_SOLVER_PLAIN", "vmemplain": "VNL_VMEM_PLAIN",
                    "ldsplain": "VNL_LDS_PLAIN"}


def build_hostsim(real: str = "float", variant: str | None = None) -> str:
    """g++ build of csrc/vnl_lib.hip against tests/hostsim/stub (kernel launch = serial loop); `variant`: with the define of
    that regression build."""
    src = os.path.join(ROOT, "vnl-brax-imitation_amd", "csrc")
    out = os.path.join(ROOT, "tests", "hostsim", "_build", f"libvnl_hostsim_{real}{'_' + variant if variant else ''}.so")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(ROOT, "include", "vnl.h"), os.path.join(ROOT, "tests", "hostsim", "stub", "hip", "hip_runtime.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        defs = [f"-DVNL_REAL={real}"] + (["-D" + HOSTSIM_VARIANTS[variant]] if variant else [])
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17"] + defs +
                              ["-I" + os.path.join(ROOT, "tests", "hostsim", "stub"), "-x", "c++",
                               os.path.join(src, "vnl_lib.hip"), "-o", out])
    return out


@functools.lru_cache(maxsize=None)
def hostsim_library(real: str = "float", variant: str | None = None) -> C.CDLL:
    return _lib.load_library(build_hostsim(real, variant), env_only=True)


import contextlib  # noqa: E402


@contextlib.contextmanager
def backend(library, dtype=None):
    """Envs constructed inside bind to `library` (the host build of the product source, or a regression build) instead
    of csrc/libvnl.so: the test seam of envs/rodent.py (`_TEST_BACKEND`), kept out of the public constructors."""
    import torch

    from vnl_brax_imitation_amd.envs import rodent as _rodent

    prev = _rodent._TEST_BACKEND
    _rodent._TEST_BACKEND = None if library is None else (library, dtype or torch.float32)
    try:
        yield
    finally:
        _rodent._TEST_BACKEND = prev


def hostsim_backend(real: str = "float"):
    import torch

    return backend(hostsim_library(real), torch.float64 if real == "double" else torch.float32)


def hostsim_env(num_envs: int, real: str = "float", **over):
    """RodentTracking bound to the host simulation (CPU tensors)."""
    import torch

    from vnl_brax_imitation_amd.envs.rodent import RodentTracking

    kw = env_kwargs()
    kw.update(over)
    clip = kw.pop("reference_clip", None) or reference_clip()
    with hostsim_backend(real):
        return RodentTracking(clip, num_envs=num_envs, device="cpu", **kw)


def unroll_setup(B, reset_info, episode_length, make_env, device):
    """make_env(B) under the Episode and AutoReset wrappers, and the acting policy of a small intention network on it."""
    import torch

    from vnl_brax_imitation_amd.envs.wrappers import AutoResetWrapper, EpisodeWrapper
    from vnl_brax_imitation_amd.ppo_imitation import ppo_networks, running_statistics

    base = make_env(B)
    env = AutoResetWrapper(EpisodeWrapper(base, episode_length=episode_length, action_repeat=1),
                           reset_info_on_autoreset=reset_info)
    nets = ppo_networks.make_intention_ppo_networks(base.traj_size, base.observation_size, base.action_size,
                                                    preprocess_observations_fn=running_statistics.normalize,
                                                    intention_latent_size=16, encoder_layer_sizes=(32,),
                                                    decoder_layer_sizes=(32,))
    flat = nets.policy_network.init(torch.Generator().manual_seed(0)).to(device)
    norm = running_statistics.init_state(base.observation_size, device=device)
    return env, ppo_networks.make_inference_fn(nets)((norm, flat))


def make_oracle(env, precision="f64"):
    """Oracle bound to the same model / clip / effective indices as `env`."""
    from oracle.oracle import Oracle

    m = env.sys
    o = Oracle(blob.to_blob(m), precision)
    o.bind_env(env.env_spec(), env.clip_arrays(0), int(m.scalars["nbody"]), int(m.scalars["nq"]),
               int(m.scalars["nv"]), int(m.scalars["nu"]))
    return o


def rel_err(a, b, floor=1e-6):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + floor)))


def scaled_err(a, b):
    """max |a-b| / max(|b|, tiny): error relative to the array's own scale."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))
