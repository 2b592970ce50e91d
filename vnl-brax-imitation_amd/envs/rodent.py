"""RodentTracking: drop-in for reference envs/rodent.py:16-470, natively batched.

Same constructor keywords (rodent.py:17-38; configs/env_config.yaml:32-106), same
reset/step protocol and State fields, same numbers (bug-compatible: SURVEY.md
Appendix C).  Differences a caller sees:

  * the env is batched (it subsumes brax's VmapWrapper): every State field has a
    leading env dimension B = num_envs;
  * the JAX PRNG stream is not reproduced: `reset` draws start frames and noise
    from a torch.Generator, or takes them explicitly (`start_frame=`, `noise=`);
  * `step` updates the State's buffers in place (the kernels own no state);
  * physics + obs/traj/reward/termination run in ONE HIP kernel launch per
    control step through the C-ABI in include/vnl.h (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..model import blob as _blob
from ..model import mjcf as _mjcf
from .base import Env, PipelineState, State

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Test seam, outside every public signature: (library, dtype) that the envs constructed while it is set bind to instead of
# csrc/libvnl.so -- the host-compiled PRODUCT source of tests/hostsim, or a regression build of it.  Set and cleared by
# tests/helpers.py `backend(...)`; None in any product use, where construction fails loudly without a HIP device.
_TEST_BACKEND = None
_METRICS = ("rcom", "rvel", "rtrunk", "rquat", "ract", "rapp", "termination_error")
# the raw model fields a domain may set per env (include/vnl.h: vnl_domain) -> (vnl_dims field of n, smallest allowed value,
# whether the bound itself is allowed; None: any finite value)
DOMAIN_FIELDS = {"cg_friction": ("ngeom_collide", 0.0, False), "act_gain": ("nu", None, False),
                 "dof_damping": ("nv", 0.0, True), "dof_armature": ("nv", 0.0, True)}
# the inertial fields a body domain may set per env, over the bodies of the model as given (include/vnl.h: vnl_body_domain)
# -> (trailing shape after (num_envs, nbody), smallest allowed value; None: any finite value)
BODY_DOMAIN_FIELDS = {"body_mass": ((), 0.0), "body_inertia": ((3,), 0.0), "body_ipos": ((3,), None)}


def packaged_model_path(name: str = "rodent", scale_factor: Optional[float] = 0.9) -> str:
    if scale_factor is None:  # models compiled without the dm_control rescale (humanoid, ant)
        return os.path.join(_PKG, "data", f"{name}.npz")
    return os.path.join(_PKG, "data", f"{name}_scale{scale_factor:g}.npz")


def _load_model(mjcf_path: str, scale_factor: float, solver: str, iterations: int, ls_iterations: int):
    if os.path.exists(mjcf_path):
        return _mjcf.compile_mjcf(mjcf_path, scale_factor=scale_factor, solver=solver, iterations=iterations,
                                  ls_iterations=ls_iterations)
    stem = os.path.splitext(os.path.basename(mjcf_path))[0]
    packaged = packaged_model_path(stem, scale_factor)
    if os.path.exists(packaged):
        model = _mjcf.CompiledModel.load(packaged)
        model.scalars.update(iterations=iterations, ls_iterations=ls_iterations,
                             solver_newton=1 if solver.lower() == "newton" else 0)
        return model
    raise FileNotFoundError(f"{mjcf_path} not found and no packaged compiled model {packaged}")


def domain_ranges_scaled(sys, friction=(0.5, 1.5), gain=None, damping=None, armature=None) -> Dict[str, tuple]:
    """`ranges` for `with_domain_ranges`: absolute (lo, hi) float64 arrays as multiples (lo, hi) of the compiled values of
    `sys` (a CompiledModel); a field given as None is left out -- it is never redrawn.  A compiled value that is negative
    (a gain may be) gets its two multiples in ascending order."""
    compiled = {"cg_friction": np.asarray(sys.cg_friction, np.float64)[:, 0], "act_gain": np.asarray(sys.act_gain, np.float64),
                "dof_damping": np.asarray(sys.dof_damping, np.float64), "dof_armature": np.asarray(sys.dof_armature, np.float64)}
    out = {}
    for k, mult in (("cg_friction", friction), ("act_gain", gain), ("dof_damping", damping), ("dof_armature", armature)):
        if mult is None:
            continue
        a, b = compiled[k] * float(mult[0]), compiled[k] * float(mult[1])
        out[k] = (np.minimum(a, b), np.maximum(a, b))
    return out


def body_domain_ranges_scaled(sys, mass=(0.7, 1.3), inertia=None, ipos=None) -> Dict[str, tuple]:
    """`ranges` for `with_body_domain_ranges`: absolute (lo, hi) float64 arrays over the bodies of `sys` (a CompiledModel) as
    given.  `mass`: multiples (lo, hi) of the compiled masses; `inertia`: multiples of the compiled principal moments, None =
    the mass multiples (with `inertia_with_mass=True` a body then scales like a change of density); `ipos`: (lo, hi) offsets
    in units of each body's |ipos|, added to every component, None = the centre of mass is not redrawn.  A `mass` of None
    leaves mass (and, with `inertia` None, the moments) out."""
    m0 = np.asarray(sys.body_mass, np.float64).reshape(-1)
    i0 = np.asarray(sys.body_inertia, np.float64).reshape(-1, 3)
    p0 = np.asarray(sys.body_ipos, np.float64).reshape(-1, 3)
    out = {}
    if mass is not None:
        out["body_mass"] = (m0 * float(mass[0]), m0 * float(mass[1]))
    inertia = mass if inertia is None else inertia
    if inertia is not None:
        out["body_inertia"] = (i0 * float(inertia[0]), i0 * float(inertia[1]))
    if ipos is not None:
        r = np.linalg.norm(p0, axis=1, keepdims=True)
        out["body_ipos"] = (p0 + float(ipos[0]) * r, p0 + float(ipos[1]) * r)
    return out


def _clamped_take(x: np.ndarray, idx: Sequence[int], axis: int) -> np.ndarray:
    """x[..., idx, ...] with JAX's clamp-out-of-range gather semantics."""
    idx = np.clip(np.asarray(idx, dtype=np.int64), 0, x.shape[axis] - 1)
    return np.take(x, idx, axis=axis)


class RodentTracking(Env):
    def __init__(
        self,
        reference_clip,
        end_eff_names: List[str],
        appendage_names: List[str],
        walker_body_names: List[str],
        joint_names: List[str],
        center_of_mass: str,
        mjcf_path: str = "./assets/rodent.xml",
        scale_factor: float = 0.9,
        solver: str = "cg",
        iterations: int = 6,
        ls_iterations: int = 6,
        healthy_z_range=(0.05, 0.5),
        reset_noise_scale=1e-3,
        clip_length: int = 250,
        sub_clip_length: int = 10,
        ref_traj_length: int = 5,
        termination_threshold: float = 5,
        body_error_multiplier: float = 1.0,
        num_envs: int = 1,
        device: Any = "cuda",
        model: Optional[_mjcf.CompiledModel] = None,
        **kwargs,
    ):
        # --- model (rodent.py:39-63) --------------------------------------------------
        self.sys = model if model is not None else _load_model(mjcf_path, scale_factor, solver, iterations,
                                                               ls_iterations)
        m = self.sys
        self._n_frames = int(kwargs.get("n_frames", 5))  # rodent.py:95-99
        self.backend = "mjx"
        # --- name -> id (rodent.py:65-93) ---------------------------------------------
        self._end_eff_idx = np.array([m.body_id(b) for b in end_eff_names], dtype=np.int32)
        self._app_idx = np.array([m.body_id(b) for b in appendage_names], dtype=np.int32)
        self._com_idx = int(m.body_id(center_of_mass))
        self._body_idxs = np.array([m.body_id(b) for b in walker_body_names], dtype=np.int32)
        self._joint_idxs = np.array([m.joint_id(j) for j in joint_names], dtype=np.int32)

        self._healthy_z_range = healthy_z_range
        self._reset_noise_scale = float(reset_noise_scale)
        self._termination_threshold = float(termination_threshold)
        self._body_error_multiplier = float(body_error_multiplier)
        self._clip_length = int(clip_length)
        self._sub_clip_length = int(sub_clip_length)
        self._ref_traj_length = int(ref_traj_length)
        if self._sub_clip_length > self._clip_length:
            raise ValueError("episode_length cannot be greater than clip_length!")  # rodent.py:116-117

        self._build(reference_clip, num_envs, device)

    # env-variant knobs (include/vnl.h VNL_ENV_*): RodentTracking's glue by default
    _env_flags = 0
    _done_threshold = 0.0
    _reward_weights = None  # with ENV_WEIGHTS: (rcom, rvel, rtrunk, rquat, ract, rapp)
    _use_clip_com = False

    def _build(self, reference_clip, num_envs, device, _library=None, _dtype=torch.float32):
        # everything set so far is configuration; what follows is per-instance device state (with_num_envs)
        if _library is None and _TEST_BACKEND is not None:  # tests/helpers.py `backend(...)` only; never set by the product
            _library, _dtype = _TEST_BACKEND
        self._config_attrs = dict(self.__dict__)
        self._build_args = (reference_clip, device, _library, _dtype)
        m = self.sys
        healthy_z_range = self._healthy_z_range
        # --- clip (rodent.py:112-115): filter body_positions to the tracked bodies -----
        clip = reference_clip.as_multi() if hasattr(reference_clip, "as_multi") else reference_clip
        f32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float32)  # noqa: E731
        bp = f32(clip.body_positions)
        self._clip = dict(
            position=f32(clip.position), quaternion=f32(clip.quaternion), joints=f32(clip.joints),
            body_positions=np.ascontiguousarray(_clamped_take(bp, self._body_idxs, axis=-2)),
            velocity=f32(clip.velocity), angular_velocity=f32(clip.angular_velocity),
            joints_velocity=f32(clip.joints_velocity),
        )
        if self._use_clip_com:
            self._clip["center_of_mass"] = f32(clip.center_of_mass)
        self._num_clips, self._T = self._clip["position"].shape[:2]
        nb = len(self._body_idxs)
        nj = int(m.scalars["nq"]) - 7
        # effective indices after the reference's id-vs-column mix-ups + JAX clamping (Appendix C.4/C.5)
        self._app_ref_col = np.clip(self._app_idx, 0, nb - 1).astype(np.int32)
        self._com_ref_col = int(np.clip(self._com_idx, 0, nb - 1))
        self._joint_cols = np.clip(self._joint_idxs, 0, nj - 1).astype(np.int32)

        # --- device library -----------------------------------------------------------------
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if _library is None:
            if self.device.type != "cuda":
                raise _lib.VnlError("RodentTracking runs on a HIP device only (device='cuda[:i]'); no CPU fallback")
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            _library = _lib.load_library()
        self._L = _library
        self._dtype = _dtype  # float64 only with the test-only host simulation built with -DVNL_REAL=double
        blob = _blob.to_blob(m)
        self._blob = C.create_string_buffer(blob, len(blob))
        self._model_h = C.c_void_p()
        _lib.check(self._L, self._L.vnl_model_create(self._blob, len(blob), C.byref(self._model_h)))
        spec = _lib.EnvSpec()
        spec.clip_frames, spec.num_clips = self._T, self._num_clips
        spec.ref_traj_length, spec.sub_clip_length, spec.n_frames = self._ref_traj_length, self._sub_clip_length, self._n_frames
        spec.num_track_bodies, spec.num_end_eff = nb, len(self._end_eff_idx)
        spec.num_appendages, spec.num_joint_cols, spec.com_ref_col = len(self._app_idx), len(self._joint_cols), self._com_ref_col
        self._keep = [self._body_idxs, self._end_eff_idx, self._app_idx, self._app_ref_col, self._joint_cols]
        ip = lambda a: a.ctypes.data_as(_lib.i32p)  # noqa: E731
        fp = lambda a: a.ctypes.data_as(_lib.f32p)  # noqa: E731
        spec.body_idxs, spec.end_eff_idx, spec.app_body = ip(self._body_idxs), ip(self._end_eff_idx), ip(self._app_idx)
        spec.app_ref_col, spec.joint_cols = ip(self._app_ref_col), ip(self._joint_cols)
        spec.healthy_z_lo, spec.healthy_z_hi = float(healthy_z_range[0]), float(healthy_z_range[1])
        spec.termination_threshold, spec.body_error_multiplier = self._termination_threshold, self._body_error_multiplier
        spec.flags, spec.done_threshold = int(self._env_flags), float(self._done_threshold)
        for i, w in enumerate(self._reward_weights or ()):
            spec.reward_weights[i] = float(w)
        for k, v in self._clip.items():
            setattr(spec, k, fp(v))
        self._env_h = C.c_void_p()
        dev_index = self.device.index if self.device.type == "cuda" else 0
        _lib.check(self._L, self._L.vnl_env_create(self._model_h, C.byref(spec), self.num_envs, dev_index,
                                                   C.byref(self._env_h)))
        self.dims = _lib.Dims()
        _lib.check(self._L, self._L.vnl_env_dims(self._env_h, C.byref(self.dims)))
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(0)

    def with_num_envs(self, num_envs: int) -> "RodentTracking":
        """A second env of the same configuration (model, clip, reward parameters) with its own batch of `num_envs`
        envs on the device -- the evaluator's env when num_eval_envs differs from the training batch."""
        new = object.__new__(type(self))
        new.__dict__.update(self._config_attrs)
        new._build(self._build_args[0], int(num_envs), *self._build_args[1:])
        if self._domain_ranges is not None:  # (the ranges, not the tables: the new env's tables hold the compiled values)
            new._set_domain_ranges(self._domain_ranges)
        if self._body_domain_ranges is not None:
            new._set_body_domain_ranges(self._body_domain_ranges)
        return new

    _domain = None  # {field: (num_envs, n) float64 tensor} of a randomised env (with_domain), else None
    _body_domain = None  # {field: (num_envs, nbody[, 3]) float64 tensor} of a body-randomised env (with_body_domain), else None

    _domain_ranges = None  # ({field: (lo, hi) float64 (n,) CPU tensors}, shared field names) of with_domain_ranges, else None

    def _set_domain_ranges(self, ranges) -> None:
        """vnl_env_set_domain_ranges of already validated ranges (the library copies them: synchronous)"""
        bounds, shared = ranges
        desc, keep = _lib.DomainRanges(), []
        for f, k in enumerate(DOMAIN_FIELDS):
            if k in bounds:
                lo, hi = (t.to(self.device).contiguous() for t in bounds[k])
                keep += [lo, hi]
                desc.lo[f], desc.hi[f] = lo.data_ptr(), hi.data_ptr()
                desc.shared |= (1 << f) if k in shared else 0
        _lib.check(self._L, self._L.vnl_env_set_domain_ranges(self._env_h, C.byref(desc), self._stream()))
        self._domain_ranges = ({k: tuple(t.clone() for t in v) for k, v in bounds.items()}, tuple(shared))

    # ({field: (lo, hi) float64 (nbody[, 3]) CPU tensors}, shared field names, inertia_with_mass) of with_body_domain_ranges
    _body_domain_ranges = None

    def _set_body_domain_ranges(self, ranges) -> None:
        """vnl_env_set_body_domain_ranges of already shaped ranges (the library validates and copies them: synchronous)"""
        bounds, shared, with_mass = ranges
        desc, keep = _lib.BodyDomainRanges(), []
        for f, k in enumerate(BODY_DOMAIN_FIELDS):
            if k in bounds:
                lo, hi = (t.to(self.device).contiguous() for t in bounds[k])
                keep += [lo, hi]
                desc.lo[f], desc.hi[f] = lo.data_ptr(), hi.data_ptr()
                desc.shared |= (1 << f) if k in shared else 0
        desc.flags = _lib.BODY_RANGES_INERTIA_WITH_MASS if with_mass else 0
        rc = self._L.vnl_env_set_body_domain_ranges(self._env_h, C.byref(desc), self._stream())
        if rc == -1:  # VNL_ERR_ARG: what the library checks (bad bounds, a jointed body without mass at the lower bounds, ...)
            raise ValueError(self._L.vnl_last_error().decode())
        _lib.check(self._L, rc)
        self._body_domain_ranges = ({k: tuple(t.clone() for t in v) for k, v in bounds.items()}, tuple(shared), bool(with_mass))

    def _with_domains(self, tables, body_tables, ranges="carry", body_ranges="carry") -> "RodentTracking":
        """A new env of this configuration and num_envs with the given parts of a domain (already validated; None: unset);
        the ranges of this env (both sets) are carried over unless others are given."""
        new = object.__new__(type(self))
        new.__dict__.update(self._config_attrs)
        new._build(self._build_args[0], self.num_envs, *self._build_args[1:])
        if tables is not None:
            desc = _lib.Domain(**{k: C.c_void_p(t.data_ptr()) for k, t in tables.items()})
            _lib.check(new._L, new._L.vnl_env_set_domain(new._env_h, C.byref(desc), new._stream()))  # (copies: synchronous)
            new._domain = dict(tables)
        if body_tables is not None:
            desc = _lib.BodyDomain(**{k: C.c_void_p(t.data_ptr()) for k, t in body_tables.items()})
            rc = new._L.vnl_env_set_body_domain(new._env_h, C.byref(desc), new._stream())
            if rc == -1:  # VNL_ERR_ARG: what only the per-env fold can tell (a jointed body without mass, ...)
                raise ValueError(new._L.vnl_last_error().decode())
            _lib.check(new._L, rc)
            new._body_domain = dict(body_tables)
        ranges = self._domain_ranges if isinstance(ranges, str) else ranges
        if ranges is not None:
            new._set_domain_ranges(ranges)
        body_ranges = self._body_domain_ranges if isinstance(body_ranges, str) else body_ranges
        if body_ranges is not None:
            new._set_body_domain_ranges(body_ranges)
        return new

    def with_body_domain_ranges(self, ranges: Mapping[str, Any], shared: Sequence[str] = (),
                                inertia_with_mass: bool = False) -> "RodentTracking":
        """A NEW env of the same model, clip, parameters and num_envs whose envs get a new BODY domain per EPISODE
        (include/vnl.h: vnl_env_set_body_domain_ranges): `reset_done` -- the fresh auto-reset -- draws mass, principal moments
        and centre of mass of every env it resets anew inside the reset kernel and folds the welded bodies there, and
        `redraw_domain` does so on request (the first episode).

          ranges  {field: (lo, hi)} with the field names of `with_body_domain`; lo / hi are scalars or arrays of shape
                  (nbody,) / (nbody, 3): ABSOLUTE bounds per element (`body_domain_ranges_scaled` builds them).  Row 0, the
                  world body, is never drawn: its bounds are replaced by the compiled values
          shared  names of fields of `ranges` that take ONE uniform per (env, episode) for all their elements
          inertia_with_mass  moment (b, k) takes the uniform of body b's mass draw (needs mass ranges): with bounds that are the
                  same multiples of the compiled values a body scales like a change of density and stays physical; the
                  moments' triangle inequality is not checked otherwise

        A field left out is never redrawn: it keeps the `with_body_domain` values of this env, else the compiled ones.  Carried
        by `with_domain` / `with_body_domain` / `with_domain_ranges` / `with_num_envs` exactly as the four-field ranges are.
        Raises ValueError on an unknown field, a wrong shape, or what the library refuses: non-finite bounds, lo > hi, a mass
        or moment lo < 0, the flag without mass ranges, or lower bounds that leave a body with dofs without mass or without a
        member of three positive moments, or a total mass of zero."""
        nbody, bounds = int(self.dims.nbody), {}
        compiled = {"body_mass": self.sys.body_mass, "body_inertia": self.sys.body_inertia, "body_ipos": self.sys.body_ipos}
        for k, v in dict(ranges).items():
            if k not in BODY_DOMAIN_FIELDS:
                raise ValueError(f"unknown body domain field {k!r}: expected some of {sorted(BODY_DOMAIN_FIELDS)}")
            shape = (nbody,) + BODY_DOMAIN_FIELDS[k][0]
            try:
                lo, hi = v
            except (TypeError, ValueError):
                raise ValueError(f"body domain range {k!r} must be a (lo, hi) pair") from None
            pair = []
            for name, x in (("lo", lo), ("hi", hi)):
                t = torch.as_tensor(x).detach().to(dtype=torch.float64, device="cpu")
                if t.dim() == 0:
                    t = t.expand(shape)
                if tuple(t.shape) != shape:
                    raise ValueError(f"body domain range {k!r}: {name} must be a scalar or have shape {shape}, got {tuple(t.shape)}")
                t = t.contiguous().clone()
                t[0] = torch.as_tensor(np.asarray(compiled[k], np.float64).reshape(shape)[0])
                pair.append(t)
            bounds[k] = tuple(pair)
        shared = tuple(shared)
        for k in shared:
            if k not in bounds:
                raise ValueError(f"shared field {k!r} has no range")
        if inertia_with_mass and "body_mass" not in bounds:
            raise ValueError("inertia_with_mass needs a range for 'body_mass'")
        return self._with_domains(self._domain, self._body_domain, body_ranges=(bounds, shared, bool(inertia_with_mass)))

    @property
    def body_domain_ranges(self) -> Optional[Dict[str, Any]]:
        """{field: (lo, hi) float64 (nbody[, 3]) tensors} of `with_body_domain_ranges` plus "shared": the shared field names
        and "inertia_with_mass"; or None."""
        if self._body_domain_ranges is None:
            return None
        bounds, shared, with_mass = self._body_domain_ranges
        return dict({k: tuple(t.clone() for t in v) for k, v in bounds.items()}, shared=tuple(shared), inertia_with_mass=with_mass)

    def with_domain_ranges(self, ranges: Mapping[str, Any], shared: Sequence[str] = ()) -> "RodentTracking":
        """A NEW env of the same model, clip, parameters and num_envs whose envs get a new physical domain per EPISODE
        (include/vnl.h: vnl_env_set_domain_ranges): `reset_done` -- the fresh auto-reset -- draws the fields in `ranges` anew
        for every env it resets, inside the reset kernel, and `redraw_domain` does so on request (the first episode).

          ranges  {field: (lo, hi)} with the field names of `with_domain`; lo / hi are scalars or arrays of the field's
                  length: ABSOLUTE bounds per element (`domain_ranges_scaled` builds them from multiples of the compiled values)
          shared  names of fields of `ranges` that take ONE uniform per (env, episode) for all their elements (every geom's
                  friction scaled alike), instead of one per element

        A field left out is never redrawn.  Domains of this env (with_domain, with_body_domain) are carried over: the tables
        keep those values until an env's first redraw; the body domain is redrawn only under `with_body_domain_ranges`.  `with_domain` /
        `with_body_domain` of the result carry the ranges, `with_num_envs` carries the ranges but not the tables.  Raises
        ValueError on an unknown field, a wrong length, or bad bounds (non-finite, lo > hi, friction lo <= 0, damping or
        armature lo < 0)."""
        d, bounds = self.dims, {}
        for k, v in dict(ranges).items():
            if k not in DOMAIN_FIELDS:
                raise ValueError(f"unknown domain field {k!r}: expected some of {sorted(DOMAIN_FIELDS)}")
            dim, least, closed = DOMAIN_FIELDS[k]
            n = int(getattr(d, dim))
            try:
                lo, hi = v
            except (TypeError, ValueError):
                raise ValueError(f"domain range {k!r} must be a (lo, hi) pair") from None
            pair = []
            for name, x in (("lo", lo), ("hi", hi)):
                t = torch.as_tensor(x).detach().to(dtype=torch.float64, device="cpu")
                if t.dim() == 0:
                    t = t.expand(n)
                if tuple(t.shape) != (n,):
                    raise ValueError(f"domain range {k!r}: {name} must be a scalar or have shape ({n},), got {tuple(t.shape)}")
                if not bool(torch.isfinite(t).all()):
                    raise ValueError(f"domain range {k!r}: {name} has non-finite values")
                pair.append(t.contiguous().clone())
            if not bool((pair[0] <= pair[1]).all()):
                raise ValueError(f"domain range {k!r}: lo must not exceed hi")
            if least is not None and not bool(((pair[0] >= least) if closed else (pair[0] > least)).all()):
                raise ValueError(f"domain range {k!r}: lo must be {'>=' if closed else '>'} {least}")
            bounds[k] = tuple(pair)
        shared = tuple(shared)
        for k in shared:
            if k not in bounds:
                raise ValueError(f"shared field {k!r} has no range")
        return self._with_domains(self._domain, self._body_domain, ranges=(bounds, shared))

    @property
    def domain_ranges(self) -> Optional[Dict[str, Any]]:
        """{field: (lo, hi) float64 (n,) tensors} of `with_domain_ranges` plus "shared": the shared field names; or None."""
        if self._domain_ranges is None:
            return None
        bounds, shared = self._domain_ranges
        return dict({k: tuple(t.clone() for t in v) for k, v in bounds.items()}, shared=tuple(shared))

    def redraw_domain(self, *, seed: int, step_base, step_offset: int = 0, env_offset: int = 0,
                      mask: Optional[torch.Tensor] = None, initial: bool = False) -> None:
        """The domain of the envs whose `mask` (B,) is nonzero (None: every env) drawn anew from this env's ranges, in place
        (vnl_env_redraw_domain): the draw `reset_done` makes for the envs it resets, keyed by (seed, step_base[0] +
        step_offset, env_offset + env index) -- ppo_imitation/philox.py domain_draws, body_domain_draws -- as a launch of its
        own; both kinds of ranges (with_domain_ranges, with_body_domain_ranges) are drawn, whichever the env has.
        `initial=True` draws from a block range of its own: the domain of a FIRST episode differs from that of a reset at the
        same counter.  `step_base`: int64 [1] on the env's device (only read), or an int.  ValueError without ranges."""
        if self._domain_ranges is None and self._body_domain_ranges is None:
            raise ValueError("redraw_domain: this env has no domain ranges (with_domain_ranges, with_body_domain_ranges)")
        B = self.num_envs
        if not isinstance(step_base, torch.Tensor):
            step_base = torch.tensor([int(step_base)], dtype=torch.int64, device=self.device)
        if step_base.dtype != torch.int64 or step_base.numel() != 1 or step_base.device != self.device:
            raise ValueError("step_base must be an int or an int64 tensor of one element on the env's device")
        mk = None
        if mask is not None:
            if tuple(mask.shape) != (B,):
                raise ValueError(f"mask must be ({B},), got {tuple(mask.shape)}")
            mk = mask.to(device=self.device, dtype=torch.float32).contiguous()
        nz = _lib.ResetNoise()
        nz.seed, nz.step_base = int(seed) & 0xFFFFFFFFFFFFFFFF, step_base.data_ptr()
        nz.step_offset, nz.env_offset = int(step_offset), int(env_offset)
        _lib.check(self._L, self._L.vnl_env_redraw_domain(self._env_h, None if mk is None else mk.data_ptr(), C.byref(nz),
                                                          int(bool(initial)), self._stream()))
        self._hold = (mk, step_base)

    def with_domain(self, domain: Mapping[str, Any]) -> "RodentTracking":
        """A NEW env of the same model, clip, parameters and num_envs whose envs each run with their own values of the raw
        model fields in `domain` (brax `randomization_fn`, MJX semantics; include/vnl.h: vnl_env_set_domain):

          cg_friction  (num_envs, ncg)  sliding friction of each collidable geom's contact rows
          act_gain     (num_envs, nu)   actuator gain (gainprm[0])
          dof_damping, dof_armature  (num_envs, nv)

        A field left out keeps the model's value.  Derived constants (invweight0, meaninertia) stay as compiled; the contact
        rows' inverse weight follows friction.  Values are fixed for the env's lifetime (auto-reset keeps them) unless the env
        has ranges (with_domain_ranges: carried over by this call, a fresh reset then redraws the env's domain).  Neither this
        env nor its CompiledModel is changed.  A body domain of this env (with_body_domain) is carried over.  `with_num_envs`
        of the result carries NO domain: an eval env is randomised by a call of its own.  Raises ValueError on an unknown
        field, a wrong shape or a bad value (non-finite, friction <= 0, damping or armature < 0)."""
        d = self.dims
        tables = {}
        for k, v in dict(domain).items():
            if k not in DOMAIN_FIELDS:
                raise ValueError(f"unknown domain field {k!r}: expected some of {sorted(DOMAIN_FIELDS)}")
            dim, lo, closed = DOMAIN_FIELDS[k]
            t = torch.as_tensor(v).detach().to(dtype=torch.float64)
            shape = (self.num_envs, int(getattr(d, dim)))
            if tuple(t.shape) != shape:
                raise ValueError(f"domain field {k!r} must have shape {shape}, got {tuple(t.shape)}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"domain field {k!r} has non-finite values")
            if lo is not None and not bool(((t >= lo) if closed else (t > lo)).all()):
                raise ValueError(f"domain field {k!r} must be {'>=' if closed else '>'} {lo}")
            tables[k] = t.to(self.device).contiguous()
        return self._with_domains(tables, self._body_domain)

    def with_body_domain(self, bodies: Mapping[str, Any]) -> "RodentTracking":
        """A NEW env of the same model, clip, parameters and num_envs whose envs each run with their own inertial fields,
        over the bodies of the model as given (MJX semantics; include/vnl.h: vnl_env_set_body_domain):

          body_mass     (num_envs, nbody)
          body_inertia  (num_envs, nbody, 3)  principal moments in the frame of the compiled body_iquat
          body_ipos     (num_envs, nbody, 3)  centre of mass in the body frame

        A field left out keeps the model's values; row 0 (the world body) is not read.  The library folds welded bodies into
        their parents per env and derives 1 / total mass per env; invweight0, meaninertia and body_subtreemass stay as
        compiled.  A four-field domain of this env (with_domain) is carried over, and `with_domain` of the result carries the
        body domain; `with_num_envs` carries neither.  Neither this env nor its CompiledModel is changed.  Raises ValueError
        on an unknown field, a wrong shape, a non-finite value, a negative mass or moment, a body with dofs left without
        mass or inertia once welded bodies are folded in, or a total mass of zero."""
        nbody = int(self.dims.nbody)
        tables = {}
        for k, v in dict(bodies).items():
            if k not in BODY_DOMAIN_FIELDS:
                raise ValueError(f"unknown body domain field {k!r}: expected some of {sorted(BODY_DOMAIN_FIELDS)}")
            tail, lo = BODY_DOMAIN_FIELDS[k]
            t = torch.as_tensor(v).detach().to(dtype=torch.float64)
            shape = (self.num_envs, nbody) + tail
            if tuple(t.shape) != shape:
                raise ValueError(f"body domain field {k!r} must have shape {shape}, got {tuple(t.shape)}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"body domain field {k!r} has non-finite values")
            if lo is not None and not bool((t[:, 1:] >= lo).all()):
                raise ValueError(f"body domain field {k!r} must be >= {lo}")
            tables[k] = t.to(self.device).contiguous()
        return self._with_domains(self._domain, tables)

    @property
    def domain(self) -> Optional[Dict[str, torch.Tensor]]:
        """The per-env field values this env was built with (with_domain and with_body_domain, both parts), or None."""
        if self._domain is None and self._body_domain is None:
            return None
        return dict(self._domain or {}, **(self._body_domain or {}))

    def domain_table(self, name: str) -> torch.Tensor:
        """(num_envs, n) copy of one of the library's per-env tables of a randomised env (vnl_env_scratch "dom_mu",
        "dom_invw", "dom_gain", "dom_damp", "dom_arm"; the body tables over the dynamic bodies "dom_mass", "dom_ipos",
        "dom_inertia6", "dom_tminv"): what the kernels read."""
        ptr, cnt = C.c_void_p(), C.c_int32()
        _lib.check(self._L, self._L.vnl_env_scratch(self._env_h, name.encode(), C.byref(ptr), C.byref(cnt)))
        total = self.num_envs * cnt.value
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            flat = torch.empty(total, dtype=self._dtype, device=self.device)
            esz = flat.element_size()
            rc = C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(flat.data_ptr()), ptr, C.c_size_t(esz * total), C.c_int(3))
            if rc != 0:
                raise _lib.VnlError(f"hipMemcpy failed: {rc}")
            flat = flat.cpu()
        else:
            ct = C.c_double if self._dtype == torch.float64 else C.c_float
            flat = torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(total,)).copy())
        return flat.view(self.num_envs, cnt.value)

    def _copy_domain_tables(self, saved: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The five four-field tables and the four body tables as one flat tensor on the env's device (they are one
        allocation, "dom_mu" first), or -- given such a tensor -- written back: a caller that runs fresh resets it must not
        keep (the warm-up of a graph capture) puts a redrawn domain, of either kind, back with this.  Synchronous."""
        ptr, cnt = C.c_void_p(), C.c_int32()
        _lib.check(self._L, self._L.vnl_env_scratch(self._env_h, b"dom_mu", C.byref(ptr), C.byref(cnt)))
        d = self.dims
        total = self.num_envs * (2 * int(d.ngeom_collide) + int(d.nu) + 2 * int(d.nv) + 10 * int(d.nbody_dynamic) + 1)
        flat = saved if saved is not None else torch.empty(total, dtype=self._dtype, device=self.device)
        assert flat.numel() == total and flat.dtype == self._dtype and flat.is_contiguous()
        nbytes = C.c_size_t(flat.element_size() * total)
        src, dst = (C.c_void_p(flat.data_ptr()), ptr) if saved is not None else (ptr, C.c_void_p(flat.data_ptr()))
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            rc = C.CDLL("libamdhip64.so").hipMemcpy(dst, src, nbytes, C.c_int(3))
            if rc != 0:
                raise _lib.VnlError(f"hipMemcpy failed: {rc}")
        else:
            C.memmove(dst, src, nbytes)
        return flat

    def __del__(self):
        try:
            if getattr(self, "_env_h", None):
                self._L.vnl_env_destroy(self._env_h)
            if getattr(self, "_model_h", None):
                self._L.vnl_model_destroy(self._model_h)
        except Exception:
            pass

    # --- brax Env protocol -----------------------------------------------------------------
    @property
    def observation_size(self) -> int:
        return int(self.dims.obs_size)

    @property
    def traj_size(self) -> int:
        return int(self.dims.traj_size)

    @property
    def action_size(self) -> int:
        return int(self.dims.nu)

    @property
    def dt(self) -> float:
        return float(self.sys.scalars["timestep"]) * self._n_frames

    def env_spec(self) -> Dict[str, Any]:
        """Effective env description (also what tests hand to the CPU oracle)."""
        return dict(
            T=self._T, ref_len=self._ref_traj_length, sub_clip_length=self._sub_clip_length, n_frames=self._n_frames,
            nb=len(self._body_idxs), nee=len(self._end_eff_idx), napp=len(self._app_idx), njc=len(self._joint_cols),
            com_ref_col=self._com_ref_col, body_idxs=self._body_idxs.tolist(), end_eff_idx=self._end_eff_idx.tolist(),
            app_body=self._app_idx.tolist(), app_ref_col=self._app_ref_col.tolist(),
            joint_cols=self._joint_cols.tolist(), healthy_z_lo=self._healthy_z_range[0],
            healthy_z_hi=self._healthy_z_range[1], termination_threshold=self._termination_threshold,
            body_error_multiplier=self._body_error_multiplier, flags=int(self._env_flags),
            done_threshold=float(self._done_threshold),
            reward_weights=list(self._reward_weights) if self._reward_weights else None,
        )

    def clip_arrays(self, clip: int = 0) -> Dict[str, np.ndarray]:
        return {k: v[clip] for k, v in self._clip.items()}

    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _alloc_state(self) -> State:
        B, dv, d = self.num_envs, self.device, self.dims
        ps = PipelineState.allocate(d, B, dv, self._dtype)
        z = lambda n, dt=self._dtype: torch.zeros((B, n) if n else (B,), dtype=dt, device=dv)  # noqa: E731
        raw = dict(obs=z(d.obs_size), reward=z(0), done=z(0), metrics=z(7), traj=z(d.traj_size),
                   termination_error=z(0), cur_frame=z(0, torch.int32), sub_clip_frame=z(0, torch.int32),
                   clip_id=z(0, torch.int32))
        metrics = {k: raw["metrics"][:, i] for i, k in enumerate(_METRICS)}
        info = dict(cur_frame=raw["cur_frame"], sub_clip_frame=raw["sub_clip_frame"], traj=raw["traj"],
                    termination_error=raw["termination_error"], clip_id=raw["clip_id"], _raw=raw)
        return State(ps, raw["obs"], raw["reward"], raw["done"], metrics, info)

    def _ptrs(self, state: State) -> _lib.StatePtrs:
        raw, ps = state.info["_raw"], state.pipeline_state
        p = _lib.StatePtrs()
        for k in PipelineState._FIELDS:
            setattr(p, k, ps.raw(k).data_ptr())
        for k in ("obs", "reward", "done", "metrics", "traj", "termination_error", "cur_frame", "sub_clip_frame",
                  "clip_id"):
            setattr(p, k, raw[k].data_ptr())
        return p

    def reset(self, rng=None, *, start_frame: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
              clip_id: Optional[torch.Tensor] = None, out: Optional[State] = None) -> State:
        """rodent.py:119-176.  `rng`: None (internal generator), an int seed or a torch.Generator (CPU).
        Explicit `start_frame` (B,) int and `noise` (B, nq) (already scaled) override the draws."""
        B, nq = self.num_envs, int(self.dims.nq)
        gen = self._gen
        if isinstance(rng, torch.Generator):
            gen = rng
        elif rng is not None:
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(rng))
        if start_frame is None:
            hi = self._clip_length - self._sub_clip_length - self._ref_traj_length  # rodent.py:123-128
            start_frame = torch.randint(0, max(hi, 1), (B,), generator=gen, dtype=torch.int32)
        if noise is None:
            noise = self._reset_noise_scale * torch.randn((B, nq), generator=gen, dtype=torch.float32)
        if clip_id is None:
            clip_id = (torch.zeros(B, dtype=torch.int32) if self._num_clips == 1 else
                       torch.randint(0, self._num_clips, (B,), generator=gen, dtype=torch.int32))
        state = out if out is not None else self._alloc_state()
        sf = torch.as_tensor(start_frame, dtype=torch.int32).to(self.device).contiguous()
        nz = torch.as_tensor(noise).to(device=self.device, dtype=self._dtype).contiguous()  # [B][nq]
        state.info["_raw"]["clip_id"].copy_(torch.as_tensor(clip_id, dtype=torch.int32).to(self.device))
        p = self._ptrs(state)
        _lib.check(self._L, self._L.vnl_env_reset(self._env_h, sf.data_ptr(), nz.data_ptr(), C.byref(p),
                                                  self._stream()))
        self._hold = (sf, nz)  # keep inputs alive until the stream has consumed them
        return state

    def _start_hi(self) -> int:
        """Start frames of this env's own `reset` are uniform in [0, _start_hi()) (rodent.py:123-128); at least 1."""
        return max(self._clip_length - self._sub_clip_length - self._ref_traj_length, 1)

    def reset_done(self, state: State, mask: torch.Tensor, *, seed: int, step_base: torch.Tensor, step_offset: int = 0,
                   env_offset: int = 0, logs=(), record: Optional[Dict[str, torch.Tensor]] = None, priority=None,
                   truncation: Optional[torch.Tensor] = None) -> State:
        """A fresh episode, in place, for the envs whose `mask` (B,) is nonzero (vnl_env_reset_done): start frame in
        [0, _start_hi()) -- the range of this env's own `reset` --, clip and reset noise drawn in the kernel from the counter-based
        stream keyed by (seed, step_base[0] + step_offset, env_offset + env index) -- ppo_imitation/philox.py reset_draws.
        reward, done and metrics keep the terminal step's values; nothing of an unmasked env changes.  `step_base`: int64 [1]
        on the env's device, only read (the caller advances it).  `logs`: up to 8 (src, log) pairs of (B[, w]) float32 /
        int32 tensors, log <- src for every env after the reset.  `record`: optional dict of int32 (B,) "start_frame",
        "clip_id" and (B, nq) "noise" tensors that receive the draws of the reset envs.
        `priority` (envs/start_priority.py StartPriority, or any object with its tensors `cdf`, `count_ended`,
        `count_failed`; the counters may be None): start frame and clip are drawn from its table instead -- philox.py
        weighted_cells -- and the episodes that end here are counted into its counters (vnl_env_reset_done_weighted), except
        those whose `truncation` (B,) float32 entry is nonzero."""
        B = self.num_envs
        if tuple(mask.shape) != (B,):
            raise ValueError(f"mask must be ({B},), got {tuple(mask.shape)}")
        if step_base.dtype != torch.int64 or step_base.numel() != 1 or step_base.device != self.device:
            raise ValueError("step_base must be an int64 tensor of one element on the env's device")
        mk = mask.to(device=self.device, dtype=torch.float32).contiguous()
        nz = _lib.ResetNoise()
        nz.seed, nz.step_base = int(seed) & 0xFFFFFFFFFFFFFFFF, step_base.data_ptr()
        nz.step_offset, nz.env_offset = int(step_offset), int(env_offset)
        nz.start_hi = self._start_hi()
        nz.noise_scale = self._reset_noise_scale
        record = record or {}
        for k, dt in (("start_frame", torch.int32), ("clip_id", torch.int32), ("noise", self._dtype)):
            t = record.get(k)
            if t is not None:
                if t.dtype != dt or not t.is_contiguous() or t.shape[0] != B or t.device != self.device:
                    raise ValueError(f"record[{k!r}] must be a contiguous {dt} tensor with {B} rows on the env's device")
                setattr(nz, k + "_out", t.data_ptr())
        logs = tuple(logs)
        if len(logs) > _lib.RESET_MAX_LOGS:
            raise ValueError(f"at most {_lib.RESET_MAX_LOGS} logs")
        arr = (_lib.ResetLog * max(len(logs), 1))()
        for o, (src, log) in zip(arr, logs):
            if src.dtype not in (torch.float32, torch.int32) or log.dtype != src.dtype or src.shape != log.shape or \
                    src.shape[0] != B or not (src.is_contiguous() and log.is_contiguous()):
                raise ValueError("a log is a (src, log) pair of contiguous float32 / int32 tensors of one shape (B[, w])")
            o.src, o.log, o.width = src.data_ptr(), log.data_ptr(), src.numel() // B
        p = self._ptrs(state)
        if priority is None:
            if truncation is not None:
                raise ValueError("truncation has no meaning without a priority: nothing is counted")
            _lib.check(self._L, self._L.vnl_env_reset_done(self._env_h, mk.data_ptr(), C.byref(nz), C.byref(p), arr, len(logs),
                                                           self._stream()))
        else:
            pr = _lib.StartPriorityDesc()
            words = [priority.cdf, priority.count_ended, priority.count_failed]
            for t in words:
                if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != self.device
                                      or t.numel() != words[0].numel()):
                    raise ValueError("a priority's cdf and counters are contiguous int32 (ncell,) tensors on the env's device")
            pr.cdf, pr.ncell = priority.cdf.data_ptr(), priority.cdf.numel()
            pr.ended = None if words[1] is None else words[1].data_ptr()
            pr.failed = None if words[2] is None else words[2].data_ptr()
            if truncation is not None:
                if truncation.dtype != torch.float32 or tuple(truncation.shape) != (B,) or not truncation.is_contiguous() or \
                        truncation.device != self.device:
                    raise ValueError(f"truncation must be a contiguous float32 ({B},) tensor on the env's device")
                pr.truncation = truncation.data_ptr()
            _lib.check(self._L, self._L.vnl_env_reset_done_weighted(self._env_h, mk.data_ptr(), C.byref(nz), C.byref(pr), C.byref(p),
                                                                    arr, len(logs), self._stream()))
        self._hold = (mk, step_base, logs, record, priority, truncation)  # keep inputs alive until the stream has consumed them
        return state

    def step(self, state: State, action: torch.Tensor) -> State:
        """rodent.py:178-239.  action: (B, nu)."""
        nu, B = int(self.dims.nu), self.num_envs
        if tuple(action.shape) != (B, nu):
            raise ValueError(f"action must be ({B},{nu}), got {tuple(action.shape)}")
        a = action.to(device=self.device, dtype=self._dtype).contiguous()
        p = self._ptrs(state)
        ev = getattr(self, "kernel_events", None)  # (start, end) torch.cuda.Event pair, used by bench.py
        if ev is not None:
            ev[0].record()
        # one-shot hand-over from the fused unroll (acting._generate_unroll_fused): the rollout post-processing of this step
        # runs as the step kernel's epilogue (vnl_env_step_post) -- inside the launch the events time
        # (.. and, from acting.evaluate_unroll, the scoring of the step after it: vnl_env_step_post_eval)
        post, self._post_desc = getattr(self, "_post_desc", None), None
        score, self._eval_desc = getattr(self, "_eval_desc", None), None
        if post is not None and score is not None:
            _lib.check(self._L, self._L.vnl_env_step_post_eval(self._env_h, a.data_ptr(), C.byref(p), C.byref(post),
                                                               C.byref(score), self._stream()))
        elif post is not None:
            _lib.check(self._L, self._L.vnl_env_step_post(self._env_h, a.data_ptr(), C.byref(p), C.byref(post), self._stream()))
        else:
            _lib.check(self._L, self._L.vnl_env_step(self._env_h, a.data_ptr(), C.byref(p), self._stream()))
        if ev is not None:
            ev[1].record()
        self._hold = (a,)
        return state

    def forward_kinematics(self, qpos: torch.Tensor, out: Optional[State] = None) -> State:
        """`mjx.kinematics` of one qpos row per env (B, nq) on the device (vnl_env_fk): returns a State whose
        pipeline_state.xpos / xquat / subtree_com_root are filled and whose qpos carries the normalised root quaternion.
        Used by the device route of clip preprocessing (preprocessing/mjx_preprocess.py: process_qpos(..., fk=...))."""
        B, nq = self.num_envs, int(self.dims.nq)
        if tuple(qpos.shape) != (B, nq):
            raise ValueError(f"qpos must be ({B},{nq}), got {tuple(qpos.shape)}")
        state = out if out is not None else self._alloc_state()
        q = qpos.to(device=self.device, dtype=self._dtype).contiguous()
        state.pipeline_state.qpos.copy_(q)
        p = self._ptrs(state)
        _lib.check(self._L, self._L.vnl_env_fk(self._env_h, q.data_ptr(), C.byref(p), self._stream()))
        self._hold = (q,)
        return state

    # --- bisection hook -----------------------------------------------------------------------
    def debug(self, mode=True) -> None:
        """Bisection hooks.  mode 1 (True): every reset/step also dumps the per-env LDS image at the end of the
        kernel; mode 2: `step` dumps it as its LAST forward pass leaves it (before the Euler update reuses the
        constraint rows' space), `reset` at its end as before.  Either mode also records the solver's discrete
        decisions (`solver_trace()`).  0 / False: off."""
        stride = C.c_int32()
        _lib.check(self._L, self._L.vnl_env_debug(self._env_h, int(mode), C.byref(stride)))
        self._dump_stride = stride.value

    def solver_trace(self) -> torch.Tensor:
        """(B, n_frames, VNL_TRACE_INTS) int32: discrete decisions of the solver call of every substep of the last
        step (row 0 only after a reset); layout in csrc/vnl_types.h."""
        ptr, cnt = C.c_void_p(), C.c_int32()
        _lib.check(self._L, self._L.vnl_env_scratch(self._env_h, b"solver_trace", C.byref(ptr), C.byref(cnt)))
        B, n = self.num_envs, cnt.value
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            flat = torch.empty(B * n, dtype=torch.int32, device=self.device)
            rc = C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(flat.data_ptr()), ptr, C.c_size_t(4 * B * n), C.c_int(3))
            if rc != 0:
                raise _lib.VnlError(f"hipMemcpy failed: {rc}")
            flat = flat.cpu()
        else:
            flat = torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(B * n,)).copy())
        return flat.view(B, max(self._n_frames, 1), -1)

    def scratch(self, name: str) -> torch.Tensor:
        """(B, count) copy of a named per-env scratch section left by the last reset/step (debug on)."""
        ptr, cnt = C.c_void_p(), C.c_int32()
        _lib.check(self._L, self._L.vnl_env_scratch(self._env_h, name.encode(), C.byref(ptr), C.byref(cnt)))
        B, n, stride = self.num_envs, cnt.value, self._dump_stride
        esz = 8 if self._dtype == torch.float64 else 4
        total = (B - 1) * stride + n
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            flat = torch.empty(total, dtype=self._dtype, device=self.device)
            hip = C.CDLL("libamdhip64.so")
            rc = hip.hipMemcpy(C.c_void_p(flat.data_ptr()), ptr, C.c_size_t(esz * total), C.c_int(3))
            if rc != 0:
                raise _lib.VnlError(f"hipMemcpy failed: {rc}")
        else:
            ct = C.c_double if self._dtype == torch.float64 else C.c_float
            flat = torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(total,)).copy())
        return torch.as_strided(flat, (B, n), (stride, 1)).contiguous()


class RodentMultiClipTracking(RodentTracking):
    """Multi-clip variant.  The reference only has a stub (rodent.py:473-475); here the clip
    container carries a leading clip axis and each env tracks `info['clip_id']`."""
