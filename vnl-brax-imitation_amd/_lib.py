"""ctypes binding of the C-ABI in include/vnl.h (libvnl.so, built by csrc/build.py).

There is no CPU fallback: if the HIP library is missing, `load_library` raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libvnl.so")

i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)


class EnvSpec(C.Structure):
    _fields_ = [
        ("clip_frames", C.c_int32),
        ("num_clips", C.c_int32),
        ("ref_traj_length", C.c_int32),
        ("sub_clip_length", C.c_int32),
        ("n_frames", C.c_int32),
        ("num_track_bodies", C.c_int32),
        ("num_end_eff", C.c_int32),
        ("num_appendages", C.c_int32),
        ("num_joint_cols", C.c_int32),
        ("com_ref_col", C.c_int32),
        ("body_idxs", i32p),
        ("end_eff_idx", i32p),
        ("app_body", i32p),
        ("app_ref_col", i32p),
        ("joint_cols", i32p),
        ("healthy_z_lo", C.c_float),
        ("healthy_z_hi", C.c_float),
        ("termination_threshold", C.c_float),
        ("body_error_multiplier", C.c_float),
        ("position", f32p),
        ("quaternion", f32p),
        ("joints", f32p),
        ("body_positions", f32p),
        ("velocity", f32p),
        ("angular_velocity", f32p),
        ("joints_velocity", f32p),
        ("flags", C.c_int32),
        ("done_threshold", C.c_float),
        ("center_of_mass", f32p),
        ("reward_weights", C.c_float * 6),
    ]


ENV_REWARD_OLD_STATE, ENV_TERM_MEAN, ENV_NO_RAPP, ENV_OBS_QPOS_QVEL = 1, 2, 4, 8  # include/vnl.h VNL_ENV_*
ENV_WEIGHTS, ENV_RACT_ACTION, ENV_METRICS_UNSCALED, ENV_TRAJ_OLD_FRAME = 16, 32, 64, 128


STATE_FLOAT_FIELDS = ("qpos", "qvel", "act", "qacc_warmstart", "xpos", "xquat", "subtree_com1", "qfrc_actuator",
                      "obs", "reward", "done", "metrics", "traj", "termination_error")
STATE_INT_FIELDS = ("cur_frame", "sub_clip_frame", "clip_id")


class StatePtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STATE_FLOAT_FIELDS + STATE_INT_FIELDS]


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nq", "nv", "nu", "nbody", "njnt", "ngeom_collide", "ncon", "nefc",
                                          "obs_size", "traj_size", "workspace_floats_per_env", "workgroups_per_cu",
                                          "nbody_dynamic", "kernel_specialised", "factor_route")]


class PolicySpec(C.Structure):
    _fields_ = [
        ("traj_size", C.c_int32),
        ("obs_size", C.c_int32),
        ("action_size", C.c_int32),
        ("latent_size", C.c_int32),
        ("num_encoder_layers", C.c_int32),
        ("num_decoder_layers", C.c_int32),
        ("encoder_layers", C.c_int32 * 8),
        ("decoder_layers", C.c_int32 * 8),
    ]


class PolicyNoise(C.Structure):  # include/vnl.h: vnl_policy_noise
    _fields_ = [("seed", C.c_uint64), ("step_base", C.c_void_p), ("step_offset", C.c_int64), ("env_offset", C.c_int64),
                ("eps_latent_out", C.c_void_p), ("eps_action_out", C.c_void_p), ("rand_action_out", C.c_void_p)]


class ResetNoise(C.Structure):  # include/vnl.h: vnl_reset_noise
    _fields_ = [("seed", C.c_uint64), ("step_base", C.c_void_p), ("step_offset", C.c_int64), ("env_offset", C.c_int64),
                ("start_hi", C.c_int32), ("noise_scale", C.c_float),
                ("start_frame_out", C.c_void_p), ("clip_id_out", C.c_void_p), ("noise_out", C.c_void_p)]


RESET_MAX_LOGS = 8


class ResetLog(C.Structure):  # include/vnl.h: vnl_reset_log
    _fields_ = [("src", C.c_void_p), ("log", C.c_void_p), ("width", C.c_int32), ("pad_", C.c_int32)]


class StartPriorityDesc(C.Structure):  # include/vnl.h: vnl_start_priority
    _fields_ = [("cdf", C.c_void_p), ("ncell", C.c_int32), ("pad_", C.c_int32), ("ended", C.c_void_p), ("failed", C.c_void_p),
                ("truncation", C.c_void_p)]


PRIORITY_MAX_CELLS = 32768

POST_MAX_OPS = 24


class PostOp(C.Structure):  # include/vnl.h: vnl_post_op
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("first", C.c_void_p), ("log", C.c_void_p),
                ("width", C.c_int32), ("pad_", C.c_int32)]


class PostDesc(C.Structure):  # include/vnl.h: vnl_post_desc
    _fields_ = [(n, C.c_void_p) for n in ("steps", "prev_done", "done", "truncation", "reward", "log_reward",
                                          "log_discount", "log_truncation")] + \
               [("episode_length", C.c_int32), ("action_repeat", C.c_int32), ("num_ops", C.c_int32),
                ("pad_", C.c_int32), ("ops", PostOp * POST_MAX_OPS)]


EVAL_WIDTH = 12  # include/vnl.h: VNL_EVAL_WIDTH
EVAL_COLUMNS = ("start_frame", "clip_id", "steps", "truncation")  # then the seven metrics and the reward


class EvalDesc(C.Structure):  # include/vnl.h: vnl_eval_desc
    _fields_ = [(n, C.c_void_p) for n in ("done", "steps", "truncation", "reward", "metrics", "cur_frame", "sub_clip_frame",
                                          "clip_id", "run", "count", "records")] + \
               [("episodes_per_env", C.c_int32), ("pad_", C.c_int32)]


RECORD_MAX_COLS = 16  # include/vnl.h: VNL_RECORD_MAX_COLS


class RecordCol(C.Structure):  # include/vnl.h: vnl_record_col
    _fields_ = [("src", C.c_void_p), ("width", C.c_int32), ("pad_", C.c_int32)]


class RecordDesc(C.Structure):  # include/vnl.h: vnl_record_desc
    _fields_ = [(n, C.c_void_p) for n in ("env_index", "done", "ref_frame", "ref_clip", "count", "open", "rows")] + \
               [(n, C.c_int32) for n in ("num_rec", "capacity", "row_width", "stop_at_done", "num_cols", "pad_")] + \
               [("cols", RecordCol * RECORD_MAX_COLS)]


class GatherOp(C.Structure):  # include/vnl.h: vnl_gather_op
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("T", C.c_int32), ("width", C.c_int32)]


class GatherDesc(C.Structure):  # include/vnl.h: vnl_gather_desc
    _fields_ = [("idx", C.c_void_p), ("N", C.c_int32), ("M", C.c_int32), ("num_ops", C.c_int32), ("pad_", C.c_int32),
                ("ops", GatherOp * POST_MAX_OPS)]


class PPOHeadArgs(C.Structure):  # include/vnl.h: vnl_ppo_head_args
    _fields_ = [(n, C.c_int32) for n in ("T", "B", "act", "latent")] + \
               [(n, C.c_void_p) for n in ("logits", "baseline", "bootstrap", "lat_mean", "lat_logvar", "raw_action",
                                          "behaviour_log_prob", "reward", "truncation", "discount", "eps_entropy")] + \
               [(n, C.c_float) for n in ("entropy_cost", "discounting", "reward_scaling", "gae_lambda",
                                         "clipping_epsilon", "kl_weight", "min_std", "var_scale")] + \
               [("normalize_advantage", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("g_logits", "g_baseline", "g_lat_mean", "g_lat_logvar", "vs", "advantages",
                                          "metrics")]


PPO_HEAD_WORKSPACE_FLOATS = 4 + 4 * 256


class PPONetSpec(C.Structure):  # include/vnl.h: vnl_ppo_net_spec
    _fields_ = [(n, C.c_int32) for n in ("traj_size", "obs_size", "action_size", "latent_size", "num_encoder_layers",
                                          "num_decoder_layers", "num_value_layers")] + \
               [("encoder_layers", C.c_int32 * 8), ("decoder_layers", C.c_int32 * 8), ("value_layers", C.c_int32 * 8)]


class PPOBatch(C.Structure):  # include/vnl.h: vnl_ppo_batch
    _fields_ = [(n, C.c_void_p) for n in ("traj", "obs", "next_obs_last", "raw_action", "behaviour_log_prob", "reward",
                                          "truncation", "discount", "eps_latent", "eps_entropy", "obs_mean", "obs_std")]


class PPOHParams(C.Structure):  # include/vnl.h: vnl_ppo_hparams
    _fields_ = [(n, C.c_float) for n in ("entropy_cost", "discounting", "reward_scaling", "gae_lambda",
                                         "clipping_epsilon", "kl_weight", "min_std", "var_scale")] + \
               [("normalize_advantage", C.c_int32), ("pad_", C.c_int32)]

class CorrPlan(C.Structure):  # include/vnl.h: vnl_corr_plan
    _fields_ = [(n, C.c_int32) for n in ("route", "chunks", "chunk_cols", "row_tiles")] + [("workspace_floats", C.c_int64)]


class Domain(C.Structure):  # include/vnl.h: vnl_domain (float64 device pointers, [num_envs][n]; null = the model's value)
    _fields_ = [(n, C.c_void_p) for n in ("cg_friction", "act_gain", "dof_damping", "dof_armature")]

class DomainRanges(C.Structure):  # include/vnl.h: vnl_domain_ranges (float64 device pointers [n_f], fields in the order of vnl_domain)
    _fields_ = [("lo", C.c_void_p * 4), ("hi", C.c_void_p * 4), ("shared", C.c_uint32), ("pad_", C.c_uint32)]

BODY_RANGES_INERTIA_WITH_MASS = 1  # include/vnl.h: VNL_BODY_RANGES_INERTIA_WITH_MASS

class BodyDomainRanges(C.Structure):  # include/vnl.h: vnl_body_domain_ranges (float64 device pointers, fields in the order of vnl_body_domain)
    _fields_ = [("lo", C.c_void_p * 3), ("hi", C.c_void_p * 3), ("shared", C.c_uint32), ("flags", C.c_uint32)]

class BodyDomain(C.Structure):  # include/vnl.h: vnl_body_domain (float64 device pointers, [num_envs][nbody (x3)]; null = the model's value)
    _fields_ = [(n, C.c_void_p) for n in ("body_mass", "body_inertia", "body_ipos")]


EXPORTS = (
    "vnl_last_error", "vnl_version", "vnl_model_create", "vnl_model_destroy", "vnl_env_create", "vnl_env_destroy",
    "vnl_env_dims", "vnl_env_reset", "vnl_env_reset_done", "vnl_env_reset_done_weighted", "vnl_start_priority_update", "vnl_env_step", "vnl_env_step_post", "vnl_env_step_post_eval", "vnl_env_fk", "vnl_env_debug", "vnl_env_scratch", "vnl_policy_create", "vnl_policy_destroy",
    "vnl_policy_num_params", "vnl_policy_forward", "vnl_policy_forward_noise", "vnl_policy_decode", "vnl_policy_decode_noise", "vnl_rollout_post", "vnl_rollout_eval", "vnl_ppo_head", "vnl_adam_step", "vnl_gather_rows",
    "vnl_ppo_update_create", "vnl_ppo_update_destroy", "vnl_ppo_update_num_params", "vnl_ppo_update_buffer",
    "vnl_ppo_minibatch_grad",
    "vnl_ppo_minibatch_grad_part",
    "vnl_env_set_domain", "vnl_env_set_body_domain", "vnl_env_set_domain_ranges", "vnl_env_redraw_domain",
    "vnl_env_set_body_domain_ranges",
    "vnl_prediction_corr_plan", "vnl_prediction_corr",
    "vnl_env_record",
)
_HIP_ONLY = ("vnl_policy_", "vnl_ppo_update_", "vnl_ppo_minibatch_", "vnl_prediction_corr")  # not in the test-only host simulation


class VnlError(RuntimeError):
    pass


def _declare(lib: C.CDLL) -> C.CDLL:
    vp = C.c_void_p
    lib.vnl_last_error.restype = C.c_char_p
    lib.vnl_version.restype = C.c_int
    lib.vnl_model_create.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.vnl_model_destroy.argtypes = [vp]
    lib.vnl_model_destroy.restype = None
    lib.vnl_env_create.argtypes = [vp, C.POINTER(EnvSpec), C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.vnl_env_destroy.argtypes = [vp]
    lib.vnl_env_destroy.restype = None
    lib.vnl_env_dims.argtypes = [vp, C.POINTER(Dims)]
    lib.vnl_env_reset.argtypes = [vp, vp, vp, C.POINTER(StatePtrs), vp]
    lib.vnl_env_reset_done.argtypes = [vp, vp, C.POINTER(ResetNoise), C.POINTER(StatePtrs), C.POINTER(ResetLog), C.c_int32, vp]
    lib.vnl_env_reset_done_weighted.argtypes = [vp, vp, C.POINTER(ResetNoise), C.POINTER(StartPriorityDesc), C.POINTER(StatePtrs),
                                                C.POINTER(ResetLog), C.c_int32, vp]
    lib.vnl_start_priority_update.argtypes = [vp, vp, vp, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, vp]
    lib.vnl_env_step.argtypes = [vp, vp, C.POINTER(StatePtrs), vp]
    if hasattr(lib, "vnl_env_step_post"):
        lib.vnl_env_step_post.argtypes = [vp, vp, C.POINTER(StatePtrs), C.POINTER(PostDesc), vp]
    if hasattr(lib, "vnl_env_step_post_eval"):
        lib.vnl_env_step_post_eval.argtypes = [vp, vp, C.POINTER(StatePtrs), C.POINTER(PostDesc), C.POINTER(EvalDesc), vp]
        lib.vnl_rollout_eval.argtypes = [C.POINTER(EvalDesc), C.c_int32, vp]
    lib.vnl_env_record.argtypes = [vp, C.POINTER(RecordDesc), vp]
    lib.vnl_env_fk.argtypes = [vp, vp, C.POINTER(StatePtrs), vp]
    lib.vnl_env_debug.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.vnl_env_scratch.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int32)]
    lib.vnl_env_set_domain.argtypes = [vp, C.POINTER(Domain), vp]
    lib.vnl_env_set_body_domain.argtypes = [vp, C.POINTER(BodyDomain), vp]
    lib.vnl_env_set_domain_ranges.argtypes = [vp, C.POINTER(DomainRanges), vp]
    lib.vnl_env_redraw_domain.argtypes = [vp, vp, C.POINTER(ResetNoise), C.c_int32, vp]
    lib.vnl_env_set_body_domain_ranges.argtypes = [vp, C.POINTER(BodyDomainRanges), vp]
    lib.vnl_rollout_post.argtypes = [C.POINTER(PostDesc), C.c_int32, vp]
    lib.vnl_ppo_head.argtypes = [C.POINTER(PPOHeadArgs), vp, vp]
    lib.vnl_gather_rows.argtypes = [C.POINTER(GatherDesc), vp]
    lib.vnl_adam_step.argtypes = [vp, vp, vp, vp, vp, C.c_int64] + [C.c_double] * 4 + [vp]
    if hasattr(lib, "vnl_ppo_update_create"):
        lib.vnl_ppo_update_create.argtypes = [C.POINTER(PPONetSpec), C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
        lib.vnl_ppo_update_destroy.argtypes = [vp]
        lib.vnl_ppo_update_destroy.restype = None
        lib.vnl_ppo_update_num_params.argtypes = [vp]
        lib.vnl_ppo_update_num_params.restype = C.c_int64
        lib.vnl_ppo_update_buffer.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int64)]
        lib.vnl_ppo_minibatch_grad.argtypes = [vp, vp, C.POINTER(PPOBatch), C.POINTER(PPOHParams), vp, vp, vp]
        lib.vnl_ppo_minibatch_grad_part.argtypes = [vp, vp, C.POINTER(PPOBatch), C.POINTER(PPOHParams), vp, vp, vp, C.c_int]
        lib.vnl_prediction_corr_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CorrPlan)]
        lib.vnl_prediction_corr.argtypes = [vp, vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp]
    if hasattr(lib, "vnl_policy_create"):
        lib.vnl_policy_create.argtypes = [C.POINTER(PolicySpec), C.c_int32, C.c_int32, C.POINTER(vp)]
        lib.vnl_policy_destroy.argtypes = [vp]
        lib.vnl_policy_destroy.restype = None
        lib.vnl_policy_num_params.argtypes = [vp]
        lib.vnl_policy_num_params.restype = C.c_int64
        lib.vnl_policy_forward.argtypes = [vp] + [vp] * 7 + [C.c_int32, C.c_int32] + [vp] * 6 + [vp, vp] + [vp]
        lib.vnl_policy_forward_noise.argtypes = [vp] + [vp] * 5 + [C.POINTER(PolicyNoise), C.c_int32, C.c_int32] + [vp] * 7 + [vp]
        # (handle; params, obs_mean, obs_std, latent, obs, eps_action; batch, deterministic; action, raw_action, log_prob, logits;
        #  rand_action, rand_log_prob; stream)
        lib.vnl_policy_decode.argtypes = [vp] + [vp] * 6 + [C.c_int32, C.c_int32] + [vp] * 4 + [vp, vp] + [vp]
        # (handle; params, obs_mean, obs_std, latent or NULL, obs; noise; batch, deterministic; action, raw_action, log_prob,
        #  logits, rand_log_prob; stream)
        lib.vnl_policy_decode_noise.argtypes = [vp] + [vp] * 5 + [C.POINTER(PolicyNoise), C.c_int32, C.c_int32] + [vp] * 5 + [vp]
        if hasattr(lib, "vnl_policy_decode_threads_"):  # (the tile-shape knob of tools/decode_bench.py: not in include/vnl.h)
            lib.vnl_policy_decode_threads_.argtypes = [vp, C.c_int32]
    return lib


_cache = {}


def load_library(path: str | None = None, env_only: bool = False) -> C.CDLL:
    """Load libvnl.so.  Raises (loudly) if it has not been built.  `env_only` is for the test-only host
    simulation, which contains the env entry points but not the MFMA policy kernel."""
    path = os.path.abspath(path or os.environ.get("VNL_LIB", DEFAULT_LIB))
    if path not in _cache:
        if not os.path.exists(path):
            raise VnlError(
                f"HIP extension not found at {path}. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback for the rollout.")
        lib = C.CDLL(path)
        missing = [s for s in EXPORTS if not hasattr(lib, s) and not (env_only and s.startswith(_HIP_ONLY))]
        if missing:
            raise VnlError(f"{path} lacks symbols {missing}")
        _cache[path] = _declare(lib)
    return _cache[path]


def check(lib: C.CDLL, rc: int) -> None:
    if rc != 0:
        raise VnlError(f"vnl error {rc}: {lib.vnl_last_error().decode()}")
