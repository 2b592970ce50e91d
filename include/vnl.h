/*
 * vnl.h -- C-ABI of the MI355X-native rodent-imitation rollout.
 *
 * The reference (talmolab/VNL-Brax-Imitation) is pure Python on JAX/MJX/Brax and
 * has no FFI of its own; this ABI is the boundary a maintainer binds (ctypes, see
 * INTEGRATION.md) to replace, for the hot path only:
 *
 *   vnl_env_reset  <->  RodentTracking.reset          reference envs/rodent.py:119-176
 *                       (+ brax PipelineEnv.pipeline_init = mjx.forward, rodent.py:148)
 *   vnl_env_step   <->  RodentTracking.step           reference envs/rodent.py:178-239
 *                       (+ PipelineEnv.pipeline_step = n_frames x mjx.step, rodent.py:181)
 *   vnl_policy_*   <->  make_inference_fn(...).policy reference ppo_imitation/ppo_networks.py:45-83
 *                       IntentionNetwork.__call__     reference ppo_imitation/intention_policy_network.py:91-105
 *   vnl_rollout_post <-> brax Episode/AutoReset wrappers (train.py:204-214) + Transition of actor_step (acting.py:34-57)
 *   vnl_env_step_post <-> vnl_env_step and vnl_rollout_post in ONE launch: each step wave post-processes its own env
 *   vnl_gather_rows / vnl_ppo_head / vnl_adam_step
 *                  <->  the minibatch gather, loss head (intention_losses.py:26-87,131-202) and optimiser update of one
 *                       PPO minibatch step (ppo_imitation/train.py:231-291)
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every state / observation / action buffer is CALLER-OWNED device memory,
 *     float32 (int32 for frame counters), row-major [env][feature] (what a
 *     torch (B, n) tensor is).  One 64-lane wavefront owns one env, so lane i
 *     touches element env*n + i: contiguous per wave, and obs/traj come out in
 *     the layout the policy GEMMs consume;
 *   - the library owns model constants, the clip copy and per-env scratch,
 *     released by vnl_env_destroy / vnl_model_destroy;
 *   - all work is enqueued asynchronously on the caller's HIP stream (passed as
 *     void* = hipStream_t); no hidden synchronisation; a handle is not
 *     thread-safe (one handle per GPU / process);
 *   - return 0 on success, negative error code otherwise; message through
 *     vnl_last_error() (thread-local).  Nothing throws across the ABI.
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     fails with VNL_ERR_NO_DEVICE.
 */
#ifndef VNL_H_
#define VNL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNL_OK 0
#define VNL_ERR_ARG -1
#define VNL_ERR_BLOB -2
#define VNL_ERR_HIP -3
#define VNL_ERR_NO_DEVICE -4
#define VNL_ERR_UNSUPPORTED -5

typedef struct vnl_model vnl_model;
typedef struct vnl_env vnl_env;
typedef struct vnl_policy vnl_policy;

/* Environment description: mirrors the constructor state of RodentTracking
 * (reference envs/rodent.py:17-117).  Index arrays are the EFFECTIVE indices
 * after the reference's (buggy) use of MuJoCo ids on filtered clip axes and
 * JAX's clamp-on-gather semantics; the Python
 * mirror derives them from names exactly as the reference does. */
typedef struct vnl_envspec {
  int32_t clip_frames;     /* T: frames per clip */
  int32_t num_clips;       /* C: clips resident (1 for the single-clip env) */
  int32_t ref_traj_length; /* rodent.py:34 */
  int32_t sub_clip_length; /* rodent.py:33 */
  int32_t n_frames;        /* physics substeps per control step, rodent.py:97-99 */
  int32_t num_track_bodies;/* width of the filtered clip.body_positions, rodent.py:113-115 */
  int32_t num_end_eff;
  int32_t num_appendages;
  int32_t num_joint_cols;
  int32_t com_ref_col;
  const int32_t* body_idxs;   /* [num_track_bodies] model body ids, rodent.py:80-85 */
  const int32_t* end_eff_idx; /* [num_end_eff] model body ids, rodent.py:65-70 */
  const int32_t* app_body;    /* [num_appendages] model body ids, rodent.py:71-76,307 */
  const int32_t* app_ref_col; /* [num_appendages] clamped columns of the filtered clip axis */
  const int32_t* joint_cols;  /* [num_joint_cols] clamped columns of the (nq-7)-wide joint axis */
  float healthy_z_lo, healthy_z_hi; /* rodent.py:31 */
  float termination_threshold;      /* rodent.py:35 */
  float body_error_multiplier;      /* rodent.py:36 */
  /* clip tensors, HOST pointers, float32, row-major (C, T, n); copied at create.
   * Fields of ReferenceClip, reference preprocessing/mjx_preprocess.py:21-40. */
  const float* position;         /* (C,T,3) */
  const float* quaternion;       /* (C,T,4) */
  const float* joints;           /* (C,T,nq-7) */
  const float* body_positions;   /* (C,T,num_track_bodies,3), already filtered */
  const float* velocity;         /* (C,T,3) */
  const float* angular_velocity; /* (C,T,3) */
  const float* joints_velocity;  /* (C,T,nq-7) */
  /* Which tracking env's glue.  0 = RodentTracking (envs/rodent.py:178-316).  HumanoidTracking (envs/humanoid.py:185-311)
   * = VNL_ENV_REWARD_OLD_STATE | VNL_ENV_TERM_MEAN | VNL_ENV_NO_RAPP | VNL_ENV_OBS_QPOS_QVEL with done_threshold 0.5. */
  int32_t flags;
  float done_threshold;          /* done when the UNSCALED rtrunk is below it: 0 (rodent.py:213), 0.5 (humanoid.py:199) */
  const float* center_of_mass;   /* (C,T,3) reference for rcom (humanoid.py:273), or NULL: body_positions[com_ref_col] (rodent.py:279) */
  /* with VNL_ENV_WEIGHTS: weights of rcom, rvel, rtrunk, rquat, ract, rapp in the total reward (ant.py:182-188:
   * 0.05, 0.01, 0.20, 0.01, 0.001, -); without it 0.01, 0.01, 0.01, 0.01, 0.0001, 0.01 (rodent.py:203-209) */
  float reward_weights[6];
} vnl_envspec;
#define VNL_ENV_REWARD_OLD_STATE 1 /* reward terms from the state BEFORE the step (humanoid.py:195: _calculate_reward(state, ..)) */
#define VNL_ENV_TERM_MEAN 2        /* termination error = means of |.| (humanoid.py:256-260), not the matrix-1 / L1 norms */
#define VNL_ENV_NO_RAPP 4          /* no appendage reward term */
#define VNL_ENV_OBS_QPOS_QVEL 8    /* observation = [qpos, qvel] only (humanoid.py:354-368) */
/* AntTracking (envs/ant.py:172-291) = the four above | the four below, done_threshold 0 */
#define VNL_ENV_WEIGHTS 16         /* reward_weights[] replace the built-in weights */
#define VNL_ENV_RACT_ACTION 32     /* ract = 0.01 * -0.015 * sum(action^2) / nu (ant.py:277), not the actuator forces */
#define VNL_ENV_METRICS_UNSCALED 64 /* metrics / termination_error hold the UNWEIGHTED terms (ant.py:197,216-225) */
#define VNL_ENV_TRAJ_OLD_FRAME 128 /* the step's reference slice starts at the OLD cur_frame + 1: ant.py:178 builds the
                                    * observation from the un-incremented info */

/* Caller-owned device buffers, row-major [num_envs][count]. */
typedef struct vnl_state {
  /* brax State.pipeline_state (mjx.Data) -- carried */
  float* qpos;           /* [nq] */
  float* qvel;           /* [nv] */
  float* act;            /* [nu] */
  float* qacc_warmstart; /* [nv] */
  /* derived by the last mjx.forward (lag qpos by one substep) */
  float* xpos;           /* [3*nbody] */
  float* xquat;          /* [4*nbody] */
  float* subtree_com1;   /* [3]  = data.subtree_com[1] */
  float* qfrc_actuator;  /* [nv] */
  /* brax State.{obs,reward,done,metrics} */
  float* obs;     /* [obs_size]  */
  float* reward;  /* [1] */
  float* done;    /* [1] */
  float* metrics; /* [7]: rcom rvel rtrunk rquat ract rapp termination_error */
  /* brax State.info */
  float* traj;              /* [traj_size] */
  float* termination_error; /* [1] */
  int32_t* cur_frame;       /* [1] */
  int32_t* sub_clip_frame;  /* [1] */
  int32_t* clip_id;         /* [1] which resident clip this env tracks (0 for single clip) */
} vnl_state;

/* Model dimensions, for sizing caller buffers. */
typedef struct vnl_dims {
  int32_t nq, nv, nu, nbody, njnt, ngeom_collide, ncon, nefc, obs_size, traj_size;
  int32_t workspace_floats_per_env; /* per-env LDS working set, in floats */
  int32_t workgroups_per_cu;        /* occupancy of the step kernel as reported by the HIP runtime */
  int32_t nbody_dynamic;            /* bodies the dynamics works on: the model's welded (jointless) bodies are folded into their
                                       parents; every one of the nbody bodies still has its row of xpos / xquat */
  int32_t kernel_specialised;       /* 1: the env runs the kernels specialised at compile time for its dimensions (the reference's
                                       rodent); 0: the generic kernels */
  int32_t factor_route;             /* the routes of the factorisations, chosen for the model at env creation: a nibble each,
                                       bits 0..3 qM's factor, 4..7 its inverse, 8..11 the Newton Hessian's factor (0: CG), in
                                       each 1 LDS-resident, 2 / 3 rows in registers (max depth < 16 / 36), 4 rows in registers
                                       over two lane sets (nv <= 128); bits 12..15: 0, or the lane sets (1, 2) of the
                                       articulated-body form that makes both factors of a substep at once (eulerdamp) */
} vnl_dims;

const char* vnl_last_error(void);
int vnl_version(void);

/* model: blob produced by vnl_brax_imitation_amd.model.blob.to_blob (host memory) */
int vnl_model_create(const void* blob, size_t nbytes, vnl_model** out);
void vnl_model_destroy(vnl_model*);

/* env: device = HIP ordinal (>= 0) */
int vnl_env_create(const vnl_model*, const vnl_envspec*, int32_t num_envs, int32_t device, vnl_env** out);
void vnl_env_destroy(vnl_env*);
int vnl_env_dims(const vnl_env*, vnl_dims* out);

/* reset: start_frame [num_envs] int32, clip_id written by caller into state->clip_id,
 * noise [num_envs][nq] (already scaled by reset_noise_scale; rodent.py:131-147). */
int vnl_env_reset(vnl_env*, const int32_t* start_frame, const float* noise, const vnl_state* state, void* stream);

/* A fresh episode for the envs whose mask word is nonzero, drawn INSIDE the kernel (the opt-in alternative to the auto-reset
 * wrapper's cached first state): a new start frame, clip and reset noise per env and episode, from stream 3 of the
 * counter layout of vnl_policy_noise below (streams 0..2 are the acting kernel's; the stream field is the low two bits of
 * counter word 3, so 3 is the last one):
 *   key     = (seed low 32 bits, seed high 32 bits)
 *   counter = (block, env_offset + e, step low 32 bits, (step >> 32) << 2 | 3),   step = *step_base + step_offset
 *   blocks 0 .. (nq + 3) / 4 - 1: the reset noise, Box-Muller as for the policy's normals, times noise_scale; element j of the
 *                                 row is output j % 4 of block j / 4
 *   block 0x80000000            : start_frame = (x0 * start_hi) >> 32, clip_id = (x1 * num_clips) >> 32 (64-bit products; a
 *                                 value's probability is off 1 / n by less than 2^-32)
 * An env's draws depend on (seed, step, env_offset + e) alone: not on the mask, the batch size or the sharding.
 * ppo_imitation/philox.py (reset_draws) restates them in torch ops.  The draws are stored -- into the record rows below, or
 * into scratch of the library's when a record pointer is null -- and the reset body of vnl_env_reset runs on the stored rows:
 * vnl_env_reset given the recorded start_frame, clip_id and noise returns the same bits.
 * Written for a reset env: the pipeline state (qpos .. qfrc_actuator), obs, traj, termination_error, cur_frame,
 * sub_clip_frame (0) and clip_id.  NOT written: reward, done and metrics, which keep the terminal step's values as under
 * brax's auto-reset.  Nothing of an env whose mask is 0 is touched; per-env domain tables stay as they are unless ranges are set
 * (vnl_env_set_domain_ranges below: then the domain of every reset env is drawn anew first).
 * Then, for EVERY env, each of the `num_logs` (0..8) log descriptors copies row src[e][width] to log[e][width] (32-bit
 * words, as vnl_rollout_post moves rows): next_observation and the logged info fields of a rollout record the post-reset
 * values without a launch of their own.
 * The kernel only READS the step counter; the caller advances it in stream order (see vnl_policy_noise).  VNL_ERR_ARG, with
 * nothing launched, for a null mask / descriptor / state / step_base, start_hi < 1, a negative offset, env_offset +
 * num_envs >= 2^32 - 1, or num_logs outside 0..8.  With vnl_env_debug on, the image and trace row 0 of reset envs are written. */
typedef struct vnl_reset_noise {
  uint64_t seed;
  const int64_t* step_base; /* device, [1], read only */
  int64_t step_offset;      /* host value, >= 0 */
  int64_t env_offset;       /* global index of env 0, >= 0 */
  int32_t start_hi;         /* start_frame uniform in [0, start_hi) */
  float noise_scale;        /* rodent.py:31 reset_noise_scale */
  int32_t* start_frame_out; /* optional records, [num_envs] / [num_envs] / [num_envs][nq] (the env's real type, as the noise of */
  int32_t* clip_id_out;     /* vnl_env_reset): only the rows of reset envs are written */
  float* noise_out;
} vnl_reset_noise;
typedef struct vnl_reset_log {
  const float* src;
  float* log;
  int32_t width, pad_;
} vnl_reset_log;
int vnl_env_reset_done(vnl_env*, const float* mask /* [num_envs] float32 */, const vnl_reset_noise*, const vnl_state*,
                       const vnl_reset_log* logs, int32_t num_logs, void* stream);

/* Prioritised start frames (opt-in): vnl_env_reset_done with the start frame and clip drawn from a TABLE and the episodes
 * that end counted, so that a training loop can start more often where episodes fail.  A cell is clip * start_hi +
 * start_frame; ncell = num_clips * start_hi, at most 32768 (frames are not binned into coarser cells).
 * A null descriptor: vnl_env_reset_done exactly (which IS this entry called with a null descriptor).
 * Counting -- for an env whose mask is set, BEFORE anything of it is overwritten: sf0 = cur_frame - sub_clip_frame is the
 *   finished episode's start frame, c0 = clip_id its clip.  If 0 <= sf0 < start_hi, 0 <= c0 < num_clips and truncation is
 *   null or truncation[e] == 0: ended[c0 * start_hi + sf0] += 1, and failed[..] += 1 if also sub_clip_frame <
 *   sub_clip_length (it ended before its sub-clip did).  Anything out of range is skipped, never indexed.  Integer atomic
 *   adds: the counts do not depend on the order.  Unmasked envs count nothing; with `ended` and `failed` null nothing is
 *   counted.
 * Draw -- word x0 of block 0x80000000 of stream 3 (the block of the uniform draws; x1 is unused):
 *   cell = #{ c < ncell - 1 : cdf[c] <= x0 }, start_frame = cell % start_hi, clip_id = cell / start_hi.
 *   cdf is nondecreasing; cell c owns the words [cdf[c - 1], cdf[c]) (cdf[-1] = 0), the last cell the rest: entry
 *   ncell - 1 is never read, and a cell of width 0 is never drawn.  The noise blocks are untouched: a weighted reset has
 *   the noise bits of the uniform one.  The rest is the reset of vnl_env_reset_done on the stored draws.
 *   ppo_imitation/philox.py (weighted_cells) restates the draw in torch ops.
 * Beyond vnl_env_reset_done's checks, with nothing launched: VNL_ERR_ARG for a null cdf, ncell != num_clips * start_hi, or
 * exactly one of ended / failed null; VNL_ERR_UNSUPPORTED for ncell > 32768. */
typedef struct vnl_start_priority {
  const uint32_t* cdf;      /* device [ncell], ncell = num_clips * start_hi */
  int32_t ncell, pad_;
  uint32_t *ended, *failed; /* device [ncell] each, or both null: no counting */
  const float* truncation;  /* device [num_envs] or null */
} vnl_start_priority;
int vnl_env_reset_done_weighted(vnl_env*, const float* mask, const vnl_reset_noise*, const vnl_start_priority*,
                                const vnl_state*, const vnl_reset_log*, int32_t num_logs, void* stream);

/* Counters -> table, in one launch of one workgroup, all in integers (exact, independent of any order).  With a = prior:
 *   n = min(ended[c], 2^20), f = min(failed[c], n)
 *   s = ((f + a) << 16) / (n + 2 a)      64-bit; the smoothed failure rate in Q16, at most 65535
 *   t = s + floor_q16                    the uniform floor: a cell that never fails keeps weight
 *   P_c = t_0 + .. + t_c (64-bit), S = P_{ncell-1} < 2^32
 *   cdf[c] = (P_c << 32) / S for c < ncell - 1, cdf[ncell - 1] = 0xFFFFFFFF
 * then ended[c] >>= decay_shift, failed[c] >>= decay_shift (0 keeps accumulating).  Every cell's width is at least 1: no
 * cell becomes unreachable.  Zero counters give the uniform table cdf[c] = ((c + 1) << 32) / ncell.
 * ppo_imitation/philox.py (start_priority_table) restates it.  VNL_ERR_ARG, with nothing launched, for a null pointer,
 * ncell < 1, prior < 1, floor_q16 outside 1..65536 or decay_shift outside 0..31; VNL_ERR_UNSUPPORTED for ncell > 32768. */
int vnl_start_priority_update(uint32_t* ended, uint32_t* failed, uint32_t* cdf, int32_t ncell, uint32_t prior,
                              uint32_t floor_q16, int32_t decay_shift, void* stream);

/* step: action [num_envs][nu]; state updated in place. */
int vnl_env_step(vnl_env*, const float* action, const vnl_state* state, void* stream);
/* Forward kinematics only (reference preprocessing/mjx_preprocess.py:85-107: `mjx.kinematics` scanned over the frames of a
 * clip): env e takes row e of qpos [num_envs][nq] and fills state->xpos, xquat, subtree_com1 and the
 * normalised root quaternion in state->qpos[e][3..7); nothing else of the state is touched. */
int vnl_env_fk(vnl_env* env, const float* qpos, const vnl_state* state, void* stream);

/* Domain randomisation (brax `randomization_fn`, MJX semantics): per-env values of four raw model fields, fixed until the
 * next call (auto-reset leaves them as they are, unless vnl_env_set_domain_ranges has set ranges).  Device pointers, float64, row-major [num_envs][n]; a null field pointer
 * means the model's value for every env:
 *   cg_friction  [ncg]  sliding friction of each collidable geom's contact rows (column 0 of the compiled cg_friction)
 *   act_gain     [nu]   gainprm[0]
 *   dof_damping  [nv], dof_armature [nv]
 * Derived constants (dof / body invweight0, meaninertia, scale) stay as compiled; the contact rows' mu and inverse weight are
 * derived per env by the upload's float64 expression, so a domain equal to the compiled values gives bit-identical tables.
 * Every value must be finite, friction > 0, damping and armature >= 0 (else VNL_ERR_ARG).  The call waits for `stream`,
 * copies and derives into library-owned tables; reset / step then run the randomised kernels.  A null `vnl_domain*` clears
 * the domain (and the ranges of vnl_env_set_domain_ranges).  vnl_env_scratch reads the tables back: "dom_mu", "dom_invw" [num_envs][ncg], "dom_gain" [num_envs][nu],
 * "dom_damp", "dom_arm" [num_envs][nv] (row stride = the returned count, vreal elements; no debug mode needed). */
typedef struct vnl_domain {
  const double *cg_friction, *act_gain, *dof_damping, *dof_armature;
} vnl_domain;
int vnl_env_set_domain(vnl_env* env, const vnl_domain* domain, void* stream);

/* A new domain per EPISODE (opt-in): per-element bounds of the four fields of vnl_domain, stored with the env.  With ranges
 * set, vnl_env_reset_done / vnl_env_reset_done_weighted draw the domain of every env they reset anew, inside the reset
 * kernel: after the start-priority counting (which reads the finished episode), before the noise and integer draws and the
 * reset body -- the forward pass of the reset, and qacc_warmstart with it, belong to the new domain.  Without ranges every
 * path is what it is without this entry, bit for bit.
 * The draw, from a third block range of stream 3 of vnl_reset_noise (beside the noise blocks 0.. and the integer block
 * 0x80000000), for field f (0 cg_friction, 1 act_gain, 2 dof_damping, 3 dof_armature) and element j:
 *   counter = (0x40000000 + initial * 0x20000000 + f * 0x00100000 + j / 4, env_offset + e, step low 32 bits,
 *              (step >> 32) << 2 | 3), word j % 4 of the block; a SHARED field (bit f of `shared`): word 0 of block j / 4 = 0 for
 *              every element -- one uniform per (env, episode) for the whole field
 *   u = (x + 0.5) * 2^-32                 float64, exact, strictly inside (0, 1)
 *   v = lo[j] + u * (hi[j] - lo[j])       float64; the difference, the product and the sum each rounded on its own (no fused
 *                                         multiply-add), so lo == hi gives exactly lo
 *   tables: dom_gain / dom_damp / dom_arm / dom_mu = (real)v; dom_invw = (real) of the upload's float64 expression
 *           (t + v^2 t) 2 v^2 / impratio, t = cg_t[j] -- the bits vnl_env_set_domain produces from the same float64 values.
 * An env's draw depends on (seed, step, env_offset + e, initial) alone.  ppo_imitation/philox.py (domain_draws) restates it.
 * vnl_env_set_domain_ranges follows the contract of vnl_env_set_domain: it waits for `stream`, copies the bounds (and cg_t,
 * impratio: what the derivation needs, as float64) into library-owned device memory, and validates on the host first --
 * VNL_ERR_ARG with the field's name, nothing launched and nothing changed, unless every value is finite, lo <= hi, friction
 * lo > 0, damping and armature lo >= 0, and lo[f] / hi[f] are both given or both null.  An env without a four-field domain
 * gets its tables at the compiled values and runs the randomised kernels from then on; an env with vnl_env_set_domain
 * values keeps them until its first redraw.  A later vnl_env_set_domain overwrites the tables, not the ranges;
 * vnl_env_set_domain(null) also clears the ranges.  The body tables (vnl_env_set_body_domain) are redrawn only
 * under ranges of their own (vnl_env_set_body_domain_ranges below).
 * vnl_env_redraw_domain is the same device function as a launch of its own -- the domain of the FIRST episode
 * (initial = 1: a block range of its own, so that it differs from a reset at the same counter) and the tests' handle on the
 * draw: seed, step_base, step_offset and env_offset of the descriptor are read; a null mask = every env.  VNL_ERR_ARG
 * without ranges, for a null descriptor / step_base, a negative offset, or initial outside 0..1. */
typedef struct vnl_domain_ranges {
  /* fields in the order of vnl_domain: cg_friction [ncg], act_gain [nu], dof_damping [nv], dof_armature [nv].
     DEVICE float64 [n_f] each: ABSOLUTE bounds per element.  lo[f] and hi[f] both null: field f is never redrawn. */
  const double* lo[4];
  const double* hi[4];
  uint32_t shared; /* bit f set: ONE uniform per (env, episode) for the whole field f; clear: one per element */
  uint32_t pad_;
} vnl_domain_ranges;
int vnl_env_set_domain_ranges(vnl_env*, const vnl_domain_ranges*, void* stream); /* null descriptor clears */
int vnl_env_redraw_domain(vnl_env*, const float* mask /* [num_envs] or null = every env */,
                          const vnl_reset_noise* /* seed, step_base, step_offset, env_offset are read */,
                          int32_t initial, void* stream);

/* Domain randomisation of the inertial fields: per-env body mass, principal moments and centre of mass over the bodies of
 * the model AS GIVEN (nbody of vnl_dims: welded bodies included), float64 DEVICE pointers, row-major
 *   body_mass [num_envs][nbody], body_inertia [num_envs][nbody][3] (in the frame of the compiled body_iquat, which is not
 *   randomisable), body_ipos [num_envs][nbody][3];
 * a null member leaves every env the compiled values; row 0 (the world body) is not read.  What the upload derives from the
 * three fields is derived per env by the upload's own float64 code: the welded bodies folded into their parents (mass,
 * centre of mass, full inertia of every dynamic body), the packed inertia and 1 / total mass; body / dof invweight0,
 * meaninertia and body_subtreemass stay as compiled (MJX semantics).  An env's full inertia is the compiled one plus
 * R(iquat) diag(body_inertia - compiled body_inertia) R(iquat)', so compiled values give bit-identical tables.
 * Every value must be finite, masses and moments >= 0; after the fold every dynamic body that carries dofs must have
 * mass > 0 and a positive diagonal of its inertia, and the total mass must be > 0 (else VNL_ERR_ARG with the field's name).
 * Same contract as vnl_env_set_domain (waits for `stream`, copies and derives; null clears this part), and the two calls
 * compose in either order: the part that is unset reads as the compiled values.  The model must carry body_inertia and
 * body_iquat (VNL_ERR_BLOB otherwise).  vnl_env_scratch: "dom_mass" [num_envs][nd], "dom_ipos" [num_envs][3 nd],
 * "dom_inertia6" [num_envs][6 nd] (xx yy zz xy xz yz), "dom_tminv" [num_envs][1], nd = nbody_dynamic. */
typedef struct vnl_body_domain {
  const double *body_mass, *body_inertia, *body_ipos;
} vnl_body_domain;
int vnl_env_set_body_domain(vnl_env* env, const vnl_body_domain* domain, void* stream);

/* A new BODY domain per episode (opt-in): per-element bounds of the three fields of vnl_body_domain, stored with the env.  With
 * ranges set, vnl_env_reset_done / vnl_env_reset_done_weighted draw mass, moments and centre of mass of every env they reset
 * anew inside the reset kernel -- at the place of the four-field redraw (vnl_domain_ranges above) and after it, before the noise
 * and integer draws and the reset body -- and derive the four body tables on the device by the fold the host runs
 * (csrc/vnl_inertial.h: float64, no fused multiply-add): the bits vnl_env_set_body_domain produces from the same float64 values.
 * The draw continues the block range of vnl_domain_ranges with the field indices f = 4 body_mass, 5 body_inertia, 6 body_ipos;
 * element j of the flattened field ([nbody], [nbody][3], [nbody][3]):
 *   counter = (0x40000000 + initial * 0x20000000 + f * 0x00100000 + j / 4, env_offset + e, step low 32 bits,
 *              (step >> 32) << 2 | 3), word j % 4; a SHARED field: word 0 of block j / 4 = 0 for every element
 *   v = lo[j] + u * (hi[j] - lo[j]), u = (x + 0.5) * 2^-32   exactly as for vnl_domain_ranges
 * With VNL_BODY_RANGES_INERTIA_WITH_MASS moment (b, k) takes the word of body b's MASS draw (the shared mass word if the mass
 * field is shared): the triangle inequality of the moments is not checked, and bounds for mass and moments that are the same
 * multiples of the compiled values then scale a body like a change of density -- a body that was physical stays physical.
 * Without the flag the moments are drawn independently.  Row 0 (the world body) is never drawn.  A field without bounds keeps,
 * per env, the values vnl_env_set_body_domain gave it (else the compiled ones).  ppo_imitation/philox.py (body_domain_draws)
 * restates the draw.
 * The contract of vnl_env_set_domain_ranges: the call waits for `stream`, validates on the host first (VNL_ERR_ARG with the
 * field's name, nothing launched and nothing changed) and copies the bounds and what the fold needs into one library-owned
 * device buffer; VNL_ERR_BLOB for body_inertia bounds on a model without body_inertia / body_iquat.  Valid: every value finite,
 * lo <= hi, mass and moment lo >= 0, lo[f] / hi[f] both given or both null, the flag only with mass bounds -- and, because the
 * kernel does not validate, a sufficient condition for every draw to pass vnl_env_set_body_domain's own checks: at the LOWER
 * bounds every dynamic body that carries dofs has a member mass sum > 0 and a member whose three moments are > 0, and the total
 * mass is > 0.  (Masses only grow from their lower bounds, so every fused mass and the total stay > 0.  The fused inertia about
 * the fused centre of mass is the sum over the members of R I R' plus a parallel-axis term m (|d|^2 1 - d d'), each positive
 * semi-definite; I of the member with three positive moments is R(iquat) diag(moments) R(iquat)' up to the rounding of the
 * compiled full inertia, positive definite -- so the sum is, and its diagonal is positive.)
 * An env without a body domain gets its body tables at the compiled values and runs the randomised kernels from then on.  A
 * later vnl_env_set_body_domain overwrites tables, not ranges; vnl_env_set_body_domain(null) clears its part AND these ranges;
 * vnl_env_set_domain(null) clears the four-field ranges only.  vnl_env_redraw_domain draws whichever of the two range sets the
 * env has, and fails with "no ranges" only when it has neither. */
#define VNL_BODY_RANGES_INERTIA_WITH_MASS 1u
typedef struct vnl_body_domain_ranges {
  /* fields in the order of vnl_body_domain: body_mass [nbody], body_inertia [nbody][3], body_ipos [nbody][3] over the
     bodies AS GIVEN; DEVICE float64, ABSOLUTE bounds per element; lo[f] and hi[f] both null: field f is never redrawn.
     Row 0 (the world body) is never drawn: it keeps the compiled values, as under vnl_env_set_body_domain. */
  const double* lo[3];
  const double* hi[3];
  uint32_t shared; /* bit f: ONE uniform per (env, episode) for the whole field f */
  uint32_t flags;  /* VNL_BODY_RANGES_INERTIA_WITH_MASS: moment (b, k) takes the uniform of body b's MASS draw */
} vnl_body_domain_ranges;
int vnl_env_set_body_domain_ranges(vnl_env*, const vnl_body_domain_ranges*, void* stream); /* null clears */

/* Bisection hooks.  The per-env working set lives in LDS; with debug on, every reset/step
 * also copies it to a device dump [num_envs][row_stride]: enable = 1 at the end of the kernel,
 * enable = 2 (step only) as the LAST forward pass of the step leaves it, i.e. before the Euler
 * update reuses the space of the constraint rows; 0 = off.  vnl_env_scratch returns the device
 * pointer of a named section inside row 0 ("qLD", "qfrc_smooth", "qacc_smooth", "qacc",
 * "efc_D", "Jaref", "qfrc_constraint", ...) and its element count; env e is at +e*row_stride.
 * The section "solver_trace" is separate from the image: int32 [num_envs][n_frames][536], the
 * discrete decisions (warm start, iteration counts, line-search bracket decisions, active-row
 * counts) of the solver call of every substep, layout in csrc/vnl_types.h (VNL_TRACE_*).
 * One section is a MODEL table, not per env, and needs no debug mode: "fac_match", the factorisation schedule as the
 * kernels load it -- uint32 [nv][count] (dev_ptr is that table, to be read as 32-bit words; count = words per ROW), byte
 * s & 3 of word s >> 2 of row a = the scratch lines row a absorbs in step s, rows padded with zero bytes to whole words. */
int vnl_env_debug(vnl_env*, int32_t enable, int32_t* row_stride);
int vnl_env_scratch(const vnl_env*, const char* name, float** dev_ptr, int32_t* count);

/* ---- policy forward (intention network), ppo_networks.py:45-83 ----------------
 * params: flat float32 device buffer in the order documented in INTEGRATION.md.
 * Inputs traj/obs row-major as produced by vnl_env_step; normaliser mean/std [obs_size].
 * eps_latent [B][latent] and eps_action [B][act] are caller-supplied N(0,1) draws
 * (the JAX threefry stream is not reproduced).  Outputs row-major. */
typedef struct vnl_policy_spec {
  int32_t traj_size, obs_size, action_size, latent_size;
  int32_t num_encoder_layers, num_decoder_layers;
  int32_t encoder_layers[8], decoder_layers[8];
} vnl_policy_spec;

int vnl_policy_create(const vnl_policy_spec*, int32_t max_batch, int32_t device, vnl_policy** out);
void vnl_policy_destroy(vnl_policy*);
int64_t vnl_policy_num_params(const vnl_policy*);
int vnl_policy_forward(vnl_policy*, const float* params, const float* obs_mean, const float* obs_std,
                       const float* traj, const float* obs, const float* eps_latent, const float* eps_action,
                       int32_t batch, int32_t deterministic, float* action, float* raw_action, float* log_prob,
                       float* logits, float* latent_mean, float* latent_logvar,
                       const float* rand_action /* [act] pre-tanh action or NULL */,
                       float* rand_log_prob /* [batch] its log-prob under every env's distribution
                                               (the reference's policy extras, ppo_networks.py:67-73), or NULL */,
                       void* stream);

/* The same forward pass with the noise drawn INSIDE the kernel, from counter-based streams keyed by
 * (seed, step, global env index): an env's draws do not depend on the batch size or on its row, so a run sharded over
 * several devices (env_offset = rank * num_envs) reproduces the unsharded one.  Generator: Philox4x32-10 (Salmon et al.
 * 2011; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with
 *   key     = (seed low 32 bits, seed high 32 bits)
 *   counter = (block, env, step low 32 bits, (step >> 32) << 2 | stream),   step = *step_base + step_offset < 2^62,
 *   stream  = 0 eps_latent, 1 eps_action, 2 the random action shared by the batch (env word 0xFFFFFFFF),
 *   env     = env_offset + row.
 * A call yields four words x0..x3, u_i = ((x_i >> 8) + 0.5) 2^-24; normals by Box-Muller, (u0, u1) -> sqrt(-2 ln u0)
 * (cos, sin)(2 pi u1) and (u2, u3) likewise; element j of a row is output j % 4 of block j / 4; stream 2 gives 2 u - 1.
 * ppo_imitation/philox.py restates it in torch ops (the tests' reference).  Everything after the draw is the arithmetic of
 * vnl_policy_forward: fed the recorded draws, that entry point returns the same bits.
 * The kernel only READS the step counter (the workgroups of a launch are not ordered against each other): the caller
 * advances it, in stream order, after the calls that share it -- a captured unroll of T steps bakes step_offset = 0..T-1
 * into its launches and adds T to *step_base once. */
typedef struct vnl_policy_noise {
  uint64_t seed;
  const int64_t* step_base;   /* device, [1], read only: step = *step_base + step_offset */
  int64_t step_offset;        /* host value, >= 0 */
  int64_t env_offset;         /* global index of row 0, >= 0; env_offset + batch < 2^32 - 1 */
  float *eps_latent_out, *eps_action_out, *rand_action_out; /* optional records of the draws used: [batch][latent],
                                                              * [batch][act], [act]; the last two stochastic mode only */
} vnl_policy_noise;
/* deterministic: stream 0 only.  rand_log_prob NULL: stream 2 is not drawn.  VNL_ERR_ARG (nothing launched) for a null
 * step_base, a negative offset or an env index that would reach 2^32 - 1. */
int vnl_policy_forward_noise(vnl_policy*, const float* params, const float* obs_mean, const float* obs_std,
                             const float* traj, const float* obs, const vnl_policy_noise*, int32_t batch,
                             int32_t deterministic, float* action, float* raw_action, float* log_prob, float* logits,
                             float* latent_mean, float* latent_logvar, float* rand_log_prob /* or NULL */, void* stream);

/* Latent-driven acting: the DECODER alone, [z | normalised obs] -> [Dense -> ReLU -> LayerNorm] x (n-1) -> Dense -> the
 * tanh-Normal tail of vnl_policy_forward, on the same handle, flat parameter buffer and vnl_policy_spec; only the decoder's
 * parameters are read (the encoder's and the two latent heads' are not).  latent is [batch][latent].  Fed
 * z = latent_mean + eps_latent * exp(latent_logvar / 2) of a vnl_policy_forward call, it returns that call's outputs up to
 * the rounding of z.
 * vnl_policy_decode: z, eps_action and rand_action are the caller's; a null latent is VNL_ERR_ARG.
 * vnl_policy_decode_noise: the streams, counters and step of vnl_policy_noise above, keyed by (seed, step, env_offset + row):
 *   stream 1  eps_action, stream 2 the random action shared by the batch -- the draws vnl_policy_forward_noise makes;
 *   stream 0  with latent == NULL, z ITSELF is the normal draw, z ~ N(0, I): the prior of the KL term, on the counters the
 *             acting kernel uses for eps_latent; recorded through eps_latent_out when that is given.  With latent given,
 *             stream 0 is not drawn and eps_latent_out is left alone.
 * deterministic: streams 1 and 2 are not drawn.  The kernel only READS the step counter.  VNL_ERR_ARG (nothing launched)
 * for obs_mean / obs_std given one without the other, batch outside 1..max_batch, a null step_base, a negative offset or an
 * env index that would reach 2^32 - 1. */
int vnl_policy_decode(vnl_policy*, const float* params, const float* obs_mean, const float* obs_std,
                      const float* latent, const float* obs, const float* eps_action, int32_t batch,
                      int32_t deterministic, float* action, float* raw_action, float* log_prob, float* logits,
                      const float* rand_action /* or NULL */, float* rand_log_prob /* or NULL */, void* stream);
int vnl_policy_decode_noise(vnl_policy*, const float* params, const float* obs_mean, const float* obs_std,
                            const float* latent /* NULL: z drawn, stream 0 */, const float* obs,
                            const vnl_policy_noise*, int32_t batch, int32_t deterministic, float* action,
                            float* raw_action, float* log_prob, float* logits, float* rand_log_prob /* or NULL */,
                            void* stream);

/* ---- rollout post-processing: the training wrappers and the Transition logging in ONE launch ----
 * brax EpisodeWrapper + AutoResetWrapper as applied by the reference's wrap_for_training
 * (ppo_imitation/train.py:204-214) and the per-step Transition of actor_step
 * (ppo_imitation/acting.py:34-57).  Per env e, in this order:
 *   steps = (prev_done ? 0 : steps) + action_repeat;  over = steps >= episode_length
 *   truncation = over ? 1 - done : 0;  done = over ? 1 : done;  prev_done = done
 *   log_reward = reward;  log_discount = 1 - done;  log_truncation = truncation   (each optional)
 *   every op:  v = (first && done) ? first[e] : src[e];  dst[e] = v (if dst);  log[e] = v (if log)
 * All arrays are row-major [num_envs][width] device buffers of 32-bit words (float32; int32 frame
 * counters are moved bit-exactly).  dst may alias src. */
#define VNL_POST_MAX_OPS 24
typedef struct vnl_post_op {
  float* dst;
  const float* src;
  const float* first;
  float* log;
  int32_t width;
  int32_t pad_;
} vnl_post_op;
typedef struct vnl_post_desc {
  float *steps, *prev_done, *done, *truncation;
  const float* reward;
  float *log_reward, *log_discount, *log_truncation;
  int32_t episode_length, action_repeat, num_ops, pad_;
  vnl_post_op ops[VNL_POST_MAX_OPS];
} vnl_post_desc;
int vnl_rollout_post(const vnl_post_desc*, int32_t num_envs, void* stream);
/* vnl_env_step followed by vnl_rollout_post(desc, num_envs = the env's own), as ONE launch: the wave that has stepped env e
 * runs the post-processing of env e as its epilogue, while the other resident waves are still in their physics -- no launch
 * that waits for the last step wave, none that the next policy launch waits for.  Same per-env semantics and order as
 * above, the same words in every buffer; the descriptor is validated as by vnl_rollout_post (same codes, same messages)
 * and copied into the launch's arguments (capturable in a hipGraph; it need not outlive the call).  The rows of an op move
 * in batches -- the loads of several ops before their stores -- so an op's src / first row must not be ANOTHER op's dst
 * or log row (dst == src of one op is fine).  For envs with a domain the randomised kernels take the same entry. */
int vnl_env_step_post(vnl_env*, const float* action, const vnl_state* state, const vnl_post_desc* desc, void* stream);

/* ---- evaluation: scored episodes, one record per episode ----
 * Each env scores its first K = episodes_per_env episodes and is ignored afterwards (K = 1: brax's EvalWrapper).  Per env e,
 * after the wrapper decision above has produced the final done, steps and truncation:
 *   c = count[e];  if c >= K: nothing of env e is written
 *   run[e][k] += metrics[e][k] (k = 0..6);  run[e][7] += reward[e]            float32 adds, in step order
 *   if done[e] != 0:
 *     records[e][c] = { cur_frame - sub_clip_frame, clip_id, steps[e], truncation[e] (0 if null), run[e][0..8) }
 *     run[e][:] = 0;  count[e] = c + 1
 * A record is VNL_EVAL_WIDTH float32 words.  Start frame and clip are what the start-priority counting of
 * vnl_env_reset_done_weighted reads, as they stand after the post-processing (i.e. before a fresh reset); with null frame
 * pointers (all three or none) columns 0 and 1 hold -1.  The caller zeroes run and count; record rows at or beyond count[e]
 * are never written.  run, count and records must not be rows of a post op.
 * VNL_ERR_ARG (nothing launched, the field named) for a null desc, done, steps, reward, metrics, run, count or records, for
 * episodes_per_env < 1 and for frame pointers partly null. */
#define VNL_EVAL_WIDTH 12
typedef struct vnl_eval_desc {
  const float *done, *steps, *truncation /* or NULL */, *reward, *metrics /* [num_envs][7] */;
  const int32_t *cur_frame, *sub_clip_frame, *clip_id; /* all three or none */
  float* run;      /* [num_envs][8] */
  int32_t* count;  /* [num_envs] */
  float* records;  /* [num_envs][episodes_per_env][VNL_EVAL_WIDTH] */
  int32_t episodes_per_env, pad_;
} vnl_eval_desc;
/* a launch of its own: for envs whose step is more than the kernel launch, after vnl_rollout_post */
int vnl_rollout_eval(const vnl_eval_desc*, int32_t num_envs, void* stream);
/* vnl_env_step, vnl_rollout_post(desc) and vnl_rollout_eval(eval) in ONE launch: the wave that has stepped env e runs the
 * post-processing and then the scoring of env e; the same words in every buffer as the three launches in that order.  Both
 * descriptors are validated as by their own entries and copied into the launch's arguments. */
int vnl_env_step_post_eval(vnl_env*, const float* action, const vnl_state* state, const vnl_post_desc* desc,
                           const vnl_eval_desc* eval, void* stream);

/* ---- recorded rollouts: per-step traces of chosen envs, one row per call ----
 * What the reference's policy_params_fn keeps of an episode it watches (train.py:154-331: qpos, termination_error, reward, the
 * logits, log_prob, rand_log_prob per step, and [reference qpos | rollout qpos] for the renderer, train.py:289-291), written on
 * the device by a launch of its own after the step (and after vnl_rollout_post / vnl_rollout_eval, before a fresh reset).
 * Per recorder r, with e = env_index ? env_index[r] : r:
 *   nothing is written if e is outside [0, num_envs), if open[r] == 0, or if c = count[r] >= capacity
 *   rows[r][c] = { reference pose | col 0 | col 1 | .. }
 *     reference pose (only with ref_frame / ref_clip): nq words -- position, quaternion and joints of clip ref_clip[e] at frame
 *       clamp(ref_frame[e], 0, T - 1), from the env's own device copy of the clip (a clip index outside [0, num_clips) is
 *       clamped likewise: never indexed)
 *     col k: `width` 32-bit words of src[e] (row e of [num_envs][width]), moved bit-exactly: float32, int32, NaN payloads;
 *       a column whose src is NULL is `width` words 0x7FC00000 (a quiet NaN: row 0, the reset state, has no policy outputs)
 *   count[r] = c + 1
 *   if stop_at_done and done is given and done[e] != 0: open[r] = 0
 * Rows at or beyond count[r] are never touched; two recorders may watch the same env.  The caller sets count = 0 and
 * open = 1.  rows, count and open must not be a column's source.  The descriptor is copied into the launch's arguments
 * (capturable in a hipGraph: the cursor lives on the device, so replays advance it; it need not outlive the call).
 * VNL_ERR_ARG (nothing launched, the field named) for a null env, desc, rows, count or open, num_rec < 1, capacity < 1,
 * num_cols outside 0..VNL_RECORD_MAX_COLS, a width < 1, ref_frame given without ref_clip or the other way round, and
 * row_width != (ref ? nq : 0) + the sum of the widths. */
#define VNL_RECORD_MAX_COLS 16
typedef struct vnl_record_col {
  const void* src;
  int32_t width, pad_;
} vnl_record_col;
typedef struct vnl_record_desc {
  const int32_t* env_index;            /* device [num_rec], or NULL: recorder r watches env r */
  const float* done;                   /* [num_envs] the wrapper's done, or NULL */
  const int32_t *ref_frame, *ref_clip; /* [num_envs], both or none: the row starts with the clip's pose */
  int32_t *count, *open;               /* [num_rec]; the caller sets count = 0 and open = 1 */
  float* rows;                         /* [num_rec][capacity][row_width] */
  int32_t num_rec, capacity, row_width, stop_at_done, num_cols, pad_;
  vnl_record_col cols[VNL_RECORD_MAX_COLS];
} vnl_record_desc;
int vnl_env_record(vnl_env*, const vnl_record_desc*, void* stream);

/* ---- PPO loss head: everything of compute_ppo_intention_loss after the network forward passes ----
 * (reference ppo_imitation/intention_losses.py:26-87 compute_gae, :131-202 loss) in three small launches: GAE,
 * advantage normalisation, tanh-Normal log-prob and entropy, clipped surrogate, value loss, latent KL,
 * their sum, AND the gradients of that sum w.r.t. the four network outputs.  Arrays are time-major
 * [T][B] (index t*B + b) float32 device buffers; logits [T*B][2*act], latents [T*B][latent]. */
typedef struct vnl_ppo_head_args {
  int32_t T, B, act, latent;
  const float *logits, *baseline, *bootstrap, *lat_mean, *lat_logvar;       /* network outputs */
  const float *raw_action, *behaviour_log_prob, *reward, *truncation, *discount, *eps_entropy;
  float entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon, kl_weight, min_std, var_scale;
  int32_t normalize_advantage, pad_;
  float *g_logits, *g_baseline, *g_lat_mean, *g_lat_logvar; /* d total_loss / d (network outputs) */
  float *vs, *advantages;                                   /* [T*B] GAE outputs (advantages before normalisation) */
  float *metrics; /* [8]: total_loss, policy_loss, v_loss, entropy_loss, kl_loss_intention, explained_variance,
                   * advantage mean, advantage std (before normalisation) */
} vnl_ppo_head_args;
/* workspace: 4 + 4 * 256 floats of device memory (statistics and per-block partial sums) */
#define VNL_PPO_HEAD_WORKSPACE_FLOATS (4 + 4 * 256)
int vnl_ppo_head(const vnl_ppo_head_args*, float* workspace, void* stream);

/* ---- minibatch gather: dst_k[t][j][:] = src_k[t][idx[j]][:] for every array k of a time-major Transition
 * (the index_select of brax's sgd_step, reference ppo_imitation/train.py:270-291), one launch for all arrays.
 * src_k is [T_k][N][width_k], dst_k [T_k][M][width_k], 32-bit words; idx [M] int64 on the device. */
typedef struct vnl_gather_op {
  float* dst;
  const float* src;
  int32_t T, width;
} vnl_gather_op;
typedef struct vnl_gather_desc {
  const int64_t* idx;
  int32_t N, M, num_ops, pad_;
  vnl_gather_op ops[VNL_POST_MAX_OPS];
} vnl_gather_desc;
int vnl_gather_rows(const vnl_gather_desc*, void* stream);

/* ---- Adam on one flat buffer (optax.adam as the reference builds it, ppo_imitation/train.py:231-233:
 * b1 0.9, b2 0.999, eps 1e-8, no weight decay): mu, nu, params updated in place in ONE launch.
 * `count` is the device-resident step number AFTER this step (the caller increments it first), so that
 * the launch can sit inside a captured hipGraph. */
int vnl_adam_step(float* params, const float* grads, float* mu, float* nu, const int64_t* count, int64_t n,
                  double lr, double b1, double b2, double eps, void* stream); /* hyper-parameters as the Python doubles they are:
                  1 - b2 is formed in double before the cast to float32, as optax does */

/* ---- PPO minibatch step, forward AND backward: the gradient of compute_ppo_intention_loss (reference
 * ppo_imitation/intention_losses.py:91-202) w.r.t. the policy and value parameters, i.e. what jax.grad computes inside
 * brax's gradient_update_fn for ppo_imitation/train.py:255-268.  Networks: the intention policy
 * (intention_policy_network.py:20-105; encoder / decoder of Dense -> ReLU -> LayerNorm, heads fc2_mean / fc2_logvar,
 * z = mean + eps exp(logvar / 2), decoder on [z | normalised obs], last decoder layer linear) and the value MLP
 * (ppo_networks.py:114-118, swish, scalar output).  `params` / `grads`: flat float32 [policy | value] in the layout of
 * INTEGRATION.md (Flax tensor order); grads is overwritten.  Minibatch arrays are time-major (index t*B + b).
 * Everything is enqueued on `stream`; no host synchronisation (capturable in a hipGraph). */
typedef struct vnl_ppo_net_spec {
  int32_t traj_size, obs_size, action_size, latent_size;
  int32_t num_encoder_layers, num_decoder_layers /* incl. the output layer of 2*action_size */, num_value_layers /* hidden */;
  int32_t encoder_layers[8], decoder_layers[8], value_layers[8];
} vnl_ppo_net_spec;
typedef struct vnl_ppo_batch {
  const float *traj;          /* [T*B][traj_size]   Transition.extras.state_extras.traj */
  const float *obs;           /* [T*B][obs_size]    Transition.observation (raw, not normalised) */
  const float *next_obs_last; /* [B][obs_size]      Transition.next_observation[-1] (bootstrap) */
  const float *raw_action, *behaviour_log_prob, *reward, *truncation, *discount;
  const float *eps_latent;    /* [T*B][latent]  N(0,1) draws of the reparameterisation */
  const float *eps_entropy;   /* [T*B][act]     N(0,1) draws of the entropy estimate */
  const float *obs_mean, *obs_std; /* [obs_size] running-statistics normaliser, or both NULL (identity) */
} vnl_ppo_batch;
typedef struct vnl_ppo_hparams {
  float entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon, kl_weight, min_std, var_scale;
  int32_t normalize_advantage, pad_;
} vnl_ppo_hparams;
typedef struct vnl_ppo_update vnl_ppo_update;
int vnl_ppo_update_create(const vnl_ppo_net_spec*, int32_t T, int32_t B, int32_t device, vnl_ppo_update** out);
void vnl_ppo_update_destroy(vnl_ppo_update*);
int64_t vnl_ppo_update_num_params(const vnl_ppo_update*);
/* device pointer of an intermediate of the LAST vnl_ppo_minibatch_grad call (valid until the next one; read it on the same
 * stream): "vs", "advantages" [T*B], "values" [T*B + B] (baseline then bootstrap), "logits" [T*B][2 act],
 * "latent_mean", "latent_logvar" [T*B][latent] */
int vnl_ppo_update_buffer(const vnl_ppo_update*, const char* name, float** dev_ptr, int64_t* count);
/* metrics [9]: [0..8) as vnl_ppo_head, [8] prediction_corr -- the mean of corrcoef([vs ; reward * reward_scaling]) over
 * its (2T)^2 entries (reference intention_losses.py:186-188), computed at every minibatch size (vnl_prediction_corr below,
 * route_request 0) */
int vnl_ppo_minibatch_grad(vnl_ppo_update*, const float* params, const vnl_ppo_batch*, const vnl_ppo_hparams*, float* grads,
                           float* metrics, void* stream);
/* The same step in two parts, for data-parallel training (reference ppo_imitation/train.py:251-268 averages the gradient over the
 * devices once per minibatch step): part 1 = forward of both networks + loss head + the VALUE network's backward -- in stream
 * order the value segment grads[policy_params .. num_params) is then final; part 2 = the policy network's backward (same
 * arguments, after part 1): the policy segment.  The caller all-reduces the value segment between the two, so that the
 * exchange overlaps part 2.  part 0 = the whole step (== vnl_ppo_minibatch_grad). */
int vnl_ppo_minibatch_grad_part(vnl_ppo_update*, const float* params, const vnl_ppo_batch*, const vnl_ppo_hparams*, float* grads,
                                float* metrics, void* stream, int part);

/* ---- prediction_corr on its own: the mean over the (2T)^2 entries of corrcoef([vs ; reward * reward_scaling]), two-pass
 * like jnp.corrcoef (row means, then the Gram matrix of the centred rows; entries clamped to [-1, 1], a NaN passed through).
 * `vs`, `reward`: time-major [T][B] float32 device buffers; `out`: one float on the device.  Route 1 is one workgroup with all
 * 2T rows in LDS ((2 T B + 2 T) * 4 <= 61440 bytes); route 2 splits B over `chunks` workgroups per pair of 64-row tiles
 * (`chunk_cols` columns each, partial Gram matrices in `workspace`, summed in ascending chunk order: no atomics, the same
 * bits on every call).  Everything is enqueued on `stream`; no host synchronisation, no allocation (capturable).
 * route_request: 0 = what vnl_ppo_minibatch_grad takes, 1 / 2 = force (1 -> VNL_ERR_ARG when the rows do not fit).
 * `workspace` needs vnl_corr_plan.workspace_floats floats (0 for route 1: it may then be NULL). */
typedef struct vnl_corr_plan {
  int32_t route; /* 1 one workgroup, 2 tiled */
  int32_t chunks, chunk_cols, row_tiles; /* route 2 (0 for route 1) */
  int64_t workspace_floats;
} vnl_corr_plan;
int vnl_prediction_corr_plan(int32_t T, int32_t B, int32_t route_request, vnl_corr_plan* out); /* needs no device */
int vnl_prediction_corr(const float* vs, const float* reward, float reward_scaling, int32_t T, int32_t B, int32_t route_request,
                        float* workspace, int64_t workspace_floats, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNL_H_ */
