// The env kernels (one env per 64-lane workgroup) as templates over the compile-time model SP: instantiated for the shared
// model in vnl_lib.hip, for per-env parameter tables (VnlSpecDom) in vnl_domain.hip.
#pragma once
#include "../../include/vnl.h"
#include "vnl_body.h"

// (VNL_KERNEL_ATTR: empty in the product; csrc/build.py --spill sets a VGPR cap to force register spills to scratch,
// the regression build for the "results must not depend on spilling" test.  VNL_SPEC_ATTR: the specialised instantiations
// are held to the two waves per SIMD of the generic kernel -- with every bound a constant the compiler unrolls further and
// would take a 257th register, i.e. half the occupancy)
#ifndef VNL_KERNEL_ATTR
#define VNL_KERNEL_ATTR
#endif
#define VNL_ENV_KERNEL __launch_bounds__(64) VNL_KERNEL_ATTR

// The rollout post-processing of ONE env (include/vnl.h above vnl_post_desc: the same decisions and the same word copies as
// vnl_post_kernel of vnl_lib.hip) by the wave that has just stepped that env: the step kernel's epilogue (vnl_env_step_post).
// A finished wave's copies run under the physics of the other resident waves instead of in a launch of their own that can
// only start when the last step wave has ended.
// One wave must not pay a round trip per op: the ops are flattened into (op, trip of VNL_LANES words) items, and the loads of
// VNL_POST_BATCH items are requested back to back before the first of their stores (value and the two store addresses of a
// slot stay in registers; a null address = nothing to store for this lane).  The loads of a batch come before its stores:
// an op's `src` / `first` row must not be another op's `dst` / `log` row (dst == src of the SAME op is fine).
// The descriptor is a by-value kernel argument that only this function reads (scalar loads from the kernel-argument
// segment, an op's ten words when the cursor enters it).
#define VNL_POST_BATCH 16
#ifdef VNL_FORKJOIN_DEFINED /* the host simulation */
#define VNL_POST_LANDED(x)
#else
#define VNL_POST_LANDED(x) asm volatile("" : "+v"(x))
#endif
VNL_HD void vnl_post_epilogue(const vnl_post_desc& d, const unsigned e, const unsigned lane) {
  VNL_SYNC_GLOBAL();  // (done, reward, obs, the state and info rows: stored by other lanes of this wave)
  // every lane evaluates the decision itself from the OLD values, which must have returned before lane 0 stores the new ones;
  // the four loads are requested together (an absent row reads `done` in its place and is not used): one round trip, not four
  const float old_prev = (d.prev_done ? d.prev_done : d.done)[e], old_steps = (d.steps ? d.steps : d.done)[e];
  const float rew = (d.reward ? d.reward : d.done)[e];
  float done = d.done[e];
  float st = d.steps ? ((d.prev_done && old_prev != 0.f) ? 0.f : old_steps) + (float)d.action_repeat : 0.f;
  bool over = d.steps && st >= (float)d.episode_length;
  float trunc = over ? 1.f - done : 0.f;
  done = over ? 1.f : done;
  VNL_SYNC_GLOBAL();
  VNL_SERIAL {
    if (d.steps) d.steps[e] = st;
    if (d.prev_done) d.prev_done[e] = done;
    d.done[e] = done;
    if (d.truncation) d.truncation[e] = trunc;
    if (d.log_reward) d.log_reward[e] = rew;
    if (d.log_discount) d.log_discount[e] = 1.f - done;
    if (d.log_truncation) d.log_truncation[e] = trunc;
  }
  const bool reset = done != 0.f;
  const int n = d.num_ops;
  int k = 0, base = 0;  // the cursor: op, first word of its next trip (wave-uniform)
  const unsigned* src = nullptr;
  unsigned *dst = nullptr, *log = nullptr;
  int width = 0;
  while (k < n) {
    unsigned v[VNL_POST_BATCH];
    unsigned *pd[VNL_POST_BATCH], *pl[VNL_POST_BATCH];
#pragma unroll
    for (int j = 0; j < VNL_POST_BATCH; j++) {
      pd[j] = pl[j] = nullptr;
      v[j] = 0u;
      if (k < n) {
        if (base == 0) {  // (all ten words of the op are requested at once: selects, no branch between its fields)
          const float *o_src = d.ops[k].src, *o_first = d.ops[k].first;
          float *o_dst = d.ops[k].dst, *o_log = d.ops[k].log;
          width = d.ops[k].width;
          const bool from_first = o_first && reset;
          const size_t row = (size_t)e * width;
          src = (const unsigned*)(from_first ? o_first : o_src) + row;
          dst = (o_dst && (from_first || (const float*)o_dst != o_src)) ? (unsigned*)o_dst + row : nullptr;
          log = o_log ? (unsigned*)o_log + row : nullptr;
        }
        const int i = base + (int)lane;
        if (i < width) {
          v[j] = src[i];
          pd[j] = dst ? dst + i : nullptr;
          pl[j] = log ? log + i : nullptr;
        }
        base += VNL_LANES;
        if (base >= width) k++, base = 0;
      }
    }
    // (the whole batch has landed before its first store: one wait here, none between the stores -- a wait inside a
    // store's own branch would have to cover the stores before it as well, which share the loads' counter)
#pragma unroll
    for (int j = 0; j < VNL_POST_BATCH; j++) VNL_POST_LANDED(v[j]);
#pragma unroll
    for (int j = 0; j < VNL_POST_BATCH; j++) {
      if (pd[j]) *pd[j] = v[j];
      if (pl[j]) *pl[j] = v[j];
    }
  }
}

// The scoring of ONE env (include/vnl.h above vnl_eval_desc: the semantics of vnl_rollout_eval, whose kernel is this function
// per env) by the wave that has just stepped and post-processed it (vnl_env_step_post_eval).  Lane i owns word i of the
// record row: lanes 0..3 the header, lanes 4..11 the eight running sums.  Every load is requested before the first value is
// used (the uniform ones -- count, done, steps, truncation, the three frame words -- by every lane: one broadcast request
// each; an absent row reads a present one in its place and is not used), the stores are one vector store each for the run
// words, the record row and the count: no atomics, no loop over words.  A store follows a load of the same address only in
// the lane that loaded it and depends on the loaded value.
VNL_HD void vnl_eval_epilogue(const vnl_eval_desc& d, const unsigned e, const unsigned lane) {
  VNL_SYNC_GLOBAL();  // (done, steps, truncation and the frame rows: stored by other lanes of this wave)
  const int K = d.episodes_per_env;
  const int c = d.count[e];
  const float done = d.done[e], steps = d.steps[e], trunc = (d.truncation ? d.truncation : d.done)[e];
  const bool frames = d.cur_frame != nullptr;
  const int cur = (frames ? d.cur_frame : d.count)[e], sub = (frames ? d.sub_clip_frame : d.count)[e];
  const int clip = (frames ? d.clip_id : d.count)[e];
  VNL_FOR(i, VNL_EVAL_WIDTH) {
    const int k = i < 4 ? 0 : i - 4;  // (a header lane reads word 0 and does not use it)
    float* run = d.run + (size_t)e * 8 + k;
    const float x = *(k < 7 ? d.metrics + (size_t)e * 7 + k : d.reward + e), r0 = *run;
    if (c < K) {
      const float r = r0 + x;
      const float head = i == 0 ? (frames ? (float)(cur - sub) : -1.f)
                                : (i == 1 ? (frames ? (float)clip : -1.f) : (i == 2 ? steps : (d.truncation ? trunc : 0.f)));
      if (i >= 4) *run = done != 0.f ? 0.f : r;
      if (done != 0.f) d.records[((size_t)e * K + c) * VNL_EVAL_WIDTH + i] = i < 4 ? head : r;
    }
  }
  VNL_SERIAL {
    if (c < K && done != 0.f) d.count[e] = c + 1;
  }
}

// One env per 64-lane workgroup; the env's whole working set lives in dynamic LDS (~25 KB ->
// 6 workgroups per CU, 1536 envs in flight on 256 CUs).  `post`: the rollout post-processing of this env as the wave's
// epilogue (vnl_env_step_post), or num_ops < 0: none (vnl_env_step).
template <class SP>
__global__ void VNL_ENV_KERNEL vnl_step_kernel(const KernelConsts* kc, DevState st, const vreal* action,
                                                      vreal* dump, vreal* dump_mid, int* trace, vnl_post_desc post) {
  VNL_LDS_DECL(lds);
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  EnvWaveT<SP> w{k->m, k->ev, st, k->L, lds, blockIdx.x, threadIdx.x, k, nullptr};
  w.step(action, dump_mid, trace);
  if (dump) w.dump(dump);
  if (post.num_ops >= 0) vnl_post_epilogue(post, blockIdx.x, threadIdx.x);
}

// The step kernel of an EVALUATION (vnl_env_step_post_eval): the step, the post-processing and then the scoring of this env
// (vnl_eval_epilogue).  A kernel of its own, instantiated in a translation unit of its own (csrc/vnl_eval.hip), and not a
// second descriptor of vnl_step_kernel: with the descriptor as an argument the specialised training kernel took one more
// VGPR (242 for 241) although it never scores -- this way the kernels a rollout launches are compiled from the text they
// had before evaluations were scored on the device.
template <class SP>
__global__ void VNL_ENV_KERNEL vnl_step_eval_kernel(const KernelConsts* kc, DevState st, const vreal* action, vreal* dump,
                                                    vreal* dump_mid, int* trace, vnl_post_desc post, vnl_eval_desc ev) {
  VNL_LDS_DECL(lds);
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  EnvWaveT<SP> w{k->m, k->ev, st, k->L, lds, blockIdx.x, threadIdx.x, k, nullptr};
  w.step(action, dump_mid, trace);
  if (dump) w.dump(dump);
  vnl_post_epilogue(post, blockIdx.x, threadIdx.x);
  vnl_eval_epilogue(ev, blockIdx.x, threadIdx.x);
}

template <class SP>
__global__ void VNL_ENV_KERNEL vnl_reset_kernel(const KernelConsts* kc, DevState st, const int* start_frame,
                                                       const vreal* noise, vreal* dump, int* trace) {
  VNL_LDS_DECL(lds);
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  EnvWaveT<SP> w{k->m, k->ev, st, k->L, lds, blockIdx.x, threadIdx.x, k, nullptr};
  w.reset(start_frame, noise, trace);
  if (dump) w.dump(dump);
}


// A fresh episode for the envs whose mask is set (EnvWaveT::reset_fresh), then up to VNL_RESET_MAX_LOGS row copies for EVERY
// env (32-bit words, as vnl_rollout_post moves rows: next_observation[t] and the logged state extras record the post-reset
// values without a launch of their own).  An env that does not reset reads its mask word and goes straight to the copies:
// no tables, no LDS.
template <class SP>
__global__ void VNL_ENV_KERNEL vnl_reset_done_kernel(const KernelConsts* kc, DevState st, ResetDoneArgs a, vreal* dump, int* trace) {
  VNL_LDS_DECL(lds);
  const unsigned e = blockIdx.x, lane = threadIdx.x;
  if (a.mask[e] != 0.f) {
    const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
    EnvWaveT<SP> w{k->m, k->ev, st, k->L, lds, e, lane, k, nullptr};
    w.reset_fresh(a, trace);
    if (dump) w.dump(dump);
    VNL_SYNC_GLOBAL();  // (the copies below read rows that other lanes stored)
  }
  for (int q = 0; q < a.num_logs; q++) {
    const unsigned* src = a.logs[q].src + (size_t)e * a.logs[q].width;
    unsigned* log = a.logs[q].log + (size_t)e * a.logs[q].width;
    VNL_FOR(i, a.logs[q].width) log[i] = src[i];
  }
}

// The domain redraw of EnvWaveT::reset_fresh as a launch of its own (vnl_env_redraw_domain: the first episode's domain, and
// what the tests compare the fused redraw with): the envs whose mask is set, or every env with a null mask; the four-field
// ranges, the body ranges (EnvWaveT::redraw_body_domain), or both, as the env has them.  Randomised instantiations only; no
// LDS, no state.
template <class SP>
__global__ void __launch_bounds__(64) vnl_redraw_domain_kernel(const KernelConsts* kc, const float* mask, const int64_t* step_base,
                                                               int64_t step_offset, uint32_t key0, uint32_t key1, uint32_t env0,
                                                               int initial) {
  const unsigned e = blockIdx.x, lane = threadIdx.x;
  if (mask && mask[e] == 0.f) return;
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  const DevState none{};
  EnvWaveT<SP> w{k->m, k->ev, none, k->L, nullptr, e, lane, k, nullptr};
  const int64_t step = *step_base + step_offset;
  const uint32_t c2 = (uint32_t)step, c3 = ((uint32_t)(step >> 32) << 2) | 3u;
  const int on = k->rng.on;  // (whichever of the two range sets the env has)
  if (on & VNL_RANGES_FOUR) w.redraw_domain(key0, key1, env0 + e, c2, c3, initial);
  if (on & VNL_RANGES_BODY) w.redraw_body_domain(key0, key1, env0 + e, c2, c3, initial);
}
