// Recorded rollouts (include/vnl.h above vnl_record_desc: vnl_env_record): one row per recorder and call -- the reference
// pose of the env's clip, then the caller's columns -- written by a kernel and a launch of their own.  A translation unit of
// its own, like vnl_domain.hip and vnl_eval.hip and for their reason: every kernel a rollout or an evaluation launches is
// compiled exactly as without this feature.  The host simulation includes it from vnl_lib.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vnl.h"
#include "vnl_body.h"

// vnl_lib.hip (vnl_env is private to it): what this unit reads of an env, host side
void vnl_env_record_view_(const vnl_env* env, int* device, int* num_envs, int* nq, DevEnv* ev);
void vnl_set_error_(const char* msg);

// the env's side of a launch, by value: its device copy of the clip (csrc/vnl_types.h DevEnv) and the bounds of the indices
struct VnlRecordView {
  const float *position, *quaternion, *joints; /* (C,T,3), (C,T,4), (C,T,nq-7) */
  int num_envs, nq, T, C;
};

// One 64-lane wave per recorder; lane i owns word i of every 64-word trip over the row.  A row is a sequence of segments --
// the three clip tables of the reference pose, then the columns -- that start wherever the one before ended, so a trip may
// take its words from several: the row is flattened into (trip, segment) items, in each of which the lanes whose word lies in
// that segment load it.  The loads of VNL_RECORD_BATCH items are requested back to back before the first store (the value and
// its place in the row stay in registers; place -1 = nothing to store for this lane), then ONE explicit vector-memory wait,
// then the stores -- the form of vnl_post_epilogue (csrc/vnl_env_kernels.h; DESIGN, "No round trip per op"): left to the
// compiler the wait sits inside each store's own branch and covers the stores before it too.
// The cursor (segment, its first word in the row, the trip) is wave-uniform: count, open, the env index, the frame and the clip
// are read by every lane as one broadcast request each and made scalar, and the descriptor is a by-value kernel argument, so a
// segment's pointer and width are scalar loads from the kernel-argument segment when the cursor enters it.  Lane 0 stores
// count and open last, as plain vector stores; no atomics, no LDS.
#define VNL_RECORD_BATCH 16
#define VNL_RECORD_NAN 0x7FC00000u
#ifdef VNL_FORKJOIN_DEFINED /* the host simulation */
#define VNL_RECORD_LANDED(v)
#else
// (an asm statement takes at most 30 operands: the wait names the first eight values, the second statement pins the rest
// behind it)
#define VNL_RECORD_LANDED(v)                                                                                           \
  do {                                                                                                                 \
    asm volatile("s_waitcnt vmcnt(0)"                                                                                  \
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])      \
                 :                                                                                                     \
                 : "memory");                                                                                          \
    asm volatile(""                                                                                                    \
                 : "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])); \
  } while (0)
#endif
static_assert(VNL_RECORD_BATCH == 16, "VNL_RECORD_LANDED names sixteen values");

VNL_HD void vnl_record_wave(const vnl_record_desc& d, const VnlRecordView& cv, const unsigned r, const unsigned lane) {
  const int c = VNL_UNIFORM_I(d.count[r]), open = VNL_UNIFORM_I(d.open[r]);
  const int e = VNL_UNIFORM_I((d.env_index ? d.env_index : d.count)[r]);  // (absent: count is read in its place, not used)
  const int env = d.env_index ? e : (int)r;
  if (env < 0 || env >= cv.num_envs || open == 0 || c >= d.capacity) return;
  const bool ref = d.ref_frame != nullptr;
  // (absent rows read a present one in their place and are not used: the three requests go out together)
  int frame = VNL_UNIFORM_I((ref ? d.ref_frame : d.count)[ref ? env : (int)r]);
  int clip = VNL_UNIFORM_I((ref ? d.ref_clip : d.count)[ref ? env : (int)r]);
  const float done = d.done ? d.done[env] : 0.f;
  frame = frame < 0 ? 0 : (frame > cv.T - 1 ? cv.T - 1 : frame);
  clip = clip < 0 ? 0 : (clip > cv.C - 1 ? cv.C - 1 : clip);
  const size_t ct = (size_t)clip * cv.T + frame;
  unsigned* const row = (unsigned*)d.rows + ((size_t)r * d.capacity + c) * d.row_width;
  const int nref = ref ? 3 : 0, nseg = nref + d.num_cols;
  int k = 0, o = 0, tb = 0;  // the cursor: segment, its first word in the row, first word of the trip (wave-uniform)
  int width = 0;
  const unsigned* src = nullptr;
  bool enter = true;
  while (k < nseg) {
    unsigned v[VNL_RECORD_BATCH];
    int at[VNL_RECORD_BATCH];
#pragma unroll
    for (int j = 0; j < VNL_RECORD_BATCH; j++) {
      at[j] = -1;
      v[j] = VNL_RECORD_NAN;
      if (k < nseg) {
        if (enter) {
          if (k < nref) {
            width = k == 0 ? 3 : (k == 1 ? 4 : cv.nq - 7);
            src = (const unsigned*)(k == 0 ? cv.position : (k == 1 ? cv.quaternion : cv.joints)) + ct * width;
          } else {
            const void* s = d.cols[k - nref].src;
            width = d.cols[k - nref].width;
            src = s ? (const unsigned*)s + (size_t)env * width : nullptr;
          }
          enter = false;
        }
        const int w = tb + (int)lane, end = o + width;
        if (w >= o && w < end) {
          at[j] = w;
          if (src) v[j] = src[w - o];
        }
        if (end <= tb + VNL_LANES) {  // the segment ends in this trip: the next one goes on in it, unless the trip is full
          k++, o = end, enter = true;
          if (end == tb + VNL_LANES) tb += VNL_LANES;
        } else {
          tb += VNL_LANES;
        }
      }
    }
    VNL_RECORD_LANDED(v);
#pragma unroll
    for (int j = 0; j < VNL_RECORD_BATCH; j++)
      if (at[j] >= 0) row[at[j]] = v[j];
  }
  VNL_SERIAL {
    d.count[r] = c + 1;
    if (d.stop_at_done && d.done && done != 0.f) d.open[r] = 0;
  }
}

__global__ void __launch_bounds__(64) vnl_record_kernel(vnl_record_desc d, VnlRecordView cv) {
  vnl_record_wave(d, cv, blockIdx.x, threadIdx.x);
}

static int vnl_record_fail(const char* what) {
  char msg[256];
  snprintf(msg, sizeof(msg), "vnl_record_desc: %s", what);
  vnl_set_error_(msg);
  return VNL_ERR_ARG;
}

extern "C" int vnl_env_record(vnl_env* env, const vnl_record_desc* d, void* stream) {
  if (!env) {
    vnl_set_error_("vnl_env_record: env is null");
    return VNL_ERR_ARG;
  }
  if (!d) {
    vnl_set_error_("vnl_env_record: desc is null");
    return VNL_ERR_ARG;
  }
  if (!d->rows) return vnl_record_fail("rows is null");
  if (!d->count) return vnl_record_fail("count is null");
  if (!d->open) return vnl_record_fail("open is null");
  if (d->num_rec < 1) return vnl_record_fail("num_rec must be at least 1");
  if (d->capacity < 1) return vnl_record_fail("capacity must be at least 1");
  if (d->num_cols < 0 || d->num_cols > VNL_RECORD_MAX_COLS) return vnl_record_fail("num_cols must be 0..16");
  if (!d->ref_frame != !d->ref_clip) return vnl_record_fail("ref_frame and ref_clip go together (both or none)");
  int device = 0;
  DevEnv ev;
  VnlRecordView cv{};
  vnl_env_record_view_(env, &device, &cv.num_envs, &cv.nq, &ev);
  cv.position = ev.position, cv.quaternion = ev.quaternion, cv.joints = ev.joints, cv.T = ev.T, cv.C = ev.C;
  int64_t sum = d->ref_frame ? cv.nq : 0;
  for (int k = 0; k < d->num_cols; k++) {
    if (d->cols[k].width < 1) return vnl_record_fail("a column's width must be at least 1");
    sum += d->cols[k].width;
  }
  if (sum != (int64_t)d->row_width)
    return vnl_record_fail("row_width must be (nq with ref_frame / ref_clip, else 0) + the sum of the columns' widths");
  // the launch goes to the env's GPU whatever the caller's current device is, which is restored afterwards
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess || (prev != device && hipSetDevice(device) != hipSuccess)) {
    vnl_set_error_("vnl_env_record: hipSetDevice failed");
    return VNL_ERR_HIP;
  }
  hipLaunchKernelGGL(vnl_record_kernel, dim3(d->num_rec), dim3(64), 0, (hipStream_t)stream, *d, cv);
  const hipError_t err = hipGetLastError();
  if (prev != device) (void)hipSetDevice(prev);
  if (err != hipSuccess) {
    char msg[256];
    snprintf(msg, sizeof(msg), "vnl_env_record: launch: %s", hipGetErrorString(err));
    vnl_set_error_(msg);
    return VNL_ERR_HIP;
  }
  return VNL_OK;
}
