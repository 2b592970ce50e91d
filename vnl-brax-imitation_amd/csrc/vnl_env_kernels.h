// The env kernels (one env per 64-lane workgroup) as templates over the compile-time model SP: instantiated for the shared
// model in vnl_lib.hip, for per-env parameter tables (VnlSpecDom) in vnl_domain.hip.
#pragma once
#include "vnl_body.h"

// (VNL_KERNEL_ATTR: empty in the product; csrc/build.py --spill sets a VGPR cap to force register spills to scratch,
// the regression build for the "results must not depend on spilling" test.  VNL_SPEC_ATTR: the specialised instantiations
// are held to the two waves per SIMD of the generic kernel -- with every bound a constant the compiler unrolls further and
// would take a 257th register, i.e. half the occupancy)
#ifndef VNL_KERNEL_ATTR
#define VNL_KERNEL_ATTR
#endif
#define VNL_ENV_KERNEL __launch_bounds__(64) VNL_KERNEL_ATTR

// One env per 64-lane workgroup; the env's whole working set lives in dynamic LDS (~25 KB ->
// 6 workgroups per CU, 1536 envs in flight on 256 CUs).
template <class SP>
__global__ void VNL_ENV_KERNEL vnl_step_kernel(const KernelConsts* kc, DevState st, const vreal* action,
                                                      vreal* dump, vreal* dump_mid, int* trace) {
  VNL_LDS_DECL(lds);
  const VNL_CAS KernelConsts* k = VNL_TO_CAS(KernelConsts, kc);
  EnvWaveT<SP> w{k->m, k->ev, st, k->L, lds, blockIdx.x, threadIdx.x, k, nullptr};
  w.step(action, dump_mid, trace);
  if (dump) w.dump(dump);
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
