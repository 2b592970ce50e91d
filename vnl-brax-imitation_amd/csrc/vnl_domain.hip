// Randomised instantiations of the env kernels (vnl_env_set_domain, vnl_env_set_body_domain): the randomisable model tables --
// five of the contact / actuator / dof parameters, four of the bodies' inertial parameters -- read per env from
// KernelConsts::dom (EnvWaveT::par, par_row).  A translation unit of its own, so that the instantiations of vnl_lib.hip -- the
// specialised rodent step kernel bench.py times among them -- are compiled exactly as without this feature (co-compiled
// template instantiations perturb each other's register allocation).  The host simulation includes it from vnl_lib.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vnl.h"
#ifdef VNL_PROFILE
#define g_vnl_prof g_vnl_prof_domain  // (diagnostic build: the stage stamps of this unit's kernels are kept apart and not read)
#endif
#include "vnl_env_kernels.h"

int vnl_domain_reset_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds, const int* start_frame,
                      const vreal* noise, vreal* dump, int* trace) {
  if (spec)
    hipLaunchKernelGGL((vnl_reset_kernel<VnlSpecDom<VnlSpecRodent>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds,
                       start_frame, noise, dump, trace);
  else
    hipLaunchKernelGGL((vnl_reset_kernel<VnlSpecDom<VnlSpecGeneric>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds,
                       start_frame, noise, dump, trace);
  return (int)hipGetLastError();
}

int vnl_domain_step_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds, const vreal* action,
                     vreal* dump, vreal* dump_mid, int* trace, const vnl_post_desc& post) {
  if (spec)
    hipLaunchKernelGGL((vnl_step_kernel<VnlSpecDom<VnlSpecRodent>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds,
                       action, dump, dump_mid, trace, post);
  else
    hipLaunchKernelGGL((vnl_step_kernel<VnlSpecDom<VnlSpecGeneric>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds,
                       action, dump, dump_mid, trace, post);
  return (int)hipGetLastError();
}

int vnl_domain_reset_done_(const KernelConsts* kc, int spec, int B, size_t lds, void* stream, const DevState& ds,
                           const ResetDoneArgs& a, vreal* dump, int* trace) {
  if (spec)
    hipLaunchKernelGGL((vnl_reset_done_kernel<VnlSpecDom<VnlSpecRodent>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds, a,
                       dump, trace);
  else
    hipLaunchKernelGGL((vnl_reset_done_kernel<VnlSpecDom<VnlSpecGeneric>>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds, a,
                       dump, trace);
  return (int)hipGetLastError();
}

int vnl_domain_redraw_(const KernelConsts* kc, int spec, int B, void* stream, const float* mask, const int64_t* step_base,
                       int64_t step_offset, uint32_t key0, uint32_t key1, uint32_t env0, int initial) {
  if (spec)
    hipLaunchKernelGGL((vnl_redraw_domain_kernel<VnlSpecDom<VnlSpecRodent>>), dim3(B), dim3(64), 0, (hipStream_t)stream, kc, mask,
                       step_base, step_offset, key0, key1, env0, initial);
  else
    hipLaunchKernelGGL((vnl_redraw_domain_kernel<VnlSpecDom<VnlSpecGeneric>>), dim3(B), dim3(64), 0, (hipStream_t)stream, kc, mask,
                       step_base, step_offset, key0, key1, env0, initial);
  return (int)hipGetLastError();
}
