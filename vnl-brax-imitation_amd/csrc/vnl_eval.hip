// The step kernels that score an evaluation (vnl_env_step_post_eval: vnl_step_eval_kernel of vnl_env_kernels.h), for the
// shared model and for per-env parameter tables.  A translation unit of its own, like vnl_domain.hip and for its reason: the
// step kernels of vnl_lib.hip and vnl_domain.hip -- the ones a rollout launches and bench.py times -- are compiled exactly as
// without this feature.  The host simulation includes it from vnl_lib.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vnl.h"
#ifdef VNL_PROFILE
#define g_vnl_prof g_vnl_prof_eval  // (diagnostic build: the stage stamps of this unit's kernels are kept apart and not read)
#endif
#include "vnl_env_kernels.h"

template <class SP>
static int vnl_eval_step_launch(const KernelConsts* kc, int B, size_t lds, void* stream, const DevState& ds, const vreal* action,
                                vreal* dump, vreal* dump_mid, int* trace, const vnl_post_desc& post, const vnl_eval_desc& ev) {
  hipLaunchKernelGGL((vnl_step_eval_kernel<SP>), dim3(B), dim3(64), lds, (hipStream_t)stream, kc, ds, action, dump, dump_mid,
                     trace, post, ev);
  return (int)hipGetLastError();
}

// `spec`: the specialised rodent instantiation; `dom`: the env has per-env tables (vnl_env_set_domain / _body_domain)
int vnl_eval_step_(const KernelConsts* kc, int spec, int dom, int B, size_t lds, void* stream, const DevState& ds,
                   const vreal* action, vreal* dump, vreal* dump_mid, int* trace, const vnl_post_desc& post,
                   const vnl_eval_desc& ev) {
  if (dom)
    return spec ? vnl_eval_step_launch<VnlSpecDom<VnlSpecRodent>>(kc, B, lds, stream, ds, action, dump, dump_mid, trace, post, ev)
                : vnl_eval_step_launch<VnlSpecDom<VnlSpecGeneric>>(kc, B, lds, stream, ds, action, dump, dump_mid, trace, post, ev);
  return spec ? vnl_eval_step_launch<VnlSpecRodent>(kc, B, lds, stream, ds, action, dump, dump_mid, trace, post, ev)
              : vnl_eval_step_launch<VnlSpecGeneric>(kc, B, lds, stream, ds, action, dump, dump_mid, trace, post, ev);
}
