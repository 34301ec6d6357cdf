// crash_shield_joint.hip -- crash_shield_joint_kernel (gw_crash_shield_joint): the coordinated crash-aware
// shield, the step outcome preview's safe masks inside the joint shield's sweeps: shield_joint_body with the
// crash preview (shield_joint_core.h).  A translation unit of its own, so that the code objects of gridenv.hip's
// step kernels, of fear_shield_joint.hip and of step_preview.hip do not change with it; gridenv.hip owns the
// preview's record buffer, runs preview_rec_kernel on it and then this kernel (launch_cf: geometry, LDS, span).
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "prof.h"
#include "shield_joint_core.h"

namespace gw {

template <int N>
__global__ void __launch_bounds__(CF_T) crash_shield_joint_kernel(Params p, JointShieldArgs a) {
    shield_joint_body<N, true>(p, a);
}

hipError_t launch_crash_shield_joint(int N, dim3 grid, dim3 block, size_t dyn, hipStream_t s, const Params &p,
                                     const JointShieldArgs &a) {
    return with_agents(N, hipErrorInvalidValue, [&](auto n) {
        gwprof::launch(crash_shield_joint_kernel<decltype(n)::value>, grid, block, dyn, s, p, a);
        return hipSuccess;  // a launch error stays in hipGetLastError for the caller (launch_cf)
    });
}

}  // namespace gw
