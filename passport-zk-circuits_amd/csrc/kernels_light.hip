// RegisterIdentityLight's prep kernel (light.hpp) and its launcher; own translation unit, so the other kernel
// units are compiled exactly as before.
#include <hip/hip_runtime.h>

#define PZK_TEMPLATE_KERNELS_ONLY
#include "light.hpp"
#include "kernels.hpp"

namespace pzk {

hipError_t launch_light_prep(const DevLayout& L, const uint8_t* inputs, const uint32_t* sha_core, ValueStore vs,
                             int32_t* status, hipStream_t st) {
  if (vs.batch == 0) return hipSuccess;
  // one lane per witness: the last workgroup is partial unless the batch is a multiple of its size
  const uint32_t groups = (vs.batch + LIGHT_PREP_THREADS - 1) / LIGHT_PREP_THREADS;
  hipLaunchKernelGGL(k_light_prep, dim3(groups), dim3(LIGHT_PREP_THREADS), 0, st, L, inputs, sha_core, vs, status);
  return hipGetLastError();
}

}  // namespace pzk
