// k_unpack_inputs (unpack.hpp) and its launcher; own translation unit, so the other kernel units are compiled
// exactly as before.
#include <hip/hip_runtime.h>

#define PZK_UNPACK_KERNEL
#include "unpack.hpp"

namespace pzk {

hipError_t launch_unpack_inputs(const PackedGroup* groups, uint32_t n_groups, uint64_t n_inputs, uint64_t row_bytes,
                                const uint8_t* packed, uint8_t* rows, uint32_t batch, hipStream_t st) {
  if (batch == 0 || n_inputs == 0) return hipSuccess;
  if (n_groups == 0 || n_groups > UNPACK_MAX_GROUPS || n_inputs >> 31) return hipErrorInvalidValue;
  // x: 32-element segments of the row, UNPACK_THREADS / 64 per workgroup (the last one partial unless n_inputs is a
  // multiple of 128); y: tiles of UNPACK_WT witnesses (the last one partial unless the batch is a multiple of it),
  // grid-strided beyond ~4096 workgroups
  const uint32_t per_wg = 32 * (UNPACK_THREADS / 64);
  const uint32_t gx = (uint32_t)((n_inputs + per_wg - 1) / per_wg), tiles = (batch + UNPACK_WT - 1) / UNPACK_WT;
  const uint32_t gy = tiles < 4096 / gx + 1 ? tiles : 4096 / gx + 1;
  hipLaunchKernelGGL(k_unpack_inputs, dim3(gx, gy), dim3(UNPACK_THREADS), 0, st, groups, n_groups, (uint32_t)n_inputs,
                     row_bytes, packed, rows, batch);
  return hipGetLastError();
}

}  // namespace pzk
