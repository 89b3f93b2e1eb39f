// Packed input rows (include/pzkwit.h): the group table shared by the host packers (host_api.cpp) and
// the runtime, and k_unpack_inputs, which expands packed rows into the 32-byte rows every other kernel reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pzk {

// One input group of the packed row. The groups tile [0, n_inputs) in flat-input order; byte_off is a multiple of 16.
struct PackedGroup {
  uint32_t elem_off, elem_len;  // the group's elements in the full row
  uint32_t kind;                // PZK_INPUT_BIT | _LIMB | _FIELD
  uint32_t byte_off;            // of the group in the packed row
};
constexpr uint32_t UNPACK_MAX_GROUPS = 32;  // (QueryIdentity has 20)

// bytes of a group without its padding to 16
inline uint64_t packed_group_bytes(uint32_t kind, uint64_t n) {
  return kind == 0 /* BIT */ ? (n + 7) / 8 : kind == 1 /* LIMB */ ? 8 * n : 32 * n;
}

// k_unpack_inputs' tiling: a workgroup of UNPACK_THREADS / 64 waves takes that many consecutive 32-element segments
// of the row (a segment = what one wave-store covers: 64 lanes x 16 B = 1 KiB) for UNPACK_WT consecutive witnesses.
constexpr uint32_t UNPACK_THREADS = 256;
constexpr uint32_t UNPACK_WT = 8;

// packed rows -> full rows on st (kernels_unpack.hip); groups = the instance's device copy of its group table
hipError_t launch_unpack_inputs(const PackedGroup* groups, uint32_t n_groups, uint64_t n_inputs, uint64_t row_bytes,
                                const uint8_t* packed, uint8_t* rows, uint32_t batch, hipStream_t st);

}  // namespace pzk

#ifdef PZK_UNPACK_KERNEL  // defined once, in kernels_unpack.hip

namespace pzk {

// Store-bound: batch x n_inputs x 32 B written, almost nothing read. The emitters' store shape (mapsink.hpp
// store_half): lane l of a wave stores half (l & 1) of element seg + (l >> 1), so every wave-store is 1 KiB of
// contiguous row. A wave keeps its segment of the row over the tile's witnesses: each lane finds its element's group
// once (the table in LDS, at most UNPACK_MAX_GROUPS entries) and then only reads and stores. A BIT group's 32
// elements of a segment are 4 bytes of packed data: every lane reads its byte directly. The upper 31 / 24 bytes of
// a BIT / LIMB element are zero: the odd lanes of such elements store zeros and read nothing.
// Grid: x = segment quads of the row, y = witness tiles (grid-strided). Lanes past the row's end (the partial last
// wave of a row) and witnesses past the batch (the partial last tile) store nothing.
__global__ void __launch_bounds__(UNPACK_THREADS)
k_unpack_inputs(const PackedGroup* __restrict__ groups, uint32_t n_groups, uint32_t n_inputs, uint64_t row_bytes,
                const uint8_t* __restrict__ packed, uint8_t* __restrict__ rows, uint32_t batch) {
  __shared__ PackedGroup tab[UNPACK_MAX_GROUPS];
  if (threadIdx.x < n_groups) tab[threadIdx.x] = groups[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t seg = (blockIdx.x * (UNPACK_THREADS / 64) + wave) * 32;  // first element of the wave's segment
  if (seg >= n_inputs) return;  // whole wave (no barrier follows)
  const uint32_t e = seg + (lane >> 1), half = lane & 1;
  const bool valid = e < n_inputs;
  uint32_t g = 0;
  if (valid)
    while (g + 1 < n_groups && e >= tab[g + 1].elem_off) g++;
  const PackedGroup G = tab[g];
  const uint32_t q = valid ? e - G.elem_off : 0;  // index in the group
  // byte offset of what this lane reads in a packed row, and how it reads it
  const uint32_t kind = G.kind;
  const uint32_t src = G.byte_off + (kind == 2 ? 32 * q + 16 * half : kind == 1 ? 8 * q : q >> 3);
  const uint32_t shift = 7 - (q & 7);
  const bool reads = valid && (kind == 2 || half == 0);
  const uint64_t out_row = 32ull * n_inputs;
  for (uint32_t t = blockIdx.y; (uint64_t)t * UNPACK_WT < batch; t += gridDim.y) {
    const uint32_t w0 = t * UNPACK_WT, nw = batch - w0 < UNPACK_WT ? batch - w0 : UNPACK_WT;
    // the tile's loads first, then its stores: UNPACK_WT independent loads in flight per lane
    uint4 v[UNPACK_WT];
#pragma unroll
    for (uint32_t i = 0; i < UNPACK_WT; i++) {
      v[i] = make_uint4(0u, 0u, 0u, 0u);
      if (reads && i < nw) {
        const uint8_t* p = packed + (uint64_t)(w0 + i) * row_bytes + src;
        if (kind == 2) {
          v[i] = *reinterpret_cast<const uint4*>(p);
        } else if (kind == 1) {
          const uint2 l = *reinterpret_cast<const uint2*>(p);
          v[i].x = l.x;
          v[i].y = l.y;
        } else {
          v[i].x = ((uint32_t)*p >> shift) & 1u;
        }
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < UNPACK_WT; i++)
      if (valid && i < nw) reinterpret_cast<uint4*>(rows + (uint64_t)(w0 + i) * out_row)[2ull * seg + lane] = v[i];
  }
}

}  // namespace pzk
#endif
