// RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) (identityManagement/registerIdentityLight.circom:15-92;
// builder_light.cpp): the one core kernel the circuit adds. Everything else it runs — the SHA cores, the BabyJubJub
// core, the Poseidon levels and every emitter — is shared with the other families.
#pragma once
#include "core_util.hpp"
#include "fr.hpp"
#include "layout.hpp"
#include "poseidon.hpp"

namespace pzk {

constexpr int LIGHT_PREP_THREADS = 64;  // witnesses per k_light_prep workgroup (one wave)

// ============================================================================ k_light_prep
// lane = witness, after the SHA core. The four dg1Chunking outputs, Bits2Num(186 | 190) with in[j] = dg1[i CH + j]
// (:45-51), into the dg1Hasher's input slots, and dg1Hash = Bits2Num(248) of the digest read backwards (:72-86): the
// DG-bit digest as a big-endian integer mod 2^248, from the job's hout words (bit i = word i / 32, bit 31 - i % 32).
// A non-bit dg1 element among the chunked ones flags the lane (the SHA core flags all 1024; skIdentity >= p is
// k_load_values'); the lane's values are then those of the elements' low bits.
__global__ void __launch_bounds__(LIGHT_PREP_THREADS) k_light_prep(DevLayout L, const uint8_t* inputs,
                                                                   const uint32_t* sha_core, ValueStore vs,
                                                                   int32_t* status) {
  core_priority();
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= vs.batch) return;
  const RegInfo& R = L.reg;
  const uint8_t* row = inputs + 32ull * (uint64_t)w * L.n_inputs;
  bool bad = false;
  for (int i = 0; i < 4; i++) {
    fr v = fr_zero();
#pragma unroll
    for (int q = 0; q < 6; q++) {  // CH <= 190 bits: six 32-bit words
      uint32_t word = 0;
      for (int k = 0; k < 32 && 32 * q + k < R.dg1_chunk; k++)
        word |= in_bit(row, R.in_dg1 + i * R.dg1_chunk + 32 * q + k, bad) << k;
      v.v[q] = word;
    }
    vs.at(R.v_dg1 + i, w) = fr_to_mont(v);
  }
  const ShaJob job = L.sha[R.j_dg1];
  const uint32_t* H = sha_core + (size_t)w * L.sha_core_words + job.hout;
  const int nw = job.algo == 1 ? 5 : job.algo == 2 ? 7 : job.algo == 3 ? 12 : job.algo == 4 ? 16 : 8;  // digest words
  fr h = fr_zero();
#pragma unroll
  for (int k = 0; k < 8; k++) h.v[k] = k < nw ? H[nw - 1 - k] : 0u;  // little-endian word k of the integer
  h.v[7] &= 0x00ffffffu;                                            // mod 2^248 (< p)
  vs.at(R.v_dg1hash, w) = fr_to_mont(h);
  if (bad) set_status(status ? status + w : nullptr, ST_INPUT_RANGE);
}

}  // namespace pzk
