// circom .r1cs files checked on the GPU (include/pzkwit.h pzk_r1cs_*): the device program the host
// parser (r1cs.cpp) produces from a file, the host evaluator (the kernels' twin), and k_r1cs_check / k_r1cs_check_long,
// which evaluate A.w * B.w = C.w over a batch of witness rows resident in HBM (kernels_r1cs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

namespace pzk {

// A constraint is short when each of its three LCs has at most R1CS_LONG_T terms (after merging). Short constraints
// run a lane per constraint in chunks; a constraint with a longer LC (Bits2Num(254)'s sum) runs a wave per constraint.
constexpr uint32_t R1CS_LONG_T = 32;
constexpr uint32_t R1CS_WT = 8;              // witnesses per tile: a workgroup reuses its staged chunk over them
constexpr uint32_t R1CS_THREADS = 256;       // four waves
constexpr uint32_t R1CS_CHUNK_C = 256;       // constraints per chunk at most: one per lane of the workgroup
// terms per chunk at most: 20 KB of LDS + 1.5 KB of offsets per workgroup, so that the kernel's registers (four waves
// per SIMD), not its LDS, bound the workgroups per CU. A short constraint has at most 3 * R1CS_LONG_T = 96 terms, so a
// chunk always holds at least 26 constraints.
constexpr uint32_t R1CS_CHUNK_TERMS = 2560;
static_assert(3 * R1CS_LONG_T <= R1CS_CHUNK_TERMS && R1CS_CHUNK_TERMS < 65536, "chunk offsets are 16-bit");

struct R1csTerm { uint32_t wire, coeff; };   // coeff: index into the coefficient table; 0 = +1, 1 = p - 1 (= -1)
struct R1csChunk { uint32_t first, count; }; // constraints first .. first + count - 1 (file order), all short

// The parsed system. LC j of constraint k (j = 0, 1, 2 for A, B, C) is terms[lc_off[3k + j] .. lc_off[3k + j + 1]):
// wires ascending, each once, no zero coefficient.
struct R1csProgram {
  uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_constraints = 0, max_terms = 0;
  uint64_t n_labels = 0;
  std::vector<uint32_t> lc_off;     // 3 * n_constraints + 1
  std::vector<R1csTerm> terms;
  std::vector<uint64_t> coeffs;     // 4 little-endian words per coefficient, NORMAL form; entries 0 and 1 are 1, p - 1
  std::vector<R1csChunk> chunks;
  std::vector<uint32_t> long_list;  // constraint indices, ascending
};

// bytes of a .r1cs file -> program; false (why set): the file is rejected (pzkwit.h lists the reasons)
bool r1cs_parse(const uint8_t* bytes, size_t len, R1csProgram& out, std::string& why);
// one witness row (32 B little-endian per wire, any 256-bit value: it counts as its residue) -> the lowest violated
// constraint index or -1, and the number of violated constraints. Plain C++, no device.
void r1cs_eval_row(const R1csProgram& P, const uint8_t* row, int32_t& first_failed, uint32_t& n_failed);

// device copy of a program (kernels_r1cs.hip); coeffs in Montgomery form
struct R1csDevice {
  uint32_t* lc_off = nullptr;
  R1csTerm* terms = nullptr;
  uint32_t* coeffs = nullptr;  // 8 words per coefficient
  R1csChunk* chunks = nullptr;
  uint32_t* long_list = nullptr;
  hipStream_t stream = nullptr;
  // the quotient stage (kernels_quotient.hip), allocated at the first quotient call: the transforms' tables, and the
  // b and c vectors of a tile of quot_rows witnesses
  uint8_t* quot_tables = nullptr;
  uint8_t* quot_scratch = nullptr;
  uint32_t quot_rows = 0;
};

// The quotient's domain (pzkwit.h): M = n_constraints + n_pub_out + n_pub_in + 1 rows, N = 2^k >= M. false: k is
// outside 1 .. 24.
constexpr uint32_t QUOT_TILE = 8;  // witnesses per tile of scratch
bool r1cs_quotient_domain(const R1csProgram& P, uint64_t& m, int& k);
// one witness row -> h, 32 N bytes, normal form. Plain C++, no device (r1cs.cpp).
void r1cs_quotient_row(const R1csProgram& P, int k, const uint8_t* row, uint8_t* h);

}  // namespace pzk

// the C ABI's handle. Host state is r1cs.cpp's; the device half is filled at the first check by kernels_r1cs.hip,
// which also sets dev_free (r1cs.cpp has no HIP runtime calls: tools/fuzz builds it with the host sanitizers).
struct pzk_r1cs {
  pzk::R1csProgram prog;
  std::mutex mu;
  int device = -1;  // bound at the first check
  pzk::R1csDevice dev;
  void (*dev_free)(pzk_r1cs*) = nullptr;
  double quot_ms[4] = {0, 0, 0, 0};  // pzk_r1cs_quotient_timing
};

// the device half, shared by the check and the quotient (kernels_r1cs.hip): the device an object is bound to at its
// first device call, and the upload of its program there (under the object's mutex, on the bound device)
namespace pzk {
struct R1csDevGuard {  // the caller's current device is restored on return (runtime.cpp DeviceGuard)
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit R1csDevGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    else prev = -1;
  }
  ~R1csDevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace pzk
struct pzk_exec;
namespace pzk {
int r1cs_bind(pzk_r1cs* r, const pzk_exec* ex);
int r1cs_ensure_device(pzk_r1cs* r);
}  // namespace pzk

#ifdef PZK_R1CS_KERNEL  // defined in kernels_r1cs.hip and kernels_quotient.hip
#include "fr.hpp"

namespace pzk {

// a witness element as its residue: rows this project writes are below p (the loop is then not entered); 2^256 - 1
// takes five subtractions
__device__ __forceinline__ fr r1cs_residue(fr w) {
  while (fr_geq_p(w)) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { uint64_t d = (uint64_t)w.v[i] - P_[i] - br; w.v[i] = (uint32_t)d; br = (d >> 32) & 1; }
  }
  return w;
}

// acc += c * w for one term, everything in normal form: +-1 add or subtract the residue; any other coefficient is in
// Montgomery form, and fr_mul(cM, w) = c * w mod p, canonical, for any 256-bit w (fr.hpp fr_to_mont_in: the first
// operand is the one that must be below p)
__device__ __forceinline__ fr r1cs_term(const fr& acc, const R1csTerm t, const uint32_t* __restrict__ coeffs,
                                        const uint8_t* __restrict__ row) {
  const fr w = load_fr(row + 32ull * t.wire);
  if (t.coeff == 0) return fr_add(acc, r1cs_residue(w));
  if (t.coeff == 1) return fr_sub(acc, r1cs_residue(w));
  fr c;
  const uint4* cp = reinterpret_cast<const uint4*>(coeffs + 8ull * t.coeff);
  const uint4 lo = cp[0], hi = cp[1];
  c.v[0] = lo.x; c.v[1] = lo.y; c.v[2] = lo.z; c.v[3] = lo.w; c.v[4] = hi.x; c.v[5] = hi.y; c.v[6] = hi.z; c.v[7] = hi.w;
  return fr_add(acc, fr_mul(c, w));
}

__device__ __forceinline__ void r1cs_report(int32_t* first_failed, uint32_t* n_failed, uint32_t witness, uint32_t k) {
  atomicMin(reinterpret_cast<uint32_t*>(first_failed) + witness, k);  // pre-set to 0xFFFFFFFF (= -1: none)
  if (n_failed) atomicAdd(n_failed + witness, 1u);
}

#ifndef PZK_R1CS_NO_KERNELS  // kernels_quotient.hip takes the device functions only
// The coefficient table, uploaded in normal form, to Montgomery form in place (once, at the first check).
__global__ void __launch_bounds__(256) k_r1cs_coeffs(uint32_t* __restrict__ coeffs, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint8_t* p = reinterpret_cast<uint8_t*>(coeffs + 8ull * i);
  store_fr(p, fr_to_mont_in(load_fr(p)));
}

// Short constraints. A workgroup takes chunks (grid x, strided) and witness tiles (grid y, strided): it stages the
// chunk's slice of the CSR in LDS once (offsets relative to the chunk, 16-bit; terms) and reuses it over every witness
// of its tiles, so the term list is read from HBM once per tile row of the grid, not once per witness. Lane l owns
// constraint chunk.first + l and runs its three LCs per witness: terms from LDS, elements gathered from the row with
// one 32-byte load each (neighbouring constraints read neighbouring wires: a wave's gathers fall in a few KB). A, B, C
// accumulate in normal form; the test is A * B / R == C / R (two Montgomery products). No cross-lane operation:
// lanes past the chunk's end idle, witnesses past the batch are not read.
__global__ void __launch_bounds__(R1CS_THREADS)
k_r1cs_check(const R1csChunk* __restrict__ chunks, uint32_t n_chunks, const uint32_t* __restrict__ lc_off,
             const R1csTerm* __restrict__ terms, const uint32_t* __restrict__ coeffs, const uint8_t* __restrict__ rows,
             uint64_t stride, uint32_t batch, int32_t* __restrict__ first_failed, uint32_t* __restrict__ n_failed) {
  __shared__ R1csTerm s_terms[R1CS_CHUNK_TERMS];
  __shared__ uint16_t s_off[3 * R1CS_CHUNK_C + 1];
  fr one = fr_zero();
  one.v[0] = 1;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const R1csChunk ch = chunks[c];
    const uint32_t t0 = lc_off[3ull * ch.first];
    const uint32_t nt = lc_off[3ull * (ch.first + ch.count)] - t0;  // <= R1CS_CHUNK_TERMS (the parser's chunking)
    __syncthreads();  // the previous chunk's readers are done
    for (uint32_t i = threadIdx.x; i <= 3 * ch.count; i += R1CS_THREADS) s_off[i] = (uint16_t)(lc_off[3ull * ch.first + i] - t0);
    for (uint32_t i = threadIdx.x; i < nt && i < R1CS_CHUNK_TERMS; i += R1CS_THREADS) s_terms[i] = terms[(uint64_t)t0 + i];
    __syncthreads();
    if (threadIdx.x < ch.count) {
      const uint32_t k = ch.first + threadIdx.x;
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = s_off[3 * threadIdx.x + j];
      for (uint32_t t = blockIdx.y; (uint64_t)t * R1CS_WT < batch; t += gridDim.y) {
        const uint32_t w0 = t * R1CS_WT, nw = batch - w0 < R1CS_WT ? batch - w0 : R1CS_WT;
        for (uint32_t i = 0; i < nw; i++) {
          const uint8_t* row = rows + (uint64_t)(w0 + i) * stride;
          fr a = fr_zero(), b = fr_zero(), cc = fr_zero();
          for (uint32_t q = o[0]; q < o[1]; q++) a = r1cs_term(a, s_terms[q], coeffs, row);
          for (uint32_t q = o[1]; q < o[2]; q++) b = r1cs_term(b, s_terms[q], coeffs, row);
          for (uint32_t q = o[2]; q < o[3]; q++) cc = r1cs_term(cc, s_terms[q], coeffs, row);
          if (!fr_eq(fr_mul(a, b), fr_mul(cc, one))) r1cs_report(first_failed, n_failed, w0 + i, k);
        }
      }
    }
  }
}

#endif  // PZK_R1CS_NO_KERNELS

// sum over the wave's 64 lanes, valid in lane 0; every lane of the wave calls it (outside any divergent branch: a
// lane without a term passes 0)
__device__ __forceinline__ fr r1cs_wave_sum(fr v) {
#pragma unroll
  for (unsigned d = 32; d >= 1; d >>= 1) v = fr_add(v, fr_shfl_down(v, d));
  return v;
}

#ifndef PZK_R1CS_NO_KERNELS
// Long constraints: a wave per constraint (grid x over groups of four, strided) and witness tile (grid y, strided).
// Lanes take the terms of each LC strided by 64 from global memory (contiguous 8-byte reads), the 64 partial sums
// are reduced with fr_add over fr_shfl_down, lane 0 tests and reports. The loop bounds and the exit are uniform over
// the wave, and the kernel has no workgroup barrier.
__global__ void __launch_bounds__(R1CS_THREADS)
k_r1cs_check_long(const uint32_t* __restrict__ long_list, uint32_t n_long, const uint32_t* __restrict__ lc_off,
                  const R1csTerm* __restrict__ terms, const uint32_t* __restrict__ coeffs,
                  const uint8_t* __restrict__ rows, uint64_t stride, uint32_t batch, int32_t* __restrict__ first_failed,
                  uint32_t* __restrict__ n_failed) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  fr one = fr_zero();
  one.v[0] = 1;
  for (uint64_t g = (uint64_t)blockIdx.x * (R1CS_THREADS / 64) + wave; g < n_long;
       g += (uint64_t)gridDim.x * (R1CS_THREADS / 64)) {
    const uint32_t k = long_list[g];
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = lc_off[3ull * k + j];
    for (uint32_t t = blockIdx.y; (uint64_t)t * R1CS_WT < batch; t += gridDim.y) {
      const uint32_t w0 = t * R1CS_WT, nw = batch - w0 < R1CS_WT ? batch - w0 : R1CS_WT;
      for (uint32_t i = 0; i < nw; i++) {
        const uint8_t* row = rows + (uint64_t)(w0 + i) * stride;
        fr a = fr_zero(), b = fr_zero(), cc = fr_zero();
        for (uint32_t q = o[0] + lane; q < o[1]; q += 64) a = r1cs_term(a, terms[q], coeffs, row);
        for (uint32_t q = o[1] + lane; q < o[2]; q += 64) b = r1cs_term(b, terms[q], coeffs, row);
        for (uint32_t q = o[2] + lane; q < o[3]; q += 64) cc = r1cs_term(cc, terms[q], coeffs, row);
        a = r1cs_wave_sum(a);
        b = r1cs_wave_sum(b);
        cc = r1cs_wave_sum(cc);
        if (lane == 0 && !fr_eq(fr_mul(a, b), fr_mul(cc, one))) r1cs_report(first_failed, n_failed, w0 + i, k);
      }
    }
  }
}

#endif  // PZK_R1CS_NO_KERNELS

}  // namespace pzk
#endif
