// Number-theoretic transforms over BN254 Fr for the quotient stage (include/pzkwit.h pzk_r1cs_quotient_*, DESIGN.md
// §16): the twiddle tables, the pass kernel and the host code that strings passes into a transform. Included by
// kernels_quotient.hip and by the test-only probe (probe/probe_ntt.hip).
//
// A transform of N = 2^k points in HBM (32 B per element, Montgomery form) is a few passes. A pass (d, q) does q
// radix-2 stages: the vector is 2^d sub-transforms of length L = 2^(k - d); within one, index = j * S + lo with
// S = L / 2^q, and the pass transforms the 2^q points j of every column lo. A workgroup holds 2^m points
// (m = min(k, NTT_R)): C = 2^(m - q) neighbouring columns, so that its global accesses come in runs of C elements.
//   inverse (decimation in frequency, natural order in, bit-reversed out): passes d = 0, q1, q1 + q2, ...; after the
//     stages the point at local row j is multiplied by w_L^-(bitrev_q(j) * lo); the last pass (S = 1) multiplies by
//     g^bitrev_k(index) / N (the coset shift) or by 1 / N instead.
//   forward (decimation in time, bit-reversed in, natural out): the same passes in reverse order, each transposed: the
//     factor w_L^+(bitrev_q(j) * lo) first, then the stages. The last pass can fold h = a' b' - c' and the conversion
//     out of Montgomery form (NTT_FWD_QUOT).
// No pass reorders the vector: bit reversal is absorbed by the pair inverse / forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef PZK_NTT_HOST_ONLY  // r1cs.cpp takes the plan and the table layout only
#include "fr.hpp"
#endif

namespace pzk {

constexpr int NTT_R = 10;         // a workgroup holds 2^NTT_R points: 33 KB of LDS + up to 16.5 KB of roots
constexpr int NTT_THREADS = 256;
constexpr int NTT_MAX_K = 24;
constexpr uint32_t NTT_PLANE = (1u << NTT_R) + (1u << (NTT_R - 5));       // words per limb plane, padded
// words per limb plane of a pass's root table, and the pass's LDS bytes: 37 KB at q = 8 (four workgroups per CU),
// 50 KB at q = 10 (three)
constexpr uint32_t ntt_tw_plane(int q) { return (1u << (q - 1)) + ((1u << (q - 1)) >> 5) + 1; }
constexpr uint32_t ntt_pass_lds(int q) { return 32 * (NTT_PLANE + ntt_tw_plane(q)); }

// w_(2^28) = 5^((p - 1) / 2^28), normal form
constexpr uint32_t NTT_ROOT28[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu,
                                    0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};

struct NttPlan { int n = 0; int q[NTT_MAX_K] = {}; };

// the default plan: the fewest passes of at most NTT_R stages, as even as they come, the larger ones first
inline NttPlan ntt_default_plan(int k) {
  NttPlan p;
  p.n = (k + NTT_R - 1) / NTT_R;
  for (int i = 0; i < p.n; i++) p.q[i] = k / p.n + (i < k % p.n ? 1 : 0);
  return p;
}
inline bool ntt_plan_ok(const NttPlan& p, int k) {
  if (k < 1 || k > NTT_MAX_K || p.n < 1 || p.n > NTT_MAX_K) return false;
  int s = 0;
  for (int i = 0; i < p.n; i++) {
    if (p.q[i] < 1 || p.q[i] > NTT_R) return false;
    s += p.q[i];
  }
  return s == k;
}

// One allocation of 32-byte elements in Montgomery form; the members are element offsets.
//   loc_f / loc_i : for q = 1 .. NTT_R at offset 2^(q - 1) - 1: w_(2^q)^(+-j), j < 2^(q - 1)
//   w*_lo, w*_hi  : w_N^(+-e) = hi[e >> t] * lo[e & (2^t - 1)], e < N
//   g_lo, g_hi    : g^e / N the same way (1 / N is in the lo half), g = w_2N
//   n_inv         : 1 / N
struct NttTables {
  const uint8_t* base = nullptr;
  uint32_t loc_f = 0, loc_i = 0, wf_lo = 0, wf_hi = 0, wi_lo = 0, wi_hi = 0, g_lo = 0, g_hi = 0, n_inv = 0, total = 0;
  int k = 0, t = 0;
};
inline NttTables ntt_table_layout(int k) {
  NttTables T;
  T.k = k;
  T.t = (k + 1) / 2;
  const uint32_t lo = 1u << T.t, hi = 1u << (k - T.t), loc = (1u << NTT_R) - 1;
  uint32_t at = 0;
  T.loc_f = at; at += loc;
  T.loc_i = at; at += loc;
  T.wf_lo = at; at += lo;
  T.wf_hi = at; at += hi;
  T.wi_lo = at; at += lo;
  T.wi_hi = at; at += hi;
  T.g_lo = at; at += lo;
  T.g_hi = at; at += hi;
  T.n_inv = at; at += 1;
  T.total = at;
  return T;
}
inline size_t ntt_table_bytes(int k) { return 32ull * ntt_table_layout(k).total; }

#ifndef PZK_NTT_HOST_ONLY

// w_(2^28)^e, e < 2^28, Montgomery form
__device__ __forceinline__ fr ntt_root_pow(uint32_t e) {
  fr sq = fr_to_mont_in(fr_const(NTT_ROOT28)), r = fr_mont_one();
  for (int b = 0; b < 28; b++) {
    if ((e >> b) & 1u) r = fr_mul_fast(r, sq);
    sq = fr_mul_fast(sq, sq);
  }
  return r;
}

// Every table entry from w_(2^28), on the device, once per object (k_qc_build, k_r1cs_coeffs are the precedents).
__global__ void __launch_bounds__(256) k_ntt_tables(uint8_t* __restrict__ out, NttTables T) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T.total) return;
  const uint32_t M28 = (1u << 28) - 1;
  const int k = T.k, t = T.t;
  uint32_t e;
  bool scale = false;
  if (i < T.wf_lo) {  // the two local tables
    const bool inv = i >= T.loc_i;
    const uint32_t j = i - (inv ? T.loc_i : T.loc_f) + 1;  // 2^(q - 1) + jj
    const int q = 32 - __clz(j);
    e = (j - (1u << (q - 1))) << (28 - q);
    if (inv) e = (0u - e) & M28;
  } else if (i < T.g_lo) {
    const bool inv = i >= T.wi_lo;
    const uint32_t lo0 = inv ? T.wi_lo : T.wf_lo, hi0 = inv ? T.wi_hi : T.wf_hi;
    e = i < hi0 ? (i - lo0) << (28 - k) : ((i - hi0) << t) << (28 - k);
    if (inv) e = (0u - e) & M28;
  } else if (i < T.n_inv) {
    scale = i < T.g_hi;
    e = scale ? (i - T.g_lo) << (27 - k) : ((i - T.g_hi) << t) << (27 - k);
  } else {
    e = 0;
    scale = true;
  }
  fr v = ntt_root_pow(e);
  if (scale) v = fr_mul_fast(v, fr_inv<true>(fr_to_mont_in(fr_u64(1ull << k))));
  store_fr(out + 32ull * i, v);
}

// vector z of row y lies at base[z] + y * stride[z]
struct NttVecs { uint8_t* base[3]; uint64_t stride[3]; };

enum { NTT_INV = 0, NTT_INV_SHIFT, NTT_INV_SCALE, NTT_FWD, NTT_FWD_QUOT };

__device__ __forceinline__ uint32_t ntt_pad(uint32_t i) { return i + (i >> 5); }
__device__ __forceinline__ fr ntt_lds_ld(const uint32_t* s, uint32_t plane, uint32_t i) {
  fr r;
  const uint32_t a = ntt_pad(i);
#pragma unroll
  for (int w = 0; w < 8; w++) r.v[w] = s[w * plane + a];
  return r;
}
__device__ __forceinline__ void ntt_lds_st(uint32_t* s, uint32_t plane, uint32_t i, const fr& x) {
  const uint32_t a = ntt_pad(i);
#pragma unroll
  for (int w = 0; w < 8; w++) s[w * plane + a] = x.v[w];
}
__device__ __forceinline__ fr ntt_two_level(const uint8_t* __restrict__ base, uint32_t lo0, uint32_t hi0, int t, uint32_t e) {
  return fr_mul_fast(load_fr(base + 32ull * (hi0 + (e >> t))), load_fr(base + 32ull * (lo0 + (e & ((1u << t) - 1)))));
}

// One pass (d, q) of the file comment over vectors v.base[0 .. gridDim.z) of rows 0 .. gridDim.y; grid x: the
// 2^(k - m) tiles. The points lie in LDS one 32-bit limb per plane, index i at word i + (i >> 5) of each plane: a
// wave's limb reads and writes of consecutive points, and of points C apart per lane, fall on distinct banks. The
// pass loads (16 B per lane, global order), computes, then stores (16 B per lane, contiguous per wave).
// NTT_FWD_QUOT (gridDim.z = 1): v.base[0] is c, v.base[1] a' and v.base[2] b'; the result a' b' - c', out of
// Montgomery form, is written over a'.
template <int MODE>
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_pass(NttVecs v, int k, int d, int q, NttTables T) {
  extern __shared__ uint32_t s_ntt[];  // ntt_pass_lds(q) bytes: the points, then the pass's 2^(q - 1) roots
  uint32_t* s_pt = s_ntt;
  uint32_t* s_tw = s_ntt + 8 * NTT_PLANE;
  const uint32_t tw_plane = ntt_tw_plane(q);
  constexpr bool FWD = MODE == NTT_FWD || MODE == NTT_FWD_QUOT;
  const uint32_t tid = threadIdx.x;
  const int m = k < NTT_R ? k : NTT_R, logC = m - q, logS = k - d - q;
  const uint32_t n_pt = 1u << m, C = 1u << logC, S = 1u << logS, o0 = blockIdx.x << logC;
  const uint32_t vz = MODE == NTT_FWD_QUOT ? 0 : blockIdx.z;
  uint8_t* row = v.base[vz] + (uint64_t)blockIdx.y * v.stride[vz];
  // local index (row j, column c) -> index in the vector
  auto gidx = [&](uint32_t idx) -> uint32_t {
    const uint32_t j = idx >> logC, o = o0 + (idx & (C - 1));
    return ((o >> logS) << (logS + q)) + (j << logS) + (o & (S - 1));
  };
  // u-th element of the tile in global order -> local index (when S < C the tile is one contiguous run)
  auto lidx = [&](uint32_t u) -> uint32_t {
    if (logS >= logC) return u;
    const uint32_t lo = u & (S - 1), j = (u >> logS) & ((1u << q) - 1), rr = u >> (logS + q);
    return (j << logC) | (rr << logS) | lo;
  };
  // the 2^q-th roots of this pass
  {
    const uint32_t t0 = (FWD ? T.loc_f : T.loc_i) + (1u << (q - 1)) - 1;
    for (uint32_t j = tid; j < (1u << (q - 1)); j += NTT_THREADS)
      ntt_lds_st(s_tw, tw_plane, j, load_fr(T.base + 32ull * (t0 + j)));
  }
  for (uint32_t u2 = tid; u2 < 2 * n_pt; u2 += NTT_THREADS) {
    const uint32_t idx = lidx(u2 >> 1), hf = u2 & 1;
    const uint4 x = *reinterpret_cast<const uint4*>(row + 32ull * gidx(idx) + 16 * hf);
    uint32_t* s = s_pt + 4 * hf * NTT_PLANE + ntt_pad(idx);
    s[0] = x.x; s[NTT_PLANE] = x.y; s[2 * NTT_PLANE] = x.z; s[3 * NTT_PLANE] = x.w;
  }
  __syncthreads();
  // the factor between this pass and its neighbour: exponent bitrev_q(j) * lo * 2^d of w_N
  auto twid = [&](uint32_t idx) -> uint32_t {
    const uint32_t j = idx >> logC, lo = (o0 + (idx & (C - 1))) & (S - 1);
    return ((__brev(j) >> (32 - q)) * lo) << d;
  };
  if (FWD && logS > 0) {
    for (uint32_t idx = tid; idx < n_pt; idx += NTT_THREADS)
      ntt_lds_st(s_pt, NTT_PLANE, idx,
                 fr_mul_fast(ntt_lds_ld(s_pt, NTT_PLANE, idx), ntt_two_level(T.base, T.wf_lo, T.wf_hi, T.t, twid(idx))));
    __syncthreads();
  }
  for (int s = 0; s < q; s++) {
    const int t = FWD ? s : q - 1 - s, lh = logC + t;
    for (uint32_t b = tid; b < n_pt / 2; b += NTT_THREADS) {
      const uint32_t lo = b & ((1u << lh) - 1), i0 = ((b >> lh) << (lh + 1)) | lo, i1 = i0 + (1u << lh);
      const fr x = ntt_lds_ld(s_pt, NTT_PLANE, i0);
      fr y = ntt_lds_ld(s_pt, NTT_PLANE, i1);
      if (FWD) {
        if (t > 0) y = fr_mul_fast(y, ntt_lds_ld(s_tw, tw_plane, (lo >> logC) << (q - 1 - t)));  // t = 0: the root is 1
        ntt_lds_st(s_pt, NTT_PLANE, i0, fr_add(x, y));
        ntt_lds_st(s_pt, NTT_PLANE, i1, fr_sub(x, y));
      } else {
        fr z = fr_sub(x, y);
        if (t > 0) z = fr_mul_fast(z, ntt_lds_ld(s_tw, tw_plane, (lo >> logC) << (q - 1 - t)));
        ntt_lds_st(s_pt, NTT_PLANE, i0, fr_add(x, y));
        ntt_lds_st(s_pt, NTT_PLANE, i1, z);
      }
    }
    __syncthreads();
  }
  if (MODE != NTT_FWD) {
    for (uint32_t idx = tid; idx < n_pt; idx += NTT_THREADS) {
      fr x = ntt_lds_ld(s_pt, NTT_PLANE, idx);
      if (MODE == NTT_INV) {
        x = fr_mul_fast(x, ntt_two_level(T.base, T.wi_lo, T.wi_hi, T.t, twid(idx)));
      } else if (MODE == NTT_INV_SHIFT) {
        x = fr_mul_fast(x, ntt_two_level(T.base, T.g_lo, T.g_hi, T.t, __brev(gidx(idx)) >> (32 - k)));
      } else if (MODE == NTT_INV_SCALE) {
        x = fr_mul_fast(x, load_fr(T.base + 32ull * T.n_inv));
      } else {
        const uint64_t at = 32ull * gidx(idx);
        const fr a = load_fr(v.base[1] + (uint64_t)blockIdx.y * v.stride[1] + at);
        const fr b = load_fr(v.base[2] + (uint64_t)blockIdx.y * v.stride[2] + at);
        x = fr_from_mont_fast(fr_sub(fr_mul_fast(a, b), x));
      }
      ntt_lds_st(s_pt, NTT_PLANE, idx, x);
    }
    __syncthreads();
  }
  uint8_t* out = MODE == NTT_FWD_QUOT ? v.base[1] + (uint64_t)blockIdx.y * v.stride[1] : row;
  for (uint32_t u2 = tid; u2 < 2 * n_pt; u2 += NTT_THREADS) {
    const uint32_t idx = lidx(u2 >> 1), hf = u2 & 1;
    const uint32_t* s = s_pt + 4 * hf * NTT_PLANE + ntt_pad(idx);
    *reinterpret_cast<uint4*>(out + 32ull * gidx(idx) + 16 * hf) = make_uint4(s[0], s[NTT_PLANE], s[2 * NTT_PLANE], s[3 * NTT_PLANE]);
  }
}

template <int MODE>
inline hipError_t ntt_launch_pass(const NttVecs& v, int nvec, int rows, int k, int d, int q, const NttTables& T, hipStream_t st) {
  const int m = k < NTT_R ? k : NTT_R;
  hipLaunchKernelGGL(k_ntt_pass<MODE>, dim3(1u << (k - m), rows, nvec), dim3(NTT_THREADS), ntt_pass_lds(q), st, v, k, d, q, T);
  return hipGetLastError();
}

// tables for 2^k points into d_tables (ntt_table_bytes(k) bytes) on st
inline hipError_t ntt_build_tables(uint8_t* d_tables, int k, NttTables& T, hipStream_t st) {
  T = ntt_table_layout(k);
  T.base = d_tables;
  hipLaunchKernelGGL(k_ntt_tables, dim3((T.total + 255) / 256), dim3(256), 0, st, d_tables, T);
  return hipGetLastError();
}

// natural order in, bit-reversed out; the last pass multiplies by g^i / N (shift) or by 1 / N
inline hipError_t ntt_inverse(const NttVecs& v, int nvec, int rows, const NttPlan& pl, const NttTables& T, bool shift, hipStream_t st) {
  int d = 0;
  for (int i = 0; i < pl.n; i++) {
    hipError_t e;
    if (i < pl.n - 1) e = ntt_launch_pass<NTT_INV>(v, nvec, rows, T.k, d, pl.q[i], T, st);
    else if (shift) e = ntt_launch_pass<NTT_INV_SHIFT>(v, nvec, rows, T.k, d, pl.q[i], T, st);
    else e = ntt_launch_pass<NTT_INV_SCALE>(v, nvec, rows, T.k, d, pl.q[i], T, st);
    if (e != hipSuccess) return e;
    d += pl.q[i];
  }
  return hipSuccess;
}

// bit-reversed in, natural out. quot: v is {c, a', b'} and the last pass writes a' b' - c' over a' (nvec = 1)
inline hipError_t ntt_forward(const NttVecs& v, int nvec, int rows, const NttPlan& pl, const NttTables& T, bool quot, hipStream_t st) {
  int d = T.k;
  for (int i = pl.n - 1; i >= 0; i--) {
    d -= pl.q[i];
    const hipError_t e = (i == 0 && quot) ? ntt_launch_pass<NTT_FWD_QUOT>(v, 1, rows, T.k, d, pl.q[i], T, st)
                                          : ntt_launch_pass<NTT_FWD>(v, nvec, rows, T.k, d, pl.q[i], T, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#endif  // PZK_NTT_HOST_ONLY

}  // namespace pzk
