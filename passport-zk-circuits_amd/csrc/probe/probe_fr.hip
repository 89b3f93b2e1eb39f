// Probe kernels for the BN254 Fr primitives (fr.hpp, core_util.hpp), the quad-spread products (fq.hpp) and the
// 64-bit-word divisions (core_util.hpp divlu, regcore.hpp div_preinv, rsa_coop.hpp kd_div). One case per lane, one
// per quad for fq. See probe.h.
#define PZK_TEMPLATE_KERNELS_ONLY  // the headers' own switch: only their templates, no kernel definitions here
#include <hip/hip_runtime.h>

#include "../core_util.hpp"
#include "../fq.hpp"
#include "../fr.hpp"
#include "../regcore.hpp"
#include "../rsa_coop.hpp"
#include "probe_util.hpp"

using namespace pzk;
using namespace pzkprobe;

namespace {

__device__ __forceinline__ fr ld8(const uint32_t* p) { fr r; for (int i = 0; i < 8; i++) r.v[i] = p[i]; return r; }
__device__ __forceinline__ void st8(uint32_t* p, const fr& a) { for (int i = 0; i < 8; i++) p[i] = a.v[i]; }

// ------------------------------------------------------------------ fr
template <int OP>
__global__ void __launch_bounds__(64) k_probe_fr(const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  const fr x = ld8(a + 8 * c);
  fr y = fr_zero();
  if (b) y = ld8(b + 8 * c);
  fr r = fr_zero();
  if constexpr (OP == PFR_ADD) r = fr_add(x, y);
  else if constexpr (OP == PFR_SUB) r = fr_sub(x, y);
  else if constexpr (OP == PFR_REDUCE_ONCE) r = fr_reduce_once(x);
  else if constexpr (OP == PFR_GEQ_P) r.v[0] = fr_geq_p(x) ? 1u : 0u;
  else if constexpr (OP == PFR_MUL) r = fr_mul(x, y);
  else if constexpr (OP == PFR_SQR) r = fr_sqr(x);
  else if constexpr (OP == PFR_MUL_FAST) r = fr_mul_fast(x, y);
  else if constexpr (OP == PFR_FROM_MONT) r = fr_from_mont(x);
  else if constexpr (OP == PFR_FROM_MONT_FAST) r = fr_from_mont_fast(x);
  else if constexpr (OP == PFR_TO_MONT) r = fr_to_mont(x);
  else if constexpr (OP == PFR_TO_MONT_IN) r = fr_to_mont_in(x);
  else if constexpr (OP == PFR_INV) r = fr_inv<false>(x);
  else if constexpr (OP == PFR_INV_FAST) r = fr_inv<true>(x);
  else if constexpr (OP == PFR_INV_SW) r = fr_inv_sw<false>(x);
  else if constexpr (OP == PFR_INV_SW_FAST) r = fr_inv_sw<true>(x);
  else if constexpr (OP == PFR_FROM_I128)
    r = fr_from_i128((uint64_t)x.v[1] << 32 | x.v[0], (uint64_t)x.v[3] << 32 | x.v[2]);
  st8(out + 8 * c, r);
}

struct FrArr {
  fr* p;
  __device__ __forceinline__ fr& operator()(int i) const { return p[i]; }
};
__global__ void __launch_bounds__(64) k_probe_fr_batch_inv(const uint32_t* x, uint32_t* out, int n, int m) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  fr xs[8], sc[8];
  for (int i = 0; i < 8; i++) { xs[i] = i < m ? ld8(x + 8 * ((size_t)c * m + i)) : fr_zero(); sc[i] = fr_zero(); }
  fr_batch_inv(FrArr{xs}, FrArr{sc}, m);
  for (int i = 0; i < m; i++) st8(out + 8 * ((size_t)c * m + i), xs[i]);
}

// ------------------------------------------------------------------ fq
// Every lane of every wave runs the operation (the settles ballot over the wave); quads past the end compute on zeros
// and skip the store.
template <int OP>
__global__ void __launch_bounds__(64) k_probe_fq(const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out,
                                                 uint32_t* out_canon, int n) {
  const int lane = blockIdx.x * 64 + threadIdx.x, c = lane >> 2;
  const bool valid = c < n;
  const QLane ql = QLane::make();
  fr fa = fr_zero(), fk = fr_zero(), fb[3] = {fr_zero(), fr_zero(), fr_zero()};
  if (valid) {
    fa = ld8(a + 8 * c);
    if (b) for (int r = 0; r < 3; r++) fb[r] = ld8(b + 8 * (3 * (size_t)c + r));
    if (k) fk = ld8(k + 8 * c);
  }
  const fq qa = fq_digit(fa, ql.q), qk = fq_digit(fk, ql.q);
  const fq qb[3] = {fq_digit(fb[0], ql.q), fq_digit(fb[1], ql.q), fq_digit(fb[2], ql.q)};
  auto rows = [&](int r, auto J) {
    constexpr int j = decltype(J)::value;
    return r == 0 ? rword<0, j>(qa) : r == 1 ? rword<1, j>(qa) : rword<2, j>(qa);
  };
  fq res = fq_zero();
  bool flag = false;
  if constexpr (OP == PFQ_MUL) res = fq_mul(qa, qb[0], ql);
  else if constexpr (OP == PFQ_MUL64) res = fq_mul64(qa, qb[0], ql);
  else if constexpr (OP == PFQ_MULQ) res = fq_mulq(qa, qb[0], ql);
  else if constexpr (OP == PFQ_DOT1) { const fq bb[1] = {qb[0]}; res = fq_dot<1>(rows, bb, qk, ql); }
  else if constexpr (OP == PFQ_DOT2) { const fq bb[2] = {qb[0], qb[1]}; res = fq_dot<2>(rows, bb, qk, ql); }
  else if constexpr (OP == PFQ_DOT3) res = fq_dot<3>(rows, qb, qk, ql);
  else if constexpr (OP == PFQ_CANON) res = fq_canon(qa, ql);
  else if constexpr (OP == PFQ_GEQ_P) flag = fq_geq_p(qa, ql);
  else if constexpr (OP == PFQ_ADD_RAW) res = fq_add_raw(qa, qb[0]);
  fr g = fq_gather(res);
  if constexpr (OP == PFQ_GEQ_P) { g = fr_zero(); g.v[0] = flag ? 1u : 0u; }
  // the chain's two conditional subtractions, only for the products (their results are below 3p; fq_add_raw's and
  // fq_geq_p's are outside fq_canon's domain)
  fr gc = fr_zero();
  if constexpr (OP <= PFQ_DOT3) gc = fq_gather(fq_canon(fq_canon(res, ql), ql));
  if (valid && ql.q == 0) {
    st8(out + 8 * c, g);
    if (out_canon) st8(out_canon + 8 * c, gc);
  }
}

// ------------------------------------------------------------------ divisions
template <int OP>
__global__ void __launch_bounds__(64) k_probe_div64(const uint64_t* u1, const uint64_t* u0, const uint64_t* v,
                                                    uint64_t* q, uint64_t* r, int n) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  uint64_t rem = 0, quo;
  if constexpr (OP == PDIV_DIVLU) {
    quo = divlu(u1[c], u0[c], v[c], &rem);
  } else {
    uint64_t vinv_r;
    const uint64_t vinv = divlu(~v[c], ~0ull, v[c], &vinv_r);
    quo = div_preinv(u1[c], u0[c], v[c], vinv, &rem);
  }
  q[c] = quo;
  r[c] = rem;
}

__global__ void __launch_bounds__(64) k_probe_kd_div(const uint64_t* a, const int* na, int sa, const uint64_t* b,
                                                     const int* nb, int sb, uint64_t* q, uint64_t* r, uint64_t* un,
                                                     uint64_t* vn, int n) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  kd_div(a + (size_t)c * sa, na[c], b + (size_t)c * sb, nb[c], q + (size_t)c * sa, r + (size_t)c * sb,
         un + (size_t)c * (sa + 1), vn + (size_t)c * sb);
}

template <int OP = 0>
int run_fr(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  if constexpr (OP < PFR_N_OPS) {
    if (op != OP) return run_fr<OP + 1>(op, a, b, out, n);
    hipLaunchKernelGGL(k_probe_fr<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, a, b, out, n);
    return (int)finish();
  } else {
    return (int)hipErrorInvalidValue;
  }
}
template <int OP = 0>
int run_fq(int op, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out, uint32_t* oc, int n) {
  if constexpr (OP < PFQ_N_OPS) {
    if (op != OP) return run_fq<OP + 1>(op, a, b, k, out, oc, n);
    hipLaunchKernelGGL(k_probe_fq<OP>, dim3((4 * n + 63) / 64), dim3(64), 0, 0, a, b, k, out, oc, n);
    return (int)finish();
  } else {
    return (int)hipErrorInvalidValue;
  }
}

}  // namespace

extern "C" int pzk_probe_fr(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  if (bad_count(n) || op < 0 || op >= PFR_N_OPS || !a || !out) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = 32 * (size_t)n;
  DBuf da, db, dout;
  PROBE_TRY(da.up(a, bytes));
  if (b) PROBE_TRY(db.up(b, bytes));
  PROBE_TRY(dout.up(nullptr, bytes));
  const int e = run_fr(op, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>(), n);
  if (e) return e;
  return (int)dout.down(out, bytes);
}

extern "C" int pzk_probe_fr_batch_inv(const uint32_t* x, uint32_t* out, int n, int m) {
  if (bad_count(n) || m < 1 || m > 8 || !x || !out) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = 32 * (size_t)n * m;
  DBuf dx, dout;
  PROBE_TRY(dx.up(x, bytes));
  PROBE_TRY(dout.up(nullptr, bytes));
  hipLaunchKernelGGL(k_probe_fr_batch_inv, dim3((n + 63) / 64), dim3(64), 0, 0, dx.as<uint32_t>(), dout.as<uint32_t>(), n, m);
  PROBE_TRY(finish());
  return (int)dout.down(out, bytes);
}

extern "C" int pzk_probe_fq(int op, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out,
                            uint32_t* out_canon, int n) {
  if (bad_count(n) || op < 0 || op >= PFQ_N_OPS || !a || !out) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = 32 * (size_t)n;
  DBuf da, db, dk, dout, dcan;
  PROBE_TRY(da.up(a, bytes));
  if (b) PROBE_TRY(db.up(b, 3 * bytes));
  if (k) PROBE_TRY(dk.up(k, bytes));
  PROBE_TRY(dout.up(nullptr, bytes));
  if (out_canon) PROBE_TRY(dcan.up(nullptr, bytes));
  const int e = run_fq(op, da.as<uint32_t>(), db.as<uint32_t>(), dk.as<uint32_t>(), dout.as<uint32_t>(),
                       dcan.as<uint32_t>(), n);
  if (e) return e;
  PROBE_TRY(dout.down(out, bytes));
  if (out_canon) PROBE_TRY(dcan.down(out_canon, bytes));
  return 0;
}

extern "C" int pzk_probe_div64(int op, const uint64_t* u1, const uint64_t* u0, const uint64_t* v, uint64_t* q,
                               uint64_t* r, int n) {
  if (bad_count(n) || (op != PDIV_DIVLU && op != PDIV_PREINV) || !u1 || !u0 || !v || !q || !r)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = 8 * (size_t)n;
  DBuf d1, d0, dv, dq, dr;
  PROBE_TRY(d1.up(u1, bytes));
  PROBE_TRY(d0.up(u0, bytes));
  PROBE_TRY(dv.up(v, bytes));
  PROBE_TRY(dq.up(nullptr, bytes));
  PROBE_TRY(dr.up(nullptr, bytes));
  if (op == PDIV_DIVLU)
    hipLaunchKernelGGL(k_probe_div64<PDIV_DIVLU>, dim3((n + 63) / 64), dim3(64), 0, 0, d1.as<uint64_t>(),
                       d0.as<uint64_t>(), dv.as<uint64_t>(), dq.as<uint64_t>(), dr.as<uint64_t>(), n);
  else
    hipLaunchKernelGGL(k_probe_div64<PDIV_PREINV>, dim3((n + 63) / 64), dim3(64), 0, 0, d1.as<uint64_t>(),
                       d0.as<uint64_t>(), dv.as<uint64_t>(), dq.as<uint64_t>(), dr.as<uint64_t>(), n);
  PROBE_TRY(finish());
  PROBE_TRY(dq.down(q, bytes));
  return (int)dr.down(r, bytes);
}

extern "C" int pzk_probe_kd_div(const uint64_t* a, const int* na, int sa, const uint64_t* b, const int* nb, int sb,
                                uint64_t* q, uint64_t* r, int n) {
  if (bad_count(n) || sa < 2 || sb < 2 || sa > 4096 || sb > sa || !a || !na || !b || !nb || !q || !r)
    return (int)hipErrorInvalidValue;
  for (int c = 0; c < n; c++) {  // kd_div's domain: 2 <= nb <= na, a nonzero top word of b, everything inside the rows
    if (nb[c] < 2 || nb[c] > sb || na[c] < nb[c] || na[c] > sa || b[(size_t)c * sb + nb[c] - 1] == 0)
      return (int)hipErrorInvalidValue;
  }
  if (n == 0) return 0;
  DBuf da, dna, db, dnb, dq, dr, dun, dvn;
  PROBE_TRY(da.up(a, 8 * (size_t)n * sa));
  PROBE_TRY(dna.up(na, sizeof(int) * (size_t)n));
  PROBE_TRY(db.up(b, 8 * (size_t)n * sb));
  PROBE_TRY(dnb.up(nb, sizeof(int) * (size_t)n));
  PROBE_TRY(dq.up(nullptr, 8 * (size_t)n * sa));
  PROBE_TRY(dr.up(nullptr, 8 * (size_t)n * sb));
  PROBE_TRY(dun.up(nullptr, 8 * (size_t)n * (sa + 1)));
  PROBE_TRY(dvn.up(nullptr, 8 * (size_t)n * sb));
  hipLaunchKernelGGL(k_probe_kd_div, dim3((n + 63) / 64), dim3(64), 0, 0, da.as<uint64_t>(), dna.as<int>(), sa,
                     db.as<uint64_t>(), dnb.as<int>(), sb, dq.as<uint64_t>(), dr.as<uint64_t>(), dun.as<uint64_t>(),
                     dvn.as<uint64_t>(), n);
  PROBE_TRY(finish());
  PROBE_TRY(dq.down(q, 8 * (size_t)n * sa));
  return (int)dr.down(r, 8 * (size_t)n * sb);
}
