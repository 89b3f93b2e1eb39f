// Probe kernels for one curve's Montgomery fields and long division (ec_core.hpp). Compiled once per curve the way
// kernels_ec.hip is: this file for PZK_EC_CURVE 0, probe_ec_bp.hip / probe_ec_p224.hip / probe_ec_bp384.hip include
// it with PZK_EC_CURVE 1 / 2 / 3. The curve-0 unit also defines the public entry points, which dispatch on cv.
#include <hip/hip_runtime.h>

#include "../ec_core.hpp"
#include "probe_util.hpp"

namespace pzk {
inline namespace PZK_EC_NS {
using namespace pzkprobe;

template <class M, int OP>
__global__ void __launch_bounds__(64) k_probe_ec_field(const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  eW x, y, r;
  for (int i = 0; i < NW; i++) { x.v[i] = a[NW * c + i]; y.v[i] = b ? b[NW * c + i] : 0u; }
  if constexpr (OP == PEC_MUL) r = m_mul_inl<M>(x, y);
  else if constexpr (OP == PEC_ADD) r = m_add<M>(x, y);
  else if constexpr (OP == PEC_SUB) r = m_sub<M>(x, y);
  else if constexpr (OP == PEC_TO) r = m_to<M>(x);
  else if constexpr (OP == PEC_FROM) r = m_from<M>(x);
  else r = m_inv<M>(x);
  for (int i = 0; i < NW; i++) out[NW * c + i] = r.v[i];
}

// a: 32 words per case (na[c] <= 31 used); q: 32 words per case, zeroed by the host; r: PWORDS per case
__global__ void __launch_bounds__(64) k_probe_ec_divmod(int mod_n, const uint64_t* a, const int* na, uint64_t* q,
                                                        uint64_t* r, int n) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  uint64_t aw[32], qw[32], rw[PWORDS], dw[PWORDS];
  for (int i = 0; i < 32; i++) { aw[i] = a[32 * (size_t)c + i]; qw[i] = 0; }
  const_words(mod_n ? EC_N : EC_P, dw);  // the divisor as div_signed / divmod_n form it
  mp_divmod<PWORDS>(aw, na[c], dw, qw, rw);
  for (int i = 0; i < 32; i++) q[32 * (size_t)c + i] = qw[i];
  for (int i = 0; i < PWORDS; i++) r[PWORDS * (size_t)c + i] = rw[i];
}

template <class M, int OP = 0>
int probe_field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  if constexpr (OP < PEC_N_OPS) {
    if (op != OP) return probe_field_op<M, OP + 1>(op, a, b, out, n);
    hipLaunchKernelGGL((k_probe_ec_field<M, OP>), dim3((n + 63) / 64), dim3(64), 0, 0, a, b, out, n);
    return (int)finish();
  } else {
    return (int)hipErrorInvalidValue;
  }
}

int probe_ec_nw_cv() { return NW; }
int probe_ec_pwords_cv() { return PWORDS; }

int probe_ec_field_cv(int mod_n, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  if (bad_count(n) || op < 0 || op >= PEC_N_OPS || !a || !out) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const size_t bytes = 4 * (size_t)NW * n;
  DBuf da, db, dout;
  PROBE_TRY(da.up(a, bytes));
  if (b) PROBE_TRY(db.up(b, bytes));
  PROBE_TRY(dout.up(nullptr, bytes));
  const int e = mod_n ? probe_field_op<ModN>(op, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>(), n)
                      : probe_field_op<ModP>(op, da.as<uint32_t>(), db.as<uint32_t>(), dout.as<uint32_t>(), n);
  if (e) return e;
  return (int)dout.down(out, bytes);
}

int probe_ec_divmod_cv(int mod_n, const uint64_t* a, const int* na, uint64_t* q, uint64_t* r, int n) {
  if (bad_count(n) || !a || !na || !q || !r) return (int)hipErrorInvalidValue;
  for (int c = 0; c < n; c++)
    if (na[c] < PWORDS || na[c] > 31) return (int)hipErrorInvalidValue;  // mp_divmod's u[32] holds na + 1 words
  if (n == 0) return 0;
  DBuf da, dna, dq, dr;
  PROBE_TRY(da.up(a, 8 * 32 * (size_t)n));
  PROBE_TRY(dna.up(na, sizeof(int) * (size_t)n));
  PROBE_TRY(dq.up(nullptr, 8 * 32 * (size_t)n));
  PROBE_TRY(dr.up(nullptr, 8 * (size_t)PWORDS * n));
  hipLaunchKernelGGL(k_probe_ec_divmod, dim3((n + 63) / 64), dim3(64), 0, 0, mod_n, da.as<uint64_t>(), dna.as<int>(),
                     dq.as<uint64_t>(), dr.as<uint64_t>(), n);
  PROBE_TRY(finish());
  PROBE_TRY(dq.down(q, 8 * 32 * (size_t)n));
  return (int)dr.down(r, 8 * (size_t)PWORDS * n);
}

}  // namespace PZK_EC_NS

#if PZK_EC_CURVE == 0
#define PZK_PROBE_DECL(ns)                                                                                 \
  namespace ns {                                                                                           \
  int probe_ec_nw_cv();                                                                                    \
  int probe_ec_pwords_cv();                                                                                \
  int probe_ec_field_cv(int mod_n, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n);    \
  int probe_ec_divmod_cv(int mod_n, const uint64_t* a, const int* na, uint64_t* q, uint64_t* r, int n);    \
  }
PZK_PROBE_DECL(ec_c1)
PZK_PROBE_DECL(ec_c2)
PZK_PROBE_DECL(ec_c3)
#undef PZK_PROBE_DECL
#define PZK_PROBE_DISPATCH(call, bad) \
  switch (cv) {                        \
    case 0: return ec_c0::call;        \
    case 1: return ec_c1::call;        \
    case 2: return ec_c2::call;        \
    case 3: return ec_c3::call;        \
    default: return bad;               \
  }
#endif
}  // namespace pzk

#if PZK_EC_CURVE == 0
using namespace pzk;
extern "C" int pzk_probe_ec_nw(int cv) { PZK_PROBE_DISPATCH(probe_ec_nw_cv(), -1) }
extern "C" int pzk_probe_ec_pwords(int cv) { PZK_PROBE_DISPATCH(probe_ec_pwords_cv(), -1) }
extern "C" int pzk_probe_ec_field(int cv, int mod_n, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n) {
  PZK_PROBE_DISPATCH(probe_ec_field_cv(mod_n, op, a, b, out, n), (int)hipErrorInvalidValue)
}
extern "C" int pzk_probe_ec_divmod(int cv, int mod_n, const uint64_t* a, const int* na, uint64_t* q, uint64_t* r, int n) {
  PZK_PROBE_DISPATCH(probe_ec_divmod_cv(mod_n, a, na, q, r, n), (int)hipErrorInvalidValue)
}
#undef PZK_PROBE_DISPATCH
#endif
