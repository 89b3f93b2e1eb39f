// libpzkprobe.so: test-only entry points that run the device arithmetic primitives (fr.hpp, fq.hpp, core_util.hpp,
// regcore.hpp, rsa_coop.hpp, ec_core.hpp) on host arrays of operands, one case per lane (per quad for fq). The
// library includes the product headers as they are and holds no arithmetic of its own; it is never linked into
// libpzkwit.so. Every entry point allocates, copies, launches, copies back and returns the HIP error code
// (hipErrorInvalidValue = 1 for a bad argument); nothing throws. tests/test_gpu_arith.py drives it.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PZK_PROBE_MAX_CASES 4096

// ---- Fr on one lane: 8 x u32 per element. a, b, out: n x 8 words (b may be NULL for unary ops).
enum {
  PFR_ADD = 0, PFR_SUB, PFR_REDUCE_ONCE, PFR_GEQ_P /* out[0] = 0 / 1 */, PFR_MUL, PFR_SQR, PFR_MUL_FAST, PFR_FROM_MONT,
  PFR_FROM_MONT_FAST, PFR_TO_MONT, PFR_TO_MONT_IN, PFR_INV, PFR_INV_FAST, PFR_INV_SW, PFR_INV_SW_FAST,
  PFR_FROM_I128 /* a[0..3] = lo, hi */, PFR_N_OPS
};
int pzk_probe_fr(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n);
// fr_batch_inv over m <= 8 elements per case: x, out: n x m x 8 words
int pzk_probe_fr_batch_inv(const uint32_t* x, uint32_t* out, int n, int m);

// ---- quad-spread Fr: one case per quad, 16 cases side by side in a wave. a, k: n x 8 words; b: n x 3 x 8 words
// (row r of case c at b[(3 c + r) * 8]). The products use b row 0. PFQ_DOTn: case c of 16-lane row rho gets
// k_c + sum_{r < n} a_{4 rho + r} * b_{c, r} (the first operands are the elements of the row's quads 0..2, by rword).
// out: n x 8 words (fq_gather of the result; PFQ_GEQ_P: out[0] = 0 / 1). out_canon (may be NULL): the result after
// two fq_canon (the chain's fq_canon2), for the ops whose result is not canonical.
enum {
  PFQ_MUL = 0, PFQ_MUL64, PFQ_MULQ, PFQ_DOT1, PFQ_DOT2, PFQ_DOT3, PFQ_CANON, PFQ_GEQ_P, PFQ_ADD_RAW, PFQ_N_OPS
};
int pzk_probe_fq(int op, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out, uint32_t* out_canon,
                 int n);

// ---- 128 / 64 division steps: op 0 = divlu, 1 = div_preinv (vinv from divlu(~v, ~0, v), as rsa_lane computes it)
enum { PDIV_DIVLU = 0, PDIV_PREINV = 1 };
int pzk_probe_div64(int op, const uint64_t* u1, const uint64_t* u0, const uint64_t* v, uint64_t* q, uint64_t* r, int n);
// kd_div: case c divides a[c * sa .. + na[c]) by b[c * sb .. + nb[c]); q: n x sa words (na - nb + 1 written), r: n x sb
int pzk_probe_kd_div(const uint64_t* a, const int* na, int sa, const uint64_t* b, const int* nb, int sb, uint64_t* q,
                     uint64_t* r, int n);

// ---- per curve cv = 0..3 (secp256r1, brainpoolP256r1, secp224r1, brainpoolP384r1)
enum { PEC_MUL = 0, PEC_ADD, PEC_SUB, PEC_TO, PEC_FROM, PEC_INV, PEC_N_OPS };
// field words NW and division words PWORDS of the curve
int pzk_probe_ec_nw(int cv);
int pzk_probe_ec_pwords(int cv);
// m_mul_inl / m_add / m_sub / m_to / m_from / m_inv of ModP (mod_n = 0) or ModN (1): a, b, out: n x NW words
int pzk_probe_ec_field(int cv, int mod_n, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int n);
// mp_divmod<PWORDS> by the curve's p (mod_n = 0) or n (1): a: n x 32 words, na[c] <= 31; q: n x 32, r: n x PWORDS
int pzk_probe_ec_divmod(int cv, int mod_n, const uint64_t* a, const int* na, uint64_t* q, uint64_t* r, int n);

// ---- the transforms of ntt.hpp: one forward or one inverse transform of batch x 2^k elements (8 words each, normal
// form, below p; converted to and from Montgomery form around the transform). forward: coefficient i at index
// bitrev_k(i) in, the evaluations at w_N^j in natural order out. inverse: evaluations in natural order in, coefficient
// i at index bitrev_k(i) out, times g^i when shift != 0 (g = w_2N). split: n_split pass sizes q summing to k, each in
// 1 .. r, or n_split = 0 for the default plan. on_device != 0: in and out are device pointers (they may be equal).
int pzk_probe_ntt(int inverse, int shift, int k, int batch, const int* split, int n_split, const uint32_t* in,
                  uint32_t* out, int on_device);
// the default plan for 2^k points: returns the number of passes (0: k out of range), their sizes in q[0 .. 24), and r
int pzk_probe_ntt_plan(int k, int* q, int* r);

#ifdef __cplusplus
}
#endif
