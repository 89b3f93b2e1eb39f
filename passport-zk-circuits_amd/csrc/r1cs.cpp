// circom's binary .r1cs format -> the device program of r1cs.hpp, and the kernels' host twin (pzk_r1cs_eval_host).
// Host only: no device code, no HIP runtime call (tools/fuzz builds this unit with the host sanitizers).
#include <string.h>

#include <algorithm>
#include <array>
#include <map>

#include "../../include/pzkwit.h"
#include "host_api.hpp"
#include "r1cs.hpp"
#define PZK_NTT_HOST_ONLY
#include "ntt.hpp"

namespace pzk {

namespace {

// ---- BN254 scalar field on the host: four 64-bit words, little-endian, normal form. Not a hot path.
typedef std::array<uint64_t, 4> F4;
const F4 FP = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

bool f_geq(const F4& a, const F4& b) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}
// a - b, returns the borrow
uint64_t f_sub_raw(F4& a, const F4& b) {
  unsigned __int128 br = 0;
  for (int i = 0; i < 4; i++) {
    const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - br;
    a[i] = (uint64_t)d;
    br = (d >> 64) & 1;
  }
  return (uint64_t)br;
}
// a, b < p
F4 f_add(const F4& a, const F4& b) {
  F4 r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)a[i] + b[i];
    r[i] = (uint64_t)c;
    c >>= 64;
  }
  if (f_geq(r, FP)) f_sub_raw(r, FP);  // p < 2^254: no carry out of the sum
  return r;
}
F4 f_sub(const F4& a, const F4& b) {
  F4 r = a;
  if (f_sub_raw(r, b)) {
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (unsigned __int128)r[i] + FP[i];
      r[i] = (uint64_t)c;
      c >>= 64;
    }
  }
  return r;
}
// x mod p for n little-endian words, by shift-and-subtract from the top bit
F4 f_reduce(const uint64_t* x, int n) {
  F4 r = {0, 0, 0, 0};
  for (int bit = 64 * n - 1; bit >= 0; bit--) {
    // r = 2 r + bit (r < p < 2^254: no overflow)
    for (int i = 3; i > 0; i--) r[i] = (r[i] << 1) | (r[i - 1] >> 63);
    r[0] = (r[0] << 1) | ((x[bit >> 6] >> (bit & 63)) & 1);
    if (f_geq(r, FP)) f_sub_raw(r, FP);
  }
  return r;
}
// a * b mod p for any 256-bit a, b
F4 f_mul(const F4& a, const F4& b) {
  uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (unsigned __int128)a[i] * b[j] + t[i + j];
      t[i + j] = (uint64_t)c;
      c >>= 64;
    }
    t[i + 4] = (uint64_t)c;
  }
  return f_reduce(t, 8);
}
F4 f_residue(const F4& w) { return f_geq(w, FP) ? f_reduce(w.data(), 4) : w; }
bool f_is_zero(const F4& a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }
F4 f_load(const uint8_t* p) {
  F4 r;
  for (int i = 0; i < 4; i++) {
    uint64_t v = 0;
    for (int k = 7; k >= 0; k--) v = (v << 8) | p[8 * i + k];
    r[i] = v;
  }
  return r;
}

void f_store(uint8_t* p, const F4& a) {
  for (int i = 0; i < 4; i++)
    for (int k = 0; k < 8; k++) p[8 * i + k] = (uint8_t)(a[i] >> (8 * k));
}

// ---- Montgomery form (R = 2^256) for the quotient's transforms: f_mul's bitwise reduction is too slow for them
const F4 F_R2 = {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull};  // R^2 mod p
const F4 F_ROOT28 = {0x9bd61b6e725b19f0ull, 0x402d111e41112ed4ull, 0x00e0a7eb8ef62abcull, 0x2a3c09f0a58a7e85ull};  // 5^((p - 1) / 2^28)
uint64_t f_pinv() {  // -p^-1 mod 2^64, by Newton's iteration
  uint64_t inv = 1;
  for (int i = 0; i < 6; i++) inv *= 2 - FP[0] * inv;
  return 0 - inv;
}
// a b / R mod p for a, b < p (operand-scanning CIOS; p < 2^254: the running sum stays below 2 p)
F4 f_mmul(const F4& a, const F4& b) {
  static const uint64_t pinv = f_pinv();
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (unsigned __int128)a[j] * b[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * pinv;
    c = ((unsigned __int128)m * FP[0] + t[0]) >> 64;
    for (int j = 1; j < 4; j++) {
      c += (unsigned __int128)m * FP[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  F4 r = {t[0], t[1], t[2], t[3]};
  if (t[4] || f_geq(r, FP)) f_sub_raw(r, FP);
  return r;
}
F4 f_to_mont(const F4& a) { return f_mmul(a, F_R2); }

// ---- bounded little-endian reader: nothing is read, and no size taken from the file is used, before it has been
// compared with the bytes that remain
struct Reader {
  const uint8_t* p;
  size_t pos, end;
  size_t left() const { return end - pos; }
  bool u32(uint32_t& v) {
    if (left() < 4) return false;
    v = (uint32_t)p[pos] | (uint32_t)p[pos + 1] << 8 | (uint32_t)p[pos + 2] << 16 | (uint32_t)p[pos + 3] << 24;
    pos += 4;
    return true;
  }
  bool u64(uint64_t& v) {
    uint32_t lo, hi;
    if (left() < 8 || !u32(lo) || !u32(hi)) return false;
    v = (uint64_t)hi << 32 | lo;
    return true;
  }
};

struct RawTerm { uint32_t wire; F4 c; };

}  // namespace

bool r1cs_parse(const uint8_t* bytes, size_t len, R1csProgram& out, std::string& why) {
  out = R1csProgram();
  Reader rd{bytes, 0, len};
  uint32_t version, n_sections;
  if (len < 12 || memcmp(bytes, "r1cs", 4) != 0) { why = "r1cs: wrong magic"; return false; }
  rd.pos = 4;
  rd.u32(version);
  rd.u32(n_sections);
  if (version != 1) { why = "r1cs: version " + std::to_string(version) + " (expected 1)"; return false; }
  // pass 1: the bounds of every section
  size_t hdr_at = 0, hdr_size = 0, con_at = 0, con_size = 0;
  bool has_hdr = false, has_con = false;
  std::vector<uint64_t> label_sizes;
  for (uint32_t s = 0; s < n_sections; s++) {
    uint32_t type;
    uint64_t size;
    if (!rd.u32(type) || !rd.u64(size)) { why = "r1cs: section " + std::to_string(s) + ": header runs past the buffer"; return false; }
    if (size > rd.left()) {
      why = "r1cs: section " + std::to_string(s) + " (type " + std::to_string(type) + "): size " + std::to_string(size) +
            " runs past the buffer (" + std::to_string(rd.left()) + " bytes left)";
      return false;
    }
    if (type == 1) {
      if (has_hdr) { why = "r1cs: duplicate header section"; return false; }
      has_hdr = true; hdr_at = rd.pos; hdr_size = (size_t)size;
    } else if (type == 2) {
      if (has_con) { why = "r1cs: duplicate constraint section"; return false; }
      has_con = true; con_at = rd.pos; con_size = (size_t)size;
    } else if (type == 3) {
      label_sizes.push_back(size);
    }  // custom gates (4, 5) and unknown types: skipped by size
    rd.pos += (size_t)size;
  }
  if (!has_hdr) { why = "r1cs: no header section (type 1)"; return false; }
  if (!has_con) { why = "r1cs: no constraint section (type 2)"; return false; }
  // the header
  Reader h{bytes, hdr_at, hdr_at + hdr_size};
  uint32_t field_size, m;
  if (!h.u32(field_size)) { why = "r1cs: header section too short"; return false; }
  if (field_size != 32) { why = "r1cs: fieldSize " + std::to_string(field_size) + " (expected 32)"; return false; }
  if (h.left() != 32 + 4 * 4 + 8 + 4) { why = "r1cs: header section is " + std::to_string(hdr_size) + " bytes (expected 64)"; return false; }
  if (f_load(bytes + h.pos) != FP) { why = "r1cs: the prime is not BN254's r"; return false; }
  h.pos += 32;
  h.u32(out.n_wires); h.u32(out.n_pub_out); h.u32(out.n_pub_in); h.u32(out.n_prv_in); h.u64(out.n_labels); h.u32(m);
  if (out.n_wires == 0) { why = "r1cs: nWires = 0"; return false; }
  if (m >> 31) { why = "r1cs: mConstraints " + std::to_string(m) + " >= 2^31"; return false; }
  for (uint64_t sz : label_sizes)
    if (sz != 8ull * out.n_wires) {
      why = "r1cs: wire-to-label section is " + std::to_string(sz) + " bytes (expected 8 * nWires = " +
            std::to_string(8ull * out.n_wires) + ")";
      return false;
    }
  // a constraint is at least three term counts
  if ((uint64_t)m * 12 > con_size) {
    why = "r1cs: mConstraints " + std::to_string(m) + " runs past the constraint section (" + std::to_string(con_size) + " bytes)";
    return false;
  }
  out.n_constraints = m;
  // pass 2: the constraints
  Reader c{bytes, con_at, con_at + con_size};
  std::map<F4, uint32_t> coeff_index;
  F4 one = {1, 0, 0, 0}, minus_one = FP;
  minus_one[0] -= 1;
  for (const F4& v : {one, minus_one}) {
    coeff_index.emplace(v, (uint32_t)coeff_index.size());
    out.coeffs.insert(out.coeffs.end(), v.begin(), v.end());
  }
  out.lc_off.reserve(3 * (size_t)m + 1);
  out.lc_off.push_back(0);
  std::vector<RawTerm> lc;
  R1csChunk cur{0, 0};
  uint32_t cur_terms = 0;
  auto close_chunk = [&]() {
    if (cur.count) out.chunks.push_back(cur);
    cur = R1csChunk{0, 0};
    cur_terms = 0;
  };
  for (uint32_t k = 0; k < m; k++) {
    uint32_t longest = 0, total = 0;
    for (int j = 0; j < 3; j++) {
      uint32_t nt;
      if (!c.u32(nt)) { why = "r1cs: constraint " + std::to_string(k) + " runs past the constraint section"; return false; }
      if (nt > c.left() / 36) {
        why = "r1cs: constraint " + std::to_string(k) + ": " + std::to_string(nt) + " terms run past the constraint section";
        return false;
      }
      lc.clear();
      for (uint32_t q = 0; q < nt; q++) {
        RawTerm t;
        c.u32(t.wire);
        t.c = f_load(bytes + c.pos);
        c.pos += 32;
        if (t.wire >= out.n_wires) {
          why = "r1cs: constraint " + std::to_string(k) + ": wire " + std::to_string(t.wire) + " >= nWires " + std::to_string(out.n_wires);
          return false;
        }
        if (f_geq(t.c, FP)) { why = "r1cs: constraint " + std::to_string(k) + ": a coefficient is >= p"; return false; }
        lc.push_back(t);
      }
      // wires ascending; a wire listed more than once: its coefficients add; a zero coefficient: no term
      std::stable_sort(lc.begin(), lc.end(), [](const RawTerm& x, const RawTerm& y) { return x.wire < y.wire; });
      uint32_t kept = 0;
      for (size_t q = 0; q < lc.size();) {
        F4 sum = lc[q].c;
        size_t e = q + 1;
        for (; e < lc.size() && lc[e].wire == lc[q].wire; e++) sum = f_add(sum, lc[e].c);
        if (!f_is_zero(sum)) {
          auto it = coeff_index.find(sum);
          if (it == coeff_index.end()) {
            it = coeff_index.emplace(sum, (uint32_t)coeff_index.size()).first;
            out.coeffs.insert(out.coeffs.end(), sum.begin(), sum.end());
          }
          if (out.terms.size() >= 0xFFFFFFFFull) { why = "r1cs: more than 2^32 - 1 terms"; return false; }
          out.terms.push_back(R1csTerm{lc[q].wire, it->second});
          kept++;
        }
        q = e;
      }
      out.lc_off.push_back((uint32_t)out.terms.size());
      longest = std::max(longest, kept);
      total += kept;
    }
    out.max_terms = std::max(out.max_terms, longest);
    if (longest > R1CS_LONG_T) {
      close_chunk();
      out.long_list.push_back(k);
    } else {
      if (cur.count == R1CS_CHUNK_C || cur_terms + total > R1CS_CHUNK_TERMS) close_chunk();
      if (cur.count == 0) cur.first = k;
      cur.count++;
      cur_terms += total;
    }
  }
  close_chunk();
  if (c.left() != 0) {
    why = "r1cs: " + std::to_string(c.left()) + " trailing bytes in the constraint section";
    return false;
  }
  return true;
}

void r1cs_eval_row(const R1csProgram& P, const uint8_t* row, int32_t& first_failed, uint32_t& n_failed) {
  first_failed = -1;
  n_failed = 0;
  for (uint32_t k = 0; k < P.n_constraints; k++) {
    F4 v[3];
    for (int j = 0; j < 3; j++) {
      F4 acc = {0, 0, 0, 0};
      for (uint32_t q = P.lc_off[3ull * k + j]; q < P.lc_off[3ull * k + j + 1]; q++) {
        const R1csTerm t = P.terms[q];
        const F4 w = f_load(row + 32ull * t.wire);
        if (t.coeff == 0) acc = f_add(acc, f_residue(w));
        else if (t.coeff == 1) acc = f_sub(acc, f_residue(w));
        else {
          F4 cf;
          memcpy(cf.data(), &P.coeffs[4ull * t.coeff], 32);
          acc = f_add(acc, f_mul(cf, w));
        }
      }
      v[j] = acc;
    }
    if (f_mul(v[0], v[1]) != v[2]) {
      if (first_failed < 0) first_failed = (int32_t)k;
      n_failed++;
    }
  }
}

bool r1cs_quotient_domain(const R1csProgram& P, uint64_t& m, int& k) {
  m = (uint64_t)P.n_constraints + P.n_pub_out + P.n_pub_in + 1;
  k = 0;
  while (k < 40 && (1ull << k) < m) k++;
  return k >= 1 && k <= NTT_MAX_K;
}

namespace {

// LC j of constraint k on a row, normal form (r1cs_eval_row's sum)
F4 lc_value(const R1csProgram& P, const uint8_t* row, uint32_t k, int j) {
  F4 acc = {0, 0, 0, 0};
  for (uint32_t q = P.lc_off[3ull * k + j]; q < P.lc_off[3ull * k + j + 1]; q++) {
    const R1csTerm t = P.terms[q];
    const F4 w = f_load(row + 32ull * t.wire);
    if (t.coeff == 0) acc = f_add(acc, f_residue(w));
    else if (t.coeff == 1) acc = f_sub(acc, f_residue(w));
    else {
      F4 cf;
      memcpy(cf.data(), &P.coeffs[4ull * t.coeff], 32);
      acc = f_add(acc, f_mul(cf, w));
    }
  }
  return acc;
}

uint32_t bitrev(uint32_t i, int k) {
  uint32_t r = 0;
  for (int b = 0; b < k; b++) r |= ((i >> b) & 1u) << (k - 1 - b);
  return r;
}

// evaluations on <w_N> -> evaluations on g <w_N>, in place, Montgomery form. W[j] = w_N^j, j < N / 2; g = w_2N;
// n_inv = 1 / N. Decimation in frequency with the inverse roots (w^-e = -W[N / 2 - e]) leaves the coefficients
// bit-reversed, the shift multiplies coefficient i at its place, decimation in time takes them back to natural order.
void to_coset(std::vector<F4>& x, int k, const std::vector<F4>& W, const F4& g, const F4& n_inv) {
  const size_t n = (size_t)1 << k;
  const F4 zero = {0, 0, 0, 0};
  for (int s = k - 1; s >= 0; s--) {
    const size_t half = (size_t)1 << s;
    for (size_t i = 0; i < n; i += 2 * half)
      for (size_t jl = 0; jl < half; jl++) {
        const size_t e = jl << (k - 1 - s);
        const F4 u = x[i + jl], v = x[i + jl + half], d = f_sub(u, v);
        x[i + jl] = f_add(u, v);
        x[i + jl + half] = e ? f_mmul(d, f_sub(zero, W[n / 2 - e])) : d;
      }
  }
  F4 gi = n_inv;
  for (size_t i = 0; i < n; i++) {
    F4& e = x[bitrev((uint32_t)i, k)];
    e = f_mmul(e, gi);
    gi = f_mmul(gi, g);
  }
  for (int s = 0; s < k; s++) {
    const size_t half = (size_t)1 << s;
    for (size_t i = 0; i < n; i += 2 * half)
      for (size_t jl = 0; jl < half; jl++) {
        const size_t e = jl << (k - 1 - s);
        const F4 u = x[i + jl], v = e ? f_mmul(x[i + jl + half], W[e]) : x[i + jl + half];
        x[i + jl] = f_add(u, v);
        x[i + jl + half] = f_sub(u, v);
      }
  }
}

}  // namespace

void r1cs_quotient_row(const R1csProgram& P, int k, const uint8_t* row, uint8_t* h) {
  const size_t n = (size_t)1 << k;
  const uint32_t nc = P.n_constraints, n_pub = P.n_pub_out + P.n_pub_in;
  const F4 zero = {0, 0, 0, 0}, one = {1, 0, 0, 0};
  std::vector<F4> a(n, zero), b(n, zero), c(n, zero);
  for (uint32_t i = 0; i < nc; i++) {
    a[i] = f_to_mont(lc_value(P, row, i, 0));
    b[i] = f_to_mont(lc_value(P, row, i, 1));
    c[i] = f_mmul(a[i], b[i]);
  }
  for (uint32_t s = 0; s <= n_pub; s++) a[nc + s] = f_to_mont(f_residue(f_load(row + 32ull * s)));
  // g = w_2N = w_(2^28)^(2^(27 - k)), w_N = g^2, 1 / N = ((p + 1) / 2)^k
  F4 g = f_to_mont(F_ROOT28);
  for (int i = 0; i < 27 - k; i++) g = f_mmul(g, g);
  const F4 w = f_mmul(g, g);
  std::vector<F4> W(n / 2);
  W[0] = f_to_mont(one);
  for (size_t j = 1; j < n / 2; j++) W[j] = f_mmul(W[j - 1], w);
  F4 half = FP;  // (p + 1) / 2 = (p >> 1) + 1, p odd
  for (int i = 0; i < 4; i++) half[i] = (half[i] >> 1) | (i < 3 ? half[i + 1] << 63 : 0);
  half[0] += 1;  // no carry: the low word of p >> 1 ends in ...000
  const F4 half_m = f_to_mont(half);
  F4 n_inv = f_to_mont(one);
  for (int i = 0; i < k; i++) n_inv = f_mmul(n_inv, half_m);
  to_coset(a, k, W, g, n_inv);
  to_coset(b, k, W, g, n_inv);
  to_coset(c, k, W, g, n_inv);
  for (size_t j = 0; j < n; j++) f_store(h + 32 * j, f_mmul(f_sub(f_mmul(a[j], b[j]), c[j]), one));
}

}  // namespace pzk

using namespace pzk;

extern "C" {

static int r1cs_load_impl(const uint8_t* bytes, size_t len, pzk_r1cs** out) {
  if (!out) return api_fail(PZK_E_ARG, "null argument");
  *out = nullptr;
  if (!bytes) return api_fail(PZK_E_ARG, "null argument");
  pzk_r1cs* r = new pzk_r1cs();
  std::string why;
  bool ok;
  try {
    ok = r1cs_parse(bytes, len, r->prog, why);
  } catch (...) {
    delete r;
    throw;  // guarded(): bad_alloc -> PZK_E_NOMEM
  }
  if (!ok) { delete r; return api_fail(PZK_E_ARG, why); }
  *out = r;
  return 0;
}

static int r1cs_get_info_impl(const pzk_r1cs* r, pzk_r1cs_info* info) {
  if (!r || !info) return api_fail(PZK_E_ARG, "null argument");
  const R1csProgram& P = r->prog;
  memset(info, 0, sizeof *info);
  info->n_wires = P.n_wires;
  info->n_pub_out = P.n_pub_out;
  info->n_pub_in = P.n_pub_in;
  info->n_prv_in = P.n_prv_in;
  info->n_labels = P.n_labels;
  info->n_constraints = P.n_constraints;
  info->n_long = (uint32_t)P.long_list.size();
  info->n_terms = P.terms.size();
  info->n_coeffs = (uint32_t)(P.coeffs.size() / 4);
  info->max_terms = P.max_terms;
  return 0;
}

static int r1cs_eval_host_impl(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride,
                               int32_t* first_failed, uint32_t* n_failed) {
  if (!r) return api_fail(PZK_E_ARG, "null argument");
  if (batch == 0) return 0;
  if (!h_wtns || !first_failed) return api_fail(PZK_E_ARG, "null argument");
  if (stride < 32ull * r->prog.n_wires || stride % 16) return api_fail(PZK_E_ARG, "bad witness stride");
  for (size_t i = 0; i < batch; i++) {
    uint32_t n;
    r1cs_eval_row(r->prog, h_wtns + stride * i, first_failed[i], n);
    if (n_failed) n_failed[i] = n;
  }
  return 0;
}

static int r1cs_quotient_info_impl(const pzk_r1cs* r, pzk_quotient_info* info) {
  if (!r || !info) return api_fail(PZK_E_ARG, "null argument");
  uint64_t m;
  int k;
  if (!r1cs_quotient_domain(r->prog, m, k))
    return api_fail(PZK_E_ARG, "quotient: " + std::to_string(m) + " rows: the domain 2^k must have 1 <= k <= 24");
  memset(info, 0, sizeof *info);
  info->log2_n = (uint32_t)k;
  info->tile = QUOT_TILE;
  info->n = 1ull << k;
  info->n_rows = m;
  info->scratch_bytes = 2ull * QUOT_TILE * (32ull << k) + ntt_table_bytes(k);
  return 0;
}

static int r1cs_quotient_host_impl(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h,
                                   size_t h_stride) {
  if (!r) return api_fail(PZK_E_ARG, "null argument");
  if (batch == 0) return 0;
  if (!h_wtns || !h) return api_fail(PZK_E_ARG, "null argument");
  uint64_t m;
  int k;
  if (!r1cs_quotient_domain(r->prog, m, k))
    return api_fail(PZK_E_ARG, "quotient: " + std::to_string(m) + " rows: the domain 2^k must have 1 <= k <= 24");
  if ((uint64_t)r->prog.n_pub_out + r->prog.n_pub_in >= r->prog.n_wires)
    return api_fail(PZK_E_ARG, "quotient: the header counts more public wires than wires");
  if (stride < 32ull * r->prog.n_wires || stride % 16) return api_fail(PZK_E_ARG, "bad witness stride");
  if (h_stride < (32ull << k) || h_stride % 16) return api_fail(PZK_E_ARG, "bad h stride");
  for (size_t i = 0; i < batch; i++) r1cs_quotient_row(r->prog, k, h_wtns + stride * i, h + h_stride * i);
  return 0;
}

int pzk_r1cs_quotient_info(const pzk_r1cs* r, pzk_quotient_info* info) {
  return guarded([&] { return r1cs_quotient_info_impl(r, info); });
}

int pzk_r1cs_quotient_host(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h,
                           size_t h_stride) {
  return guarded([&] { return r1cs_quotient_host_impl(r, h_wtns, batch, stride, h, h_stride); });
}

int pzk_r1cs_load(const uint8_t* bytes, size_t len, pzk_r1cs** out) {
  return guarded([&] { return r1cs_load_impl(bytes, len, out); });
}

void pzk_r1cs_destroy(pzk_r1cs* r) {
  if (!r) return;
  if (r->dev_free) r->dev_free(r);
  delete r;
}

int pzk_r1cs_get_info(const pzk_r1cs* r, pzk_r1cs_info* info) {
  return guarded([&] { return r1cs_get_info_impl(r, info); });
}

int pzk_r1cs_eval_host(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, int32_t* first_failed,
                       uint32_t* n_failed) {
  return guarded([&] { return r1cs_eval_host_impl(r, h_wtns, batch, stride, first_failed, n_failed); });
}

}  // extern "C"
