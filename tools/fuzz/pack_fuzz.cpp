// Host ASan/UBSan driver for the packed input rows (include/pzkwit.h): the layout queries, pzk_pack_inputs
// and pzk_unpack_inputs_host (passport-zk-circuits_amd/csrc/host_api.cpp). Reads records from stdin:
//   pzk_params (12 x i32), u32 n (rows), u32 seed, u8 mode
// mode 0: n rows over the packed domain (random bits, limbs, 32-byte strings) -> pack -> unpack: byte-identical;
// mode 1: the same rows with every third one pushed out of the domain (a bit element of 2, a bit element with a high
//         byte, a limb of 2^64): those rows must get status 1 and a zero packed row, the others must round-trip;
// mode 2: n packed rows of random bytes -> unpack -> pack: the packed rows again, with the pad bits and bytes zero.
// Every buffer is a heap block of exactly the size the API documents for n rows (n = 0: null pointers), so a read or
// write past it is a sanitizer report. Prints one line per record: "ok <row_bytes> <rows refused>" or "err <code>";
// a broken invariant prints "BAD <what>" and exits 2. Built by tools/fuzz/Makefile with -fsanitize=address,undefined
// (-fno-sanitize-recover): any report aborts the run (tests/test_pack_fuzz.py).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pzkwit.h"
#include "../../passport-zk-circuits_amd/csrc/host_api.hpp"

namespace pzk {
static thread_local std::string g_msg;
int api_fail(int code, const std::string& msg) { g_msg = msg; return code; }
}  // namespace pzk

static bool read_n(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static uint64_t g_rng;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int bad(const char* what) {
  printf("BAD %s\n", what);
  return 2;
}

int main() {
  pzk_params prm;
  while (read_n(&prm, sizeof prm)) {
    uint32_t n, seed;
    uint8_t mode;
    if (!read_n(&n, 4) || !read_n(&seed, 4) || !read_n(&mode, 1)) break;
    g_rng = seed;
    pzk_info info;
    uint64_t row_bytes = 0;
    int rc = pzk_layout_query(&prm, &info, nullptr);
    if (!rc) rc = pzk_packed_layout(&prm, &row_bytes);
    if (rc) { printf("err %d\n", rc); fflush(stdout); continue; }
    // the group table through the C ABI: tiles the packed row in order, 16-byte aligned
    struct G { uint32_t kind; uint64_t off, len, elems, el0; };
    std::vector<G> groups;
    uint64_t el = 0, end = 0;
    for (uint32_t i = 0; i < info.n_input_groups; i++) {
      G g{};
      if (pzk_packed_group(&prm, i, &g.kind, &g.off, &g.len)) return bad("group query");
      if (g.off % 16 || g.off < end || g.kind > PZK_INPUT_FIELD) return bad("group offset");
      g.elems = g.kind == PZK_INPUT_BIT ? 0 : g.kind == PZK_INPUT_LIMB ? g.len / 8 : g.len / 32;
      groups.push_back(g);
      end = g.off + g.len;
    }
    if (pzk_packed_group(&prm, info.n_input_groups, nullptr, nullptr, nullptr) != PZK_E_ARG) return bad("group past the end");
    if (row_bytes % 16 || end > row_bytes || row_bytes - end >= 16) return bad("row size");
    // a BIT group's element count is not in its byte length: the groups tile [0, n_inputs), so with the layout's own
    // table (the same build) as the element reference
    pzk::Layout L;
    std::string why;
    if (!pzk::build_layout(prm, L, why) || L.inputs.size() != groups.size()) return bad("layout");
    for (size_t i = 0; i < groups.size(); i++) {
      if (groups[i].kind != PZK_INPUT_BIT && groups[i].elems != L.inputs[i].length) return bad("group length");
      if (groups[i].kind == PZK_INPUT_BIT && groups[i].len != (L.inputs[i].length + 7) / 8) return bad("bit group length");
      groups[i].elems = L.inputs[i].length;
      groups[i].el0 = el;
      el += groups[i].elems;
    }
    if (el != info.n_inputs) return bad("groups do not tile the inputs");
    const size_t in_row = 32 * (size_t)info.n_inputs;
    std::unique_ptr<uint8_t[]> rows(n ? new uint8_t[in_row * n] : nullptr), back(n ? new uint8_t[in_row * n] : nullptr),
        packed(n ? new uint8_t[row_bytes * n] : nullptr), packed2(n ? new uint8_t[row_bytes * n] : nullptr);
    std::unique_ptr<int32_t[]> status(n ? new int32_t[n] : nullptr);
    uint32_t refused = 0;
    if (mode == 2) {
      for (size_t k = 0; k < row_bytes * n; k++) packed[k] = (uint8_t)rnd();
      if (pzk_unpack_inputs_host(&prm, packed.get(), n, rows.get())) return bad("unpack");
      if (pzk_pack_inputs(&prm, rows.get(), n, packed2.get(), status.get(), 1 + (int)(seed % 3))) return bad("pack");
      for (uint32_t r = 0; r < n; r++) {
        if (status[r]) return bad("an unpacked row did not pack");
        std::vector<uint8_t> want(row_bytes, 0);  // the random row without its pad bits / bytes
        const uint8_t* src = packed.get() + row_bytes * r;
        for (const G& g : groups) {
          memcpy(want.data() + g.off, src + g.off, g.len);
          if (g.kind == PZK_INPUT_BIT && g.elems % 8) want[g.off + g.len - 1] &= (uint8_t)(0xFF00 >> (g.elems % 8));
        }
        if (memcmp(want.data(), packed2.get() + row_bytes * r, row_bytes)) return bad("pack(unpack(x)) != x");
      }
    } else {
      if (n) memset(rows.get(), 0, in_row * n);
      std::vector<uint8_t> out_of_domain(n, 0);
      for (uint32_t r = 0; r < n; r++) {
        uint8_t* row = rows.get() + in_row * r;
        for (const G& g : groups)
          for (uint64_t j = 0; j < g.elems; j++) {
            uint8_t* e = row + 32 * (g.el0 + j);
            if (g.kind == PZK_INPUT_BIT) e[0] = (uint8_t)(rnd() & 1);
            else for (int k = 0; k < (g.kind == PZK_INPUT_LIMB ? 8 : 32); k++) e[k] = (uint8_t)rnd();
          }
        if (mode == 1 && r % 3 == 1) {  // one element of a BIT or LIMB group out of the domain, if the row has one
          std::vector<const G*> narrow;
          for (const G& g : groups)
            if (g.kind != PZK_INPUT_FIELD && g.elems) narrow.push_back(&g);
          if (!narrow.empty()) {
            const G& g = *narrow[rnd() % narrow.size()];
            uint8_t* e = row + 32 * (g.el0 + rnd() % g.elems);
            if (g.kind == PZK_INPUT_LIMB) e[8 + rnd() % 24] = 1 + (uint8_t)(rnd() % 255);
            else if (rnd() & 1) e[0] = 2 + (uint8_t)(rnd() % 254);
            else e[1 + rnd() % 31] = 1 + (uint8_t)(rnd() % 255);
            out_of_domain[r] = 1;
          }
        }
      }
      if (pzk_pack_inputs(&prm, rows.get(), n, packed.get(), status.get(), 1 + (int)(seed % 3))) return bad("pack");
      if (pzk_unpack_inputs_host(&prm, packed.get(), n, back.get())) return bad("unpack");
      for (uint32_t r = 0; r < n; r++) {
        if (status[r] != out_of_domain[r]) return bad("status");
        if (out_of_domain[r]) {
          refused++;
          for (size_t k = 0; k < row_bytes; k++)
            if (packed[row_bytes * r + k]) return bad("a refused row's packed row is not zero");
        } else if (memcmp(rows.get() + in_row * r, back.get() + in_row * r, in_row)) {
          return bad("unpack(pack(row)) != row");
        }
      }
    }
    // null buffers with rows to process are an argument error, not a crash
    if (pzk_pack_inputs(&prm, nullptr, 1, nullptr, nullptr, 1) != PZK_E_ARG) return bad("null rows accepted");
    if (pzk_unpack_inputs_host(&prm, nullptr, 1, nullptr) != PZK_E_ARG) return bad("null packed rows accepted");
    printf("ok %llu %u\n", (unsigned long long)row_bytes, refused);
    fflush(stdout);
  }
  return 0;
}
