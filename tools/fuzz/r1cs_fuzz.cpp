// Host ASan/UBSan driver for the .r1cs loader and the kernels' host twin (include/pzkwit.h pzk_r1cs_*,
// passport-zk-circuits_amd/csrc/r1cs.cpp). Reads records from stdin:
//   u32 len, len bytes (a .r1cs file, or what a mutation left of one)
// and runs pzk_r1cs_load, pzk_r1cs_get_info, pzk_r1cs_eval_host on two all-zero witness rows (a system of more than
// 2^20 wires is loaded but not evaluated: its rows would be gigabytes), then pzk_r1cs_destroy. The file is a heap block
// of exactly len bytes and the rows one of exactly 2 x 32 x n_wires, so a read past either is a sanitizer report.
// Prints one line per record: "ok <n_wires> <n_constraints> <n_terms> <first_failed>" or "err <code>"; a broken
// invariant prints "BAD <what>" and exits 2. Built by tools/fuzz/Makefile with -fsanitize=address,undefined
// (-fno-sanitize-recover): any report aborts the run (tests/test_r1cs_fuzz.py).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/pzkwit.h"
#include "../../passport-zk-circuits_amd/csrc/host_api.hpp"

namespace pzk {
static thread_local std::string g_msg;
int api_fail(int code, const std::string& msg) { g_msg = msg; return code; }
}  // namespace pzk

static bool read_n(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static int bad(const char* what) {
  printf("BAD %s\n", what);
  return 2;
}

int main() {
  uint32_t len;
  while (read_n(&len, 4)) {
    if (len > (64u << 20)) return bad("record length");
    std::unique_ptr<uint8_t[]> file(new uint8_t[len ? len : 1]);
    if (!read_n(file.get(), len)) break;
    pzk_r1cs* r = nullptr;
    pzk::g_msg.clear();
    const int rc = pzk_r1cs_load(file.get(), len, &r);
    if (rc) {
      if (r) return bad("a handle with an error");
      if (rc != PZK_E_ARG && rc != PZK_E_NOMEM) return bad("error code");
      if (pzk::g_msg.empty()) return bad("no reason");
      printf("err %d\n", rc);
      fflush(stdout);
      continue;
    }
    pzk_r1cs_info info;
    if (pzk_r1cs_get_info(r, &info)) return bad("get_info");
    if (info.n_wires == 0 || info.n_constraints >> 31 || info.n_long > info.n_constraints || info.n_coeffs < 2 ||
        info.n_terms > len / 36 || info.max_terms > info.n_terms)
      return bad("info");
    int32_t first[2] = {7, 7};
    uint32_t cnt[2] = {7, 7};
    if (info.n_wires <= (1u << 20)) {
      const size_t stride = 32 * (size_t)info.n_wires;
      std::unique_ptr<uint8_t[]> rows(new uint8_t[2 * stride]);
      memset(rows.get(), 0, 2 * stride);
      if (pzk_r1cs_eval_host(r, rows.get(), 2, stride, first, cnt)) return bad("eval_host");
      // the zero row: every LC is 0, every constraint holds
      if (first[0] != -1 || first[1] != -1 || cnt[0] || cnt[1]) return bad("the zero witness violates a constraint");
      if (pzk_r1cs_eval_host(r, rows.get(), 1, stride - 16, first, cnt) != PZK_E_ARG) return bad("short stride accepted");
    }
    pzk_r1cs_destroy(r);
    printf("ok %u %u %llu %d\n", info.n_wires, info.n_constraints, (unsigned long long)info.n_terms, first[0]);
    fflush(stdout);
  }
  return 0;
}
