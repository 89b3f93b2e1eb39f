// Host ASan/UBSan driver for the quotient's host twin (include/pzkwit.h pzk_r1cs_quotient_host,
// passport-zk-circuits_amd/csrc/r1cs.cpp). Reads records from stdin:
//   u32 len, len bytes (a valid .r1cs file), u32 batch, u32 stride, batch x stride bytes of witness rows
// and runs pzk_r1cs_load, pzk_r1cs_quotient_info and pzk_r1cs_quotient_host. The file, the rows and the result are heap
// blocks of exactly len, batch x stride and batch x 32 N bytes, so a read or write past any of them is a sanitizer
// report. Writes per record to stdout: i32 return code, u32 log2 N, then the batch x 32 N result bytes (when the code
// is 0). A broken invariant prints "BAD <what>" to stderr and exits 2. Built by tools/fuzz/Makefile with
// -fsanitize=address,undefined (-fno-sanitize-recover): any report aborts the run (tests/test_quotient_host.py).
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
  fprintf(stderr, "BAD %s\n", what);
  return 2;
}

int main() {
  uint32_t len;
  while (read_n(&len, 4)) {
    if (len > (64u << 20)) return bad("record length");
    std::unique_ptr<uint8_t[]> file(new uint8_t[len ? len : 1]);
    uint32_t batch, stride;
    if (!read_n(file.get(), len) || !read_n(&batch, 4) || !read_n(&stride, 4)) return bad("truncated record");
    if (batch == 0 || batch > 64 || stride > (32u << 20)) return bad("record sizes");
    std::unique_ptr<uint8_t[]> rows(new uint8_t[(size_t)batch * stride]);
    if (!read_n(rows.get(), (size_t)batch * stride)) return bad("truncated rows");
    pzk_r1cs* r = nullptr;
    if (pzk_r1cs_load(file.get(), len, &r) || !r) return bad("load");
    pzk_quotient_info qi;
    int32_t rc = pzk_r1cs_quotient_info(r, &qi);
    uint32_t k = 0;
    if (rc == 0) {
      k = qi.log2_n;
      if (k < 1 || k > 24 || qi.n != (1ull << k) || qi.n_rows > qi.n || qi.n_rows <= qi.n / 2) return bad("info");
      if (k > 16) return bad("a case too large for this driver");
      const size_t h_stride = 32 * (size_t)qi.n;
      std::unique_ptr<uint8_t[]> h(new uint8_t[batch * h_stride]);
      memset(h.get(), 0xEE, batch * h_stride);
      if (pzk_r1cs_quotient_host(r, rows.get(), batch, stride, h.get(), h_stride - 16) != PZK_E_ARG) return bad("short h stride accepted");
      if (pzk_r1cs_quotient_host(r, rows.get(), batch, stride, h.get(), h_stride + 8) != PZK_E_ARG) return bad("misaligned h stride accepted");
      rc = pzk_r1cs_quotient_host(r, rows.get(), batch, stride, h.get(), h_stride);
      fwrite(&rc, 4, 1, stdout);
      fwrite(&k, 4, 1, stdout);
      if (rc == 0) fwrite(h.get(), 1, batch * h_stride, stdout);
    } else {
      if (rc != PZK_E_ARG || pzk::g_msg.empty()) return bad("info error");
      fwrite(&rc, 4, 1, stdout);
      fwrite(&k, 4, 1, stdout);
    }
    pzk_r1cs_destroy(r);
    fflush(stdout);
  }
  return 0;
}
