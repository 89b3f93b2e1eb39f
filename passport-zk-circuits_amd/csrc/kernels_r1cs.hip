// k_r1cs_check / k_r1cs_check_long (r1cs.hpp), the device half of a pzk_r1cs and the two check entry points of the
// C ABI; own translation unit, so the other kernel units are compiled exactly as before.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pzkwit.h"
#include "host_api.hpp"

#define PZK_R1CS_KERNEL
#include "r1cs.hpp"

using namespace pzk;

#define R1CS_HIPCHK(x)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return api_fail(PZK_E_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

namespace {

typedef R1csDevGuard DevGuard;

void r1cs_dev_free(pzk_r1cs* r) {
  if (r->device < 0) return;
  DevGuard dg(r->device);
  if (dg.err != hipSuccess) return;
  R1csDevice& D = r->dev;
  if (D.stream) (void)hipStreamSynchronize(D.stream);
  for (void* p : {(void*)D.lc_off, (void*)D.terms, (void*)D.coeffs, (void*)D.chunks, (void*)D.long_list,
                  (void*)D.quot_tables, (void*)D.quot_scratch})
    if (p) (void)hipFree(p);
  if (D.stream) (void)hipStreamDestroy(D.stream);
  D = R1csDevice();
}

template <class T, class V>
int r1cs_upload(T** dst, const V* src, size_t n) {
  // (an empty table still gets an allocation: the kernels take the pointer, and read nothing through it)
  if (hipMalloc(dst, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return api_fail(PZK_E_NOMEM, "device allocation of the r1cs program failed");
  }
  if (n) R1CS_HIPCHK(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

// first check (or quotient): the program goes to the current device, the coefficient table to Montgomery form there
int pzk::r1cs_ensure_device(pzk_r1cs* r) {
  if (r->dev.stream) return 0;
  const R1csProgram& P = r->prog;
  R1csDevice& D = r->dev;
  r->dev_free = r1cs_dev_free;
  static_assert(sizeof(uint64_t) * 4 == sizeof(uint32_t) * 8, "coefficient layout");
  int rc = r1cs_upload(&D.lc_off, P.lc_off.data(), P.lc_off.size());
  if (!rc) rc = r1cs_upload(&D.terms, P.terms.data(), P.terms.size());
  if (!rc) rc = r1cs_upload(&D.coeffs, reinterpret_cast<const uint32_t*>(P.coeffs.data()), 2 * P.coeffs.size());
  if (!rc) rc = r1cs_upload(&D.chunks, P.chunks.data(), P.chunks.size());
  if (!rc) rc = r1cs_upload(&D.long_list, P.long_list.data(), P.long_list.size());
  if (rc) { r1cs_dev_free(r); return rc; }
  hipStream_t st = nullptr;
  if (hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) {
    r1cs_dev_free(r);
    return api_fail(PZK_E_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
  }
  const uint32_t nc = (uint32_t)(P.coeffs.size() / 4);
  hipLaunchKernelGGL(k_r1cs_coeffs, dim3((nc + 255) / 256), dim3(256), 0, st, D.coeffs, nc);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  D.stream = st;
  if (e != hipSuccess) {
    r1cs_dev_free(r);
    return api_fail(PZK_E_HIP, std::string("k_r1cs_coeffs: ") + hipGetErrorString(e));
  }
  return 0;
}

namespace {

// both kernels on st; first_failed / n_failed are pre-set on the same stream
int r1cs_launch(pzk_r1cs* r, const uint8_t* d_wtns, uint32_t batch, size_t stride, int32_t* d_first, uint32_t* d_n,
                hipStream_t st) {
  const R1csProgram& P = r->prog;
  const R1csDevice& D = r->dev;
  R1CS_HIPCHK(hipMemsetAsync(d_first, 0xFF, sizeof(int32_t) * (size_t)batch, st));
  if (d_n) R1CS_HIPCHK(hipMemsetAsync(d_n, 0, sizeof(uint32_t) * (size_t)batch, st));
  // x: chunks (or groups of four long constraints), y: witness tiles; both grid-strided above ~64k workgroups
  const uint32_t tiles = (batch + R1CS_WT - 1) / R1CS_WT;
  auto grid = [&](size_t items) {
    const uint32_t gx = (uint32_t)std::min<size_t>(items, 65536);
    return dim3(gx, std::min<uint32_t>(tiles, std::min<uint32_t>(65536 / gx + 1, 65535)));
  };
  if (!P.chunks.empty()) {
    hipLaunchKernelGGL(k_r1cs_check, grid(P.chunks.size()), dim3(R1CS_THREADS), 0, st, D.chunks, (uint32_t)P.chunks.size(),
                       D.lc_off, D.terms, D.coeffs, d_wtns, (uint64_t)stride, batch, d_first, d_n);
    R1CS_HIPCHK(hipGetLastError());
  }
  if (!P.long_list.empty()) {
    const size_t groups = (P.long_list.size() + R1CS_THREADS / 64 - 1) / (R1CS_THREADS / 64);
    hipLaunchKernelGGL(k_r1cs_check_long, grid(groups), dim3(R1CS_THREADS), 0, st, D.long_list, (uint32_t)P.long_list.size(),
                       D.lc_off, D.terms, D.coeffs, d_wtns, (uint64_t)stride, batch, d_first, d_n);
    R1CS_HIPCHK(hipGetLastError());
  }
  return 0;
}

int r1cs_check_args(const pzk_r1cs* r, const void* wtns, size_t batch, size_t stride, const void* first) {
  if (!r || !wtns || !first) return api_fail(PZK_E_ARG, "null argument");
  if (batch >> 31) return api_fail(PZK_E_ARG, "batch >= 2^31: split it");
  if (stride < 32ull * r->prog.n_wires || stride % 16) return api_fail(PZK_E_ARG, "bad witness stride");
  return 0;
}

}  // namespace

// device bound at the first check; the object's own stream unless the caller gives one
int pzk::r1cs_bind(pzk_r1cs* r, const pzk_exec* ex) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return api_fail(PZK_E_NODEVICE, "no HIP device visible: pzkwit has no CPU fallback (pzk_r1cs_eval_host is the host twin)");
  }
  if (r->device < 0) {
    int dev = ex && ex->device >= 0 ? ex->device : -1;
    if (dev < 0) R1CS_HIPCHK(hipGetDevice(&dev));
    if (dev >= ndev) return api_fail(PZK_E_ARG, "pzk_exec.device " + std::to_string(dev) + ": no such device");
    r->device = dev;
  } else if (ex && ex->device >= 0 && ex->device != r->device) {
    return api_fail(PZK_E_ARG, "pzk_exec.device " + std::to_string(ex->device) + " != the device of this pzk_r1cs's first check, " +
                                   std::to_string(r->device));
  }
  return 0;
}

namespace {

int r1cs_check_batch_impl(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, int32_t* d_first,
                          uint32_t* d_n, const pzk_exec* ex) {
  if (r && batch == 0) return 0;
  if (int rc = r1cs_check_args(r, d_wtns, batch, stride, d_first)) return rc;
  if ((uintptr_t)d_wtns % 16) return api_fail(PZK_E_ARG, "witness rows must be 16-byte aligned");
  std::lock_guard<std::mutex> lock(r->mu);
  if (int rc = r1cs_bind(r, ex)) return rc;
  DevGuard dg(r->device);
  if (dg.err != hipSuccess) return api_fail(PZK_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
  if (int rc = r1cs_ensure_device(r)) return rc;
  hipStream_t st = (ex && ex->stream) ? (hipStream_t)ex->stream : r->dev.stream;
  if (int rc = r1cs_launch(r, d_wtns, (uint32_t)batch, stride, d_first, d_n, st)) return rc;
  if (ex && (ex->flags & PZK_EXEC_SYNC)) R1CS_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int r1cs_check_batch_host_impl(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, int32_t* first,
                               uint32_t* n_failed, const pzk_exec* ex) {
  if (r && batch == 0) return 0;
  if (int rc = r1cs_check_args(r, h_wtns, batch, stride, first)) return rc;
  std::lock_guard<std::mutex> lock(r->mu);
  if (int rc = r1cs_bind(r, ex)) return rc;
  DevGuard dg(r->device);
  if (dg.err != hipSuccess) return api_fail(PZK_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
  if (int rc = r1cs_ensure_device(r)) return rc;
  hipStream_t st = (ex && ex->stream) ? (hipStream_t)ex->stream : r->dev.stream;
  uint8_t* d_rows = nullptr;
  uint32_t* d_res = nullptr;  // first_failed, then n_failed
  auto release = [&]() {
    if (d_rows) (void)hipFree(d_rows);
    if (d_res) (void)hipFree(d_res);
  };
  if (hipMalloc(&d_rows, batch * stride) != hipSuccess || hipMalloc(&d_res, 8 * batch) != hipSuccess) {
    (void)hipGetLastError();
    release();
    return api_fail(PZK_E_NOMEM, "device allocation of the witness rows failed");
  }
  int rc = 0;
  hipError_t e = hipMemcpyAsync(d_rows, h_wtns, batch * stride, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) rc = r1cs_launch(r, d_rows, (uint32_t)batch, stride, (int32_t*)d_res, n_failed ? d_res + batch : nullptr, st);
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(first, d_res, 4 * batch, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && !rc && n_failed) e = hipMemcpyAsync(n_failed, d_res + batch, 4 * batch, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // the results are host memory: the call is complete on return
  release();
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return api_fail(PZK_E_HIP, std::string("pzk_r1cs_check_batch_host: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return 0;
}

}  // namespace

extern "C" {

int pzk_r1cs_check_batch(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, int32_t* d_first_failed,
                         uint32_t* d_n_failed, const pzk_exec* ex) {
  return guarded([&] { return r1cs_check_batch_impl(r, d_wtns, batch, stride, d_first_failed, d_n_failed, ex); });
}

int pzk_r1cs_check_batch_host(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, int32_t* first_failed,
                              uint32_t* n_failed, const pzk_exec* ex) {
  return guarded([&] { return r1cs_check_batch_host_impl(r, h_wtns, batch, stride, first_failed, n_failed, ex); });
}

}  // extern "C"
