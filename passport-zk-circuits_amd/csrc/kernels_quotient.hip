// Groth16's quotient evaluations for witness rows in HBM (include/pzkwit.h pzk_r1cs_quotient_*):
// k_r1cs_ab / k_r1cs_ab_long / k_r1cs_ab_tail write the rows a, b, c = a b of the QAP, ntt.hpp's passes take each to
// the coset, and the last pass over c leaves h = a' b' - c'. Own translation unit; the device program, the binding and
// the stream are the check's (r1cs.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pzkwit.h"
#include "host_api.hpp"

#define PZK_R1CS_KERNEL
#define PZK_R1CS_NO_KERNELS
#include "r1cs.hpp"
#include "ntt.hpp"

using namespace pzk;

#define QUOT_HIPCHK(x)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return api_fail(PZK_E_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

namespace pzk {

// a, b (normal form, below p) -> Montgomery a, b and a b
__device__ __forceinline__ void quot_abc(fr& a, fr& b, fr& c) {
  a = fr_mul_fast(a, fr_const(R2_));
  b = fr_mul_fast(b, fr_const(R2_));
  c = fr_mul_fast(a, b);
}

// Short constraints: k_r1cs_check's shape (workgroup per chunk, the chunk's terms staged in LDS, lane per constraint,
// the tile's witnesses in turn), writing instead of testing: a_k, b_k and c_k = a_k b_k in Montgomery form into row
// i's vectors v.base[0..2] + i * v.stride[0..2]. A wave's 64 elements leave as two 1 KiB stores of 16 B per lane
// (wave_store); every lane of the wave takes part, a lane past the chunk's end on zeros that are not stored.
__global__ void __launch_bounds__(R1CS_THREADS)
k_r1cs_ab(const R1csChunk* __restrict__ chunks, uint32_t n_chunks, const uint32_t* __restrict__ lc_off,
          const R1csTerm* __restrict__ terms, const uint32_t* __restrict__ coeffs, const uint8_t* __restrict__ rows,
          uint64_t stride, uint32_t batch, NttVecs v) {
  __shared__ R1csTerm s_terms[R1CS_CHUNK_TERMS];
  __shared__ uint16_t s_off[3 * R1CS_CHUNK_C + 1];
  __shared__ uint4 s_stage[(R1CS_THREADS / 64) * 128];
  const uint32_t wave = threadIdx.x >> 6;
  uint4* stage = s_stage + wave * 128;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const R1csChunk ch = chunks[c];
    const uint32_t t0 = lc_off[3ull * ch.first];
    const uint32_t nt = lc_off[3ull * (ch.first + ch.count)] - t0;  // <= R1CS_CHUNK_TERMS (the parser's chunking)
    __syncthreads();  // the previous chunk's readers are done
    for (uint32_t i = threadIdx.x; i <= 3 * ch.count; i += R1CS_THREADS) s_off[i] = (uint16_t)(lc_off[3ull * ch.first + i] - t0);
    for (uint32_t i = threadIdx.x; i < nt && i < R1CS_CHUNK_TERMS; i += R1CS_THREADS) s_terms[i] = terms[(uint64_t)t0 + i];
    __syncthreads();
    uint32_t o[4] = {0, 0, 0, 0};
    if (threadIdx.x < ch.count) {
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = s_off[3 * threadIdx.x + j];
    }
    const uint32_t w0 = 64 * wave, nvalid = ch.count > w0 ? (ch.count - w0 < 64 ? ch.count - w0 : 64) : 0;
    const uint64_t at = 32ull * (ch.first + w0);
    for (uint32_t i = blockIdx.y; i < batch; i += gridDim.y) {
      const uint8_t* row = rows + (uint64_t)i * stride;
      fr a = fr_zero(), b = fr_zero(), cc;
      for (uint32_t q = o[0]; q < o[1]; q++) a = r1cs_term(a, s_terms[q], coeffs, row);
      for (uint32_t q = o[1]; q < o[2]; q++) b = r1cs_term(b, s_terms[q], coeffs, row);
      quot_abc(a, b, cc);
      wave_store(v.base[0] + (uint64_t)i * v.stride[0] + at, el_fr(a), nvalid, stage);
      wave_store(v.base[1] + (uint64_t)i * v.stride[1] + at, el_fr(b), nvalid, stage);
      wave_store(v.base[2] + (uint64_t)i * v.stride[2] + at, el_fr(cc), nvalid, stage);
    }
  }
}

// Long constraints: k_r1cs_check_long's shape, a wave per constraint; the two wave sums run with every lane of the
// wave, outside any branch, and lane 0 stores the three elements.
__global__ void __launch_bounds__(R1CS_THREADS)
k_r1cs_ab_long(const uint32_t* __restrict__ long_list, uint32_t n_long, const uint32_t* __restrict__ lc_off,
               const R1csTerm* __restrict__ terms, const uint32_t* __restrict__ coeffs, const uint8_t* __restrict__ rows,
               uint64_t stride, uint32_t batch, NttVecs v) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t g = (uint64_t)blockIdx.x * (R1CS_THREADS / 64) + wave; g < n_long;
       g += (uint64_t)gridDim.x * (R1CS_THREADS / 64)) {
    const uint32_t k = long_list[g];
    uint32_t o[3];
#pragma unroll
    for (int j = 0; j < 3; j++) o[j] = lc_off[3ull * k + j];
    for (uint32_t i = blockIdx.y; i < batch; i += gridDim.y) {
      const uint8_t* row = rows + (uint64_t)i * stride;
      fr a = fr_zero(), b = fr_zero(), cc;
      for (uint32_t q = o[0] + lane; q < o[1]; q += 64) a = r1cs_term(a, terms[q], coeffs, row);
      for (uint32_t q = o[1] + lane; q < o[2]; q += 64) b = r1cs_term(b, terms[q], coeffs, row);
      a = r1cs_wave_sum(a);
      b = r1cs_wave_sum(b);
      quot_abc(a, b, cc);
      if (lane == 0) {
        store_fr(v.base[0] + (uint64_t)i * v.stride[0] + 32ull * k, a);
        store_fr(v.base[1] + (uint64_t)i * v.stride[1] + 32ull * k, b);
        store_fr(v.base[2] + (uint64_t)i * v.stride[2] + 32ull * k, cc);
      }
    }
  }
}

// Rows nc .. n - 1 of the three vectors: a = w_s for the public wires s = 0 .. n_pub (the rows snarkjs' setup appends),
// zero after them; b = c = 0. A lane per 16-byte half of an element.
__global__ void __launch_bounds__(256)
k_r1cs_ab_tail(const uint8_t* __restrict__ rows, uint64_t stride, uint32_t nc, uint32_t n_pub, uint32_t n, NttVecs v) {
  const uint64_t u2 = 2ull * nc + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t i = (uint32_t)(u2 >> 1), hf = (uint32_t)(u2 & 1), y = blockIdx.y;
  if (i >= n) return;
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (i - nc <= n_pub) {
    const fr a = fr_mul_fast(r1cs_residue(load_fr(rows + (uint64_t)y * stride + 32ull * (i - nc))), fr_const(R2_));
    x = hf ? make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]) : make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  }
  const uint64_t at = 32ull * i + 16 * hf;
  *reinterpret_cast<uint4*>(v.base[0] + (uint64_t)y * v.stride[0] + at) = x;
  *reinterpret_cast<uint4*>(v.base[1] + (uint64_t)y * v.stride[1] + at) = make_uint4(0u, 0u, 0u, 0u);
  *reinterpret_cast<uint4*>(v.base[2] + (uint64_t)y * v.stride[2] + at) = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace pzk

namespace {

// first quotient call: the tables and the tile's b and c vectors, on the bound device; the build is waited for
int quot_ensure(pzk_r1cs* r, int k) {
  R1csDevice& D = r->dev;
  if (D.quot_tables) return 0;
  const size_t n = (size_t)1 << k;
  uint8_t *tab = nullptr, *scr = nullptr;
  if (hipMalloc(&tab, ntt_table_bytes(k)) != hipSuccess || hipMalloc(&scr, 2 * 32 * n * QUOT_TILE) != hipSuccess) {
    (void)hipGetLastError();
    if (tab) (void)hipFree(tab);
    return api_fail(PZK_E_NOMEM, "device allocation of the quotient scratch failed");
  }
  NttTables T;
  hipError_t e = ntt_build_tables(tab, k, T, D.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(D.stream);
  if (e != hipSuccess) {
    (void)hipFree(tab);
    (void)hipFree(scr);
    return api_fail(PZK_E_HIP, std::string("k_ntt_tables: ") + hipGetErrorString(e));
  }
  D.quot_tables = tab;
  D.quot_scratch = scr;
  D.quot_rows = QUOT_TILE;
  return 0;
}

int quot_args(const pzk_r1cs* r, const void* wtns, size_t batch, size_t stride, const void* h, size_t h_stride, int& k) {
  if (!r || !wtns || !h) return api_fail(PZK_E_ARG, "null argument");
  uint64_t m;
  if (!r1cs_quotient_domain(r->prog, m, k))
    return api_fail(PZK_E_ARG, "quotient: " + std::to_string(m) + " rows: the domain 2^k must have 1 <= k <= 24");
  if ((uint64_t)r->prog.n_pub_out + r->prog.n_pub_in >= r->prog.n_wires)
    return api_fail(PZK_E_ARG, "quotient: the header counts more public wires than wires");
  if (batch >> 31) return api_fail(PZK_E_ARG, "batch >= 2^31: split it");
  if (stride < 32ull * r->prog.n_wires || stride % 16) return api_fail(PZK_E_ARG, "bad witness stride");
  if (h_stride < (32ull << k) || h_stride % 16) return api_fail(PZK_E_ARG, "bad h stride");
  return 0;
}

// one tile of rows <= QUOT_TILE witnesses on st; ev (five events) brackets the stages when not null
int quot_tile(pzk_r1cs* r, int k, const uint8_t* d_wtns, uint32_t rows, size_t stride, uint8_t* d_h, size_t h_stride,
              hipStream_t st, hipEvent_t* ev) {
  const R1csProgram& P = r->prog;
  const R1csDevice& D = r->dev;
  const uint64_t n = 1ull << k;
  NttTables T = ntt_table_layout(k);
  T.base = D.quot_tables;
  const NttPlan pl = ntt_default_plan(k);
  NttVecs v;
  v.base[0] = d_h; v.stride[0] = h_stride;
  v.base[1] = D.quot_scratch; v.stride[1] = 32 * n;
  v.base[2] = D.quot_scratch + 32 * n * QUOT_TILE; v.stride[2] = 32 * n;
  if (ev) QUOT_HIPCHK(hipEventRecord(ev[0], st));
  if (!P.chunks.empty()) {
    const uint32_t gx = (uint32_t)std::min<size_t>(P.chunks.size(), 65536);
    hipLaunchKernelGGL(k_r1cs_ab, dim3(gx, std::min<uint32_t>(rows, gx < 2048 ? rows : 1)), dim3(R1CS_THREADS), 0, st, D.chunks,
                       (uint32_t)P.chunks.size(), D.lc_off, D.terms, D.coeffs, d_wtns, (uint64_t)stride, rows, v);
    QUOT_HIPCHK(hipGetLastError());
  }
  if (!P.long_list.empty()) {
    const size_t groups = (P.long_list.size() + R1CS_THREADS / 64 - 1) / (R1CS_THREADS / 64);
    hipLaunchKernelGGL(k_r1cs_ab_long, dim3((uint32_t)std::min<size_t>(groups, 65536), rows), dim3(R1CS_THREADS), 0, st,
                       D.long_list, (uint32_t)P.long_list.size(), D.lc_off, D.terms, D.coeffs, d_wtns, (uint64_t)stride, rows, v);
    QUOT_HIPCHK(hipGetLastError());
  }
  const uint64_t tail = 2 * (n - P.n_constraints);  // >= 2: M > n_constraints
  hipLaunchKernelGGL(k_r1cs_ab_tail, dim3((uint32_t)((tail + 255) / 256), rows), dim3(256), 0, st, d_wtns, (uint64_t)stride,
                     P.n_constraints, P.n_pub_out + P.n_pub_in, (uint32_t)n, v);
  QUOT_HIPCHK(hipGetLastError());
  if (ev) QUOT_HIPCHK(hipEventRecord(ev[1], st));
  QUOT_HIPCHK(ntt_inverse(v, 3, (int)rows, pl, T, true, st));
  if (ev) QUOT_HIPCHK(hipEventRecord(ev[2], st));
  QUOT_HIPCHK(ntt_forward(v, 2, (int)rows, pl, T, false, st));
  if (ev) QUOT_HIPCHK(hipEventRecord(ev[3], st));
  NttVecs q;  // {c, a', b'}
  q.base[0] = v.base[2]; q.stride[0] = v.stride[2];
  q.base[1] = v.base[0]; q.stride[1] = v.stride[0];
  q.base[2] = v.base[1]; q.stride[2] = v.stride[1];
  QUOT_HIPCHK(ntt_forward(q, 1, (int)rows, pl, T, true, st));
  if (ev) QUOT_HIPCHK(hipEventRecord(ev[4], st));
  return 0;
}

int quot_launch(pzk_r1cs* r, int k, const uint8_t* d_wtns, size_t batch, size_t stride, uint8_t* d_h, size_t h_stride,
                hipStream_t st, bool timing) {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = 0;
  if (timing)
    for (auto& e : ev)
      if (hipEventCreate(&e) != hipSuccess) { rc = api_fail(PZK_E_HIP, "hipEventCreate failed"); break; }
  for (size_t b0 = 0; !rc && b0 < batch; b0 += QUOT_TILE) {
    const uint32_t rows = (uint32_t)std::min<size_t>(QUOT_TILE, batch - b0);
    rc = quot_tile(r, k, d_wtns + b0 * stride, rows, stride, d_h + b0 * h_stride, h_stride, st, timing ? ev : nullptr);
    if (!rc && timing) {
      if (hipEventSynchronize(ev[4]) != hipSuccess) { rc = api_fail(PZK_E_HIP, "hipEventSynchronize failed"); break; }
      for (int s = 0; s < 4; s++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[s], ev[s + 1]) == hipSuccess) r->quot_ms[s] += ms;
      }
    }
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int quotient_batch_impl(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, uint8_t* d_h, size_t h_stride,
                        const pzk_exec* ex) {
  if (r && batch == 0) return 0;
  int k;
  if (int rc = quot_args(r, d_wtns, batch, stride, d_h, h_stride, k)) return rc;
  if ((uintptr_t)d_wtns % 16 || (uintptr_t)d_h % 16) return api_fail(PZK_E_ARG, "witness and h rows must be 16-byte aligned");
  std::lock_guard<std::mutex> lock(r->mu);
  if (int rc = r1cs_bind(r, ex)) return rc;
  R1csDevGuard dg(r->device);
  if (dg.err != hipSuccess) return api_fail(PZK_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
  if (int rc = r1cs_ensure_device(r)) return rc;
  if (int rc = quot_ensure(r, k)) return rc;
  hipStream_t st = (ex && ex->stream) ? (hipStream_t)ex->stream : r->dev.stream;
  if (int rc = quot_launch(r, k, d_wtns, batch, stride, d_h, h_stride, st, ex && (ex->flags & PZK_EXEC_TIMING))) return rc;
  if (ex && (ex->flags & PZK_EXEC_SYNC)) QUOT_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int quotient_batch_host_impl(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h, size_t h_stride,
                             const pzk_exec* ex) {
  if (r && batch == 0) return 0;
  int k;
  if (int rc = quot_args(r, h_wtns, batch, stride, h, h_stride, k)) return rc;
  if (batch > SIZE_MAX / std::max(stride, h_stride)) return api_fail(PZK_E_ARG, "batch * stride overflows");
  std::lock_guard<std::mutex> lock(r->mu);
  if (int rc = r1cs_bind(r, ex)) return rc;
  R1csDevGuard dg(r->device);
  if (dg.err != hipSuccess) return api_fail(PZK_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
  if (int rc = r1cs_ensure_device(r)) return rc;
  if (int rc = quot_ensure(r, k)) return rc;
  hipStream_t st = (ex && ex->stream) ? (hipStream_t)ex->stream : r->dev.stream;
  const size_t row_h = (size_t)32 << k;  // the device rows are dense: bytes past 32 N of a host row are not written
  uint8_t *d_rows = nullptr, *d_h = nullptr;
  auto release = [&]() {
    if (d_rows) (void)hipFree(d_rows);
    if (d_h) (void)hipFree(d_h);
  };
  if (hipMalloc(&d_rows, batch * stride) != hipSuccess || hipMalloc(&d_h, batch * row_h) != hipSuccess) {
    (void)hipGetLastError();
    release();
    return api_fail(PZK_E_NOMEM, "device allocation of the witness and h rows failed");
  }
  int rc = 0;
  hipError_t e = hipMemcpyAsync(d_rows, h_wtns, batch * stride, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) rc = quot_launch(r, k, d_rows, batch, stride, d_h, row_h, st, ex && (ex->flags & PZK_EXEC_TIMING));
  if (e == hipSuccess && !rc)
    e = hipMemcpy2DAsync(h, h_stride, d_h, row_h, row_h, batch, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // the result is host memory: the call is complete on return
  release();
  if (rc) return rc;
  if (e != hipSuccess || es != hipSuccess)
    return api_fail(PZK_E_HIP, std::string("pzk_r1cs_quotient_batch_host: ") + hipGetErrorString(e != hipSuccess ? e : es));
  return 0;
}

}  // namespace

extern "C" {

int pzk_r1cs_quotient_batch(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, uint8_t* d_h, size_t h_stride,
                            const pzk_exec* ex) {
  return guarded([&] { return quotient_batch_impl(r, d_wtns, batch, stride, d_h, h_stride, ex); });
}

int pzk_r1cs_quotient_batch_host(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h,
                                 size_t h_stride, const pzk_exec* ex) {
  return guarded([&] { return quotient_batch_host_impl(r, h_wtns, batch, stride, h, h_stride, ex); });
}

int pzk_r1cs_quotient_timing(pzk_r1cs* r, double ms[4], int reset) {
  return guarded([&] {
    if (!r || !ms) return api_fail(PZK_E_ARG, "null argument");
    std::lock_guard<std::mutex> lock(r->mu);
    for (int s = 0; s < 4; s++) {
      ms[s] = r->quot_ms[s];
      if (reset) r->quot_ms[s] = 0;
    }
    return 0;
  });
}

}  // extern "C"
