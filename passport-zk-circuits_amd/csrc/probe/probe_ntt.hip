// Probe entry points for the transforms of ntt.hpp: one forward or inverse transform on the default plan or on an
// explicit split, so that tests reach the two- and three-pass code at sizes Python checks exhaustively. See probe.h.
#include <hip/hip_runtime.h>

#include "../ntt.hpp"
#include "probe_util.hpp"

using namespace pzk;
using namespace pzkprobe;

namespace {

// dst = src to (TO) or from Montgomery form, 32 B per element
template <bool TO>
__global__ void __launch_bounds__(256) k_probe_mont(const uint8_t* src, uint8_t* dst, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const fr x = load_fr(src + 32 * i);
  store_fr(dst + 32 * i, TO ? fr_to_mont_in(x) : fr_from_mont_fast(x));
}

}  // namespace

extern "C" {

int pzk_probe_ntt_plan(int k, int* q, int* r) {
  if (r) *r = NTT_R;
  if (k < 1 || k > NTT_MAX_K) return 0;
  const NttPlan p = ntt_default_plan(k);
  if (q)
    for (int i = 0; i < NTT_MAX_K; i++) q[i] = i < p.n ? p.q[i] : 0;
  return p.n;
}

int pzk_probe_ntt(int inverse, int shift, int k, int batch, const int* split, int n_split, const uint32_t* in,
                  uint32_t* out, int on_device) {
  if (k < 1 || k > NTT_MAX_K || batch < 1 || batch > 64 || !in || !out || n_split < 0 || n_split > NTT_MAX_K ||
      (n_split && !split))
    return (int)hipErrorInvalidValue;
  NttPlan pl = ntt_default_plan(k);
  if (n_split) {
    pl.n = n_split;
    for (int i = 0; i < n_split; i++) pl.q[i] = split[i];
  }
  if (!ntt_plan_ok(pl, k)) return (int)hipErrorInvalidValue;
  const uint64_t n = 1ull << k, total = n * (uint64_t)batch;
  DBuf tab, work;
  PROBE_TRY(tab.up(nullptr, ntt_table_bytes(k)));
  NttTables T;
  PROBE_TRY(ntt_build_tables(tab.as<uint8_t>(), k, T, nullptr));
  uint8_t* w;
  if (on_device) {
    w = reinterpret_cast<uint8_t*>(out);
  } else {
    PROBE_TRY(work.up(in, 32 * total));
    w = work.as<uint8_t>();
  }
  const uint8_t* src = on_device ? reinterpret_cast<const uint8_t*>(in) : w;
  hipLaunchKernelGGL(k_probe_mont<true>, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, nullptr, src, w, total);
  PROBE_TRY(hipGetLastError());
  NttVecs v;
  for (int z = 0; z < 3; z++) { v.base[z] = w; v.stride[z] = 32 * n; }
  PROBE_TRY(inverse ? ntt_inverse(v, 1, batch, pl, T, shift != 0, nullptr) : ntt_forward(v, 1, batch, pl, T, false, nullptr));
  hipLaunchKernelGGL(k_probe_mont<false>, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, nullptr, w, w, total);
  PROBE_TRY(finish());
  if (!on_device) PROBE_TRY(work.down(out, 32 * total));
  return 0;
}

}  // extern "C"
