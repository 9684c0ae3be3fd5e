// allhits.hip -- all-hits ray queries (pbrhip_trace_all, pbrhip_trace_all_device): per ray the number of accepted hits in
// (tmin, tmax] and the K nearest of them, ordered by (t, canonical primitive id, u).
//
//   k_all_hits   one ray per lane in a grid-stride loop, k_query_nearest's launch class (256 lanes, kSimpleLdsStack stack entries per
//                lane in LDS, the rest in the spill area, four blocks per CU).  The contract, the list of the K best -- kept in the ray's
//                own output row -- and the traversal are dallhits.h's; the primitive and box tests are dtrace.h's, so entry 0 of a row is
//                pbrhip_trace_closest_device's ident of the same ray and the result is a property of (ray, primitive set) alone.
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction.
#include <type_traits>

#include "allhits_kernels.h"
#include "dallhits.h"
#include "feature_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

// COUNT: a.count is given (the interval never shrinks); otherwise a.ident is and a.k >= 1
template <bool COUNT, bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_all_hits(DScene sc, AllHitsArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  uint32_t overflow = 0u;
  const uint32_t K = a.ident ? a.k : 0u;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const float4 o4 = a.rays[2 * (size_t)i], d4 = a.rays[2 * (size_t)i + 1];
    AllList L;
    L.row = K ? a.ident + (size_t)i * K : nullptr, L.K = K, L.len = 0u, L.cnt = 0u, L.kth = d4.w;
    if (ray_active(o4, d4))
      all_traverse<COUNT, CURVES, WIDE>(sc, ld3(o4), ld3(d4), o4.w, d4.w, L, stk + threadIdx.x, kBlock, &overflow,
                                        a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
    for (uint32_t j = L.len; j < K; j++) L.row[j] = make_uint4(kNone, 0u, 0u, 0u);
    if (COUNT) a.count[i] = L.cnt;
  }
  if (overflow) *a.overflow = 1u;
}

void launch_all_hits(hipStream_t s, const DScene& sc, const AllHitsArgs& a, const Knobs& k) {
  if (!a.n) return;
  const uint32_t g = feature_grid<kBlock>(a.n);
  with_flags([&](auto cnt, auto c, auto w) { hipLaunchKernelGGL((k_all_hits<cnt, c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, a.count != nullptr,
             sc.num_curves != 0, use_wide(sc, k));
}

}  // namespace pb
