// knearest.hip -- k-nearest queries (pbrhip_k_nearest, pbrhip_k_nearest_device): per query point the number of primitives
// within max_dist and the K nearest of them, ordered by (D2, canonical primitive id, piece index).
//
//   k_knearest   one query per lane in a grid-stride loop, k_all_hits' launch class (256 lanes, kSimpleLdsStack stack entries per lane in
//                LDS, the rest in the spill area, four blocks per CU).  The contract, the list of the K best -- kept in the query's own
//                output rows -- and the traversal are dknearest.h's; the candidate of (point, unit) is dnearest.h's, so entry 0 of a row
//                is pbrhip_nearest_point_device's answer and the result is a property of (point, primitive set) alone.
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction.
#include <type_traits>

#include "dknearest.h"
#include "feature_kernels.h"
#include "knearest_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

// COUNT: a.count is given (the bound never shrinks); otherwise a.ident is and a.k >= 1
template <bool COUNT, bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_knearest(DScene sc, KNearestArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  uint32_t overflow = 0u;
  const uint32_t K = a.ident ? a.k : 0u;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const float4 pt = a.points[i];
    KList L;
    L.row = K ? a.ident + (size_t)i * K : nullptr, L.cl = K && a.closest ? a.closest + (size_t)i * K : nullptr;
    L.K = K, L.len = 0u, L.cnt = 0u, L.md2 = pt.w * pt.w, L.kth = L.md2;
    if (point_active(pt))
      knearest_traverse<COUNT, CURVES, WIDE>(sc, V3(pt.x, pt.y, pt.z), L, stk + threadIdx.x, kBlock, &overflow, a.spill + blockIdx.x * kBlock + threadIdx.x,
                                             gridDim.x * kBlock);
    knearest_finish(L);
    if (COUNT) a.count[i] = L.cnt;
  }
  if (overflow) *a.overflow = 1u;
}

void launch_k_nearest(hipStream_t s, const DScene& sc, const KNearestArgs& a, const Knobs& k) {
  if (!a.n) return;
  const uint32_t g = feature_grid<kBlock>(a.n);
  with_flags([&](auto cnt, auto c, auto w) { hipLaunchKernelGGL((k_knearest<cnt, c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, a.count != nullptr,
             sc.num_curves != 0, use_wide(sc, k));
}

}  // namespace pb
