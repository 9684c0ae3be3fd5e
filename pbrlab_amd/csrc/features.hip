// features.hip -- first-hit feature buffers (pbrhip_render_features): per pixel the sums, over a range of passes, of
// what the camera ray of each sample saw first -- albedo, viewer-facing shading normal, distance -- and the number of samples.
//
// The kernel is the first-hit walker (dfirsthit.h::first_hit_walk, which says what a lane does) over the renderer's own camera rays.
// A translation unit of its own: the render kernels' code objects do not depend on it.
#include "dfirsthit.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_features(DScene sc, FeatureArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  first_hit_walk<CURVES, WIDE, false>(sc, a, nullptr, stk, CameraRays{a});
}

// the <CURVES, WIDE> of the tree the render of this scene walks; the binary tree's instance always carries the curve code (the hooks' rule)
void launch_features(hipStream_t s, const DScene& sc, const FeatureArgs& a, const Knobs& k) {
  if (!a.npix || !a.npass) return;
  const uint32_t g = feature_grid<kBlock>(a.npix);
  with_hook_tree([&](auto c, auto w) { hipLaunchKernelGGL((k_features<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, sc, k);
}

}  // namespace pb
