// feature_kernels.h -- launch interface of the first-hit feature kernel (features.hip) and the edge-avoiding filter (denoise.hip).
// DESIGN.md §12.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

// What one launch of k_features needs besides the scene.  Lane = one pixel of `pix`; the lane walks the passes
// [first_pass, first_pass + npass) in ascending order and adds each sample to the pixel's sums, which it loads before and stores after.
struct FeatureArgs {
  UserCamera ucam;  // the caller's camera (user != 0) ...
  Camera cam;       // ... or the reference's
  uint32_t user;
  uint32_t width, height;
  uint64_t seed_seq;
  const uint32_t* pix;  // the rank's pixels (y * width + x) in the order the paths of a pass are laid out in: a wave is an 8 x 8 patch
  uint32_t npix;
  uint32_t first_pass, npass;
  const float4* mat_albedo;  // per material: albedo rgb | base-colour texture id (kNone: the rgb stands)
  float4* albedo_hits;       // W x H: sum of albedo rgb | hits; or null
  float4* normal_depth;      // W x H: sum of the feature normal | sum of t; or null
  uint32_t* count;           // W x H: samples; or null
  uint32_t* overflow;        // set to 1 when a traversal needed more than kStackDepth stack entries
  uint32_t* spill;           // traversal-stack spill area: (kStackDepth - kSimpleLdsStack) x threads of the grid
};
constexpr uint32_t kFeatureBlocksPerCU = 4;  // 40 KB of LDS stack per block: four blocks per CU = four waves per SIMD, 128 VGPRs
constexpr uint32_t kFeatureGridCap = 4096;   // (the spill area of the one-ray-per-lane grids, kernels.h::kSpillWords)
// grid of a one-query-per-lane kernel of this launch class (k_features, k_features_emission, k_motion, k_query_nearest, k_signed_query,
// k_all_hits) over n queries: blocks of BLOCK lanes, at most kFeatureGridCap of them, each thread with a stack of its own in the spill
// area (kernels.h::kSpillWords, which is why that header is included here)
template <int BLOCK>
inline uint32_t feature_grid(uint32_t n) {
  static_assert((size_t)(kStackDepth - kSimpleLdsStack) * kFeatureGridCap * BLOCK <= kSpillWords, "spill area: one stack per thread of the grid");
  const uint32_t g = (n + BLOCK - 1) / BLOCK;
  return g < kFeatureGridCap ? g : kFeatureGridCap;
}
void launch_features(hipStream_t s, const DScene& sc, const FeatureArgs& a, const Knobs& k);

// The filter's parameters as the kernels take them (pbrhip_denoise has resolved the defaults).
struct DenoiseArgs {
  uint32_t width, height;
  const float4* rgba;           // RenderLayer sums
  const uint32_t* count;
  const float4* albedo_hits;    // or null (with normal_depth and feature_count: no features)
  const float4* normal_depth;
  const uint32_t* feature_count;
  uint32_t no_albedo;
  float sigma_color, sigma_depth;
  uint32_t normal_squarings;
};
// guide = N.xyz | z of every pixel, e0 = e(0).rgb | kind (kDenoise*): two 16-byte words per tap
void launch_denoise_prepare(hipStream_t s, const DenoiseArgs& a, float4* e0, float4* guide);
// iteration i (step 2^i): src -> dst; last: dst is the caller's out_rgba and receives e x albedo | 1
void launch_denoise_iteration(hipStream_t s, const DenoiseArgs& a, uint32_t i, bool last, const float4* src, const float4* guide, float4* dst);

}  // namespace pb
