// emission.hip -- the first-hit emission layer (pbrhip_render_features_emission, pbrhip_emission_split, pbrhip_emission_merge;
// DESIGN.md §18): the light the camera sees directly, kept apart from the light surfaces reflect, so that only the latter is divided
// by the albedo.
//
//   k_features_emission  features.hip::k_features' walker (dfirsthit.h::first_hit_walk) with EMISSION on: one more sum, what the renderer
//                        adds to L at depth 0 (kernels.hip::path_head with first == true: weight 1, throughput 1; env_miss_path for a
//                        camera ray), and the number of samples that added it
//   k_emission_split     per pixel: the sums minus the emission sums, clamped at 0; the albedo sums with hits := samples (a miss is black)
//   k_emission_merge     per pixel: filtered + emission / samples
//
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction.
#include "dfirsthit.h"
#include "emission_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_features_emission(DScene sc, FeatureArgs a, float4* emission) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  first_hit_walk<CURVES, WIDE, true>(sc, a, emission, stk, CameraRays{a});
}

// launch_features' grid and its rule for <CURVES, WIDE> (features.hip)
void launch_features_emission(hipStream_t s, const DScene& sc, const FeatureArgs& a, float4* emission, const Knobs& k) {
  if (!a.npix || !a.npass) return;
  const uint32_t g = feature_grid<kBlock>(a.npix);
  with_hook_tree([&](auto c, auto w) { hipLaunchKernelGGL((k_features_emission<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a, emission); }, sc, k);
}

// ------------------------------------------------------------------ split and merge
// The definitions are include/pbrhip.h's.  A thread reads its pixel before it writes it: out_rgba may be rgba, out_albedo_hits may be
// albedo_hits, out may be filtered (hence no __restrict__ on those).
__device__ __forceinline__ float pos_part(float d) { return d > 0.0f ? d : 0.0f; }  // (a NaN difference gives 0)

__global__ __launch_bounds__(kBlock) void k_emission_split(EmissionSplitArgs a) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < a.npx; p += (size_t)gridDim.x * kBlock) {
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.count[p] != 0u) {
      const float4 c = a.rgba[p], e = a.emission[p];
      out = make_float4(pos_part(c.x - e.x), pos_part(c.y - e.y), pos_part(c.z - e.z), c.w);
    }
    a.out_rgba[p] = out;
    if (a.out_albedo_hits) {
      const float4 ah = a.albedo_hits[p];
      a.out_albedo_hits[p] = make_float4(ah.x, ah.y, ah.z, (float)a.feature_count[p]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_emission_merge(EmissionMergeArgs a) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < a.npx; p += (size_t)gridDim.x * kBlock) {
    float4 out = a.filtered[p];
    const uint32_t cnt = a.count[p];
    if (cnt != 0u) {
      const float4 e = a.emission[p];
      const float fc = (float)cnt;
      out.x = out.x + e.x / fc, out.y = out.y + e.y / fc, out.z = out.z + e.z / fc;
    }
    a.out[p] = out;
  }
}

static inline uint32_t pixel_grid(size_t npx) {
  const size_t g = (npx + kBlock - 1) / kBlock;
  return (uint32_t)(g < 8192 ? g : 8192);
}
void launch_emission_split(hipStream_t s, const EmissionSplitArgs& a) {
  if (!a.npx) return;
  hipLaunchKernelGGL(k_emission_split, dim3(pixel_grid(a.npx)), dim3(kBlock), 0, s, a);
}
void launch_emission_merge(hipStream_t s, const EmissionMergeArgs& a) {
  if (!a.npx) return;
  hipLaunchKernelGGL(k_emission_merge, dim3(pixel_grid(a.npx)), dim3(kBlock), 0, s, a);
}

}  // namespace pb
