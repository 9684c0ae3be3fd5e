// emission_kernels.h -- launch interface of the feature pass with a first-hit emission layer and of the per-pixel split and merge
// (emission.hip).  DESIGN.md §18.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "feature_kernels.h"

namespace pb {

// k_features_emission: k_features' arguments (feature_kernels.h) and one more image.  The grid, the spill area and the <CURVES, WIDE>
// instance are launch_features'.
void launch_features_emission(hipStream_t s, const DScene& sc, const FeatureArgs& a, float4* emission, const Knobs& k);

// pbrhip_emission_split's arguments as the kernel takes them
struct EmissionSplitArgs {
  size_t npx;
  const float4* rgba;  // RenderLayer sums
  const uint32_t* count;
  const float4* emission;           // sum of Le_first rgb | emitting samples
  const float4* albedo_hits;        // or null (with feature_count and out_albedo_hits)
  const uint32_t* feature_count;
  float4* out_rgba;                 // may be rgba
  float4* out_albedo_hits;          // may be albedo_hits
};
void launch_emission_split(hipStream_t s, const EmissionSplitArgs& a);

// pbrhip_emission_merge's
struct EmissionMergeArgs {
  size_t npx;
  const float4* filtered;
  const float4* emission;
  const uint32_t* count;
  float4* out;  // may be filtered
};
void launch_emission_merge(hipStream_t s, const EmissionMergeArgs& a);

}  // namespace pb
