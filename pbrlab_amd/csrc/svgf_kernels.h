// svgf_kernels.h -- launch interface of the object-id gather, the variance-carrying accumulation and the variance-guided filter
// (svgf.hip).  DESIGN.md §17.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"

namespace pb {

// ids[p] = word 24 + what of the ShadeRec of slot ident[4 p]; kNone for a miss or a slot >= num_slots
void launch_object_ids(hipStream_t s, const ShadeRec* shade, uint32_t num_slots, const uint4* ident, size_t npx, uint32_t what, uint32_t* ids);

// pbrhip_svgf_accumulate's arguments as the kernel takes them
struct SvgfAccumArgs {
  uint32_t width, height;
  const float4* rgba;           // RenderLayer sums
  const uint32_t* count;
  const float4* albedo_hits;    // with feature_count, or both null: a = 1
  const uint32_t* feature_count;
  const float4* motion;
  const float4* guide;
  const uint32_t* ids;          // or null: no identity test
  const float4* hist_illum;     // e.rgb | history length; or null (with hist_var, hist_guide): no history
  const float* hist_var;
  const float4* hist_guide;
  const uint32_t* hist_ids;     // with ids and a history
  float alpha_min, sigma_depth, normal_cos_min, max_history;
  float4* out_illum;
  float* out_var;
};
void launch_svgf_accumulate(hipStream_t s, const SvgfAccumArgs& a);

// pbrhip_svgf_filter's arguments as the kernels take them (the defaults resolved)
struct SvgfFilterArgs {
  uint32_t width, height;
  const float4* illum;          // e.rgb | history length (> 0: live)
  const float* var;
  const float4* guide;          // N.xyz | z; z == 0: background
  const uint32_t* ids;          // or null
  const float4* albedo_hits;    // with feature_count, or both null
  const uint32_t* feature_count;
  float sigma_lum, sigma_depth;
  uint32_t normal_squarings;
};
// ev = e(0).rgb | v(0) of every pixel; v < 0 marks a pixel that is not live: with the caller's guide and ids a tap is two 16-byte loads
// and one 4-byte load
void launch_svgf_prepare(hipStream_t s, const SvgfFilterArgs& a, float4* ev);
// iteration i (step 2^i): src -> dst; feedback (or null) receives e(i+1).rgb | length; `last` multiplies the clamped albedo back
void launch_svgf_iteration(hipStream_t s, const SvgfFilterArgs& a, uint32_t i, bool last, const float4* src, float4* dst, float4* feedback);

}  // namespace pb
