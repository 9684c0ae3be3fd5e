// temporal_kernels.h -- launch interface of the motion kernel and the temporal accumulation (temporal.hip).  DESIGN.md §16.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "knobs.h"

namespace pb {

// What one launch of k_motion needs besides the scene.  Lane = one pixel of `pix`: the pixel-centre pinhole ray of the current camera,
// its closest hit, and where the snapshot's camera saw the hit's point on the snapshot's slots.
struct MotionArgs {
  UserCamera ucam, ucam_prev;  // the caller's camera now / at the snapshot (user, user_prev != 0) ...
  Camera cam, cam_prev;        // ... or the reference's
  uint32_t user, user_prev;
  uint32_t width, height;
  const uint32_t* pix;         // the rank's pixels (y * width + x), ensure_pixels' order
  uint32_t npix;
  const float4* prev_slots;    // the snapshot of DScene::slots: 4 words per slot, the current scene's slot order
  float4* motion;              // W x H: mx, my, z_prev, valid (0 none, 1 a triangle, 2 a curve); or null
  float4* guide;               // W x H: viewer-facing shading normal (a curve's tangent as it is) | t; or null
  uint4* ident;                // W x H: slot, bits of u, v, t; or null
  uint32_t* overflow;          // set to 1 when a traversal needed more than kStackDepth stack entries
  uint32_t* spill;             // traversal-stack spill area (kernels.h::kSpillWords)
};
void launch_motion(hipStream_t s, const DScene& sc, const MotionArgs& a, const Knobs& k);

constexpr float kMotionCurve = 2.0f;  // motion.w of a hit on a curve: its guide is a tangent, which has no facing

// pbrhip_temporal_accumulate's arguments as the kernel takes them
struct TemporalArgs {
  uint32_t width, height;
  const float4* rgba;        // RenderLayer sums
  const uint32_t* count;
  const float4* motion;
  const float4* guide;
  const float4* hist_rgba;   // accumulated mean | history length; or null (with hist_guide): no history
  const float4* hist_guide;
  float alpha_min, sigma_depth, normal_cos_min, max_history;
  float4* out;
};
void launch_temporal(hipStream_t s, const TemporalArgs& a);

}  // namespace pb
