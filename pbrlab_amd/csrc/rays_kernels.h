// rays_kernels.h -- launch interface of the ray-list kernels (rays.hip): paths that start from caller-supplied rays, the three
// projections that write such rays, and the feature kernel over them.  DESIGN.md §14.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

// A caller's first rays (device memory): two 16-byte words per ray, org | tmin and dir | tmax (pbrhip_ray).  The ray of (pixel gpix,
// pass) is rays[2 * ((ray_passes == 1 ? 0 : pass - base_pass) * width * height + gpix)].
struct RaySource {
  const float4* rays;
  uint32_t ray_passes;    // 1: one ray per pixel, reused by every pass; else the passes of the call
  uint32_t camera_draws;  // draws the sample's generator is advanced by before the path takes it over (0 .. kMaxCameraDraws)
  uint32_t base_pass;     // the call's first pass: the pass of the buffer's first plane
  uint32_t height;
};
constexpr uint32_t kMaxCameraDraws = 16;

// k_generate_camera's twin (kernels.h::launch_generate_camera): clears the radiance and stores each path's first ray as given (tmin and
// tmax included), throughput (1, 1, 1 | pdf +inf), generator state (hold 0) and trace-queue entry.  An inactive ray (dtrace.h::ray_active)
// becomes a certain miss with throughput 0: its sample adds (0, 0, 0, 1).
void launch_generate_rays(hipStream_t s, const PathState& P, const RaySource& r, uint32_t npaths);

enum : uint32_t { kProjLatLong = 0, kProjFisheye = 1, kProjOrtho = 2 };
struct ProjectArgs {
  UserCamera cam;       // the frame: eye, r, u, f
  uint32_t projection;  // kProj*
  float param;          // fisheye: half the field of view in radians; ortho: half the height in world units
  uint32_t width, height, first_pass, npass;
  uint64_t seed_seq;
  float4* rays;         // npass x width x height rays
};
void launch_project_rays(hipStream_t s, const ProjectArgs& a);

// k_features (feature_kernels.h) with the ray of each sample loaded instead of computed
struct FeatureRayArgs {
  RaySource src;        // (camera_draws is not used: no generator runs)
  uint32_t width;
  const uint32_t* pix;
  uint32_t npix;
  uint32_t first_pass, npass;
  const float4* mat_albedo;
  float4* albedo_hits;
  float4* normal_depth;
  uint32_t* count;
  uint32_t* overflow;
  uint32_t* spill;
};
void launch_features_rays(hipStream_t s, const DScene& sc, const FeatureRayArgs& a, const Knobs& k);

}  // namespace pb
