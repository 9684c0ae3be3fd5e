// sdf_kernels.h -- launch interface of the signed-distance kernels (sdf.hip): the pseudonormal table of a committed
// scene and the signed nearest-point queries that read it (pbrhip_signed_distance*, pbrhip_scene_signed_distance_info).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

constexpr uint32_t kSdfRows = 7;  // rows of the table per slot: ab, bc, ca, a, b, c, face (xyz | 0); zeros for a curve slot

// The table from the slots as they are (DScene::slots), in two launches.  faces: 2 x ns working words (unit normal | has one;
// corner angles at a, b, c | 0).  slot_feat / feat_off / feat_items: sdf_topology.h's lists on the device.  table: kSdfRows x ns.
struct SdfTableArgs {
  const float4* slots;
  uint32_t ns;
  const uint32_t* slot_feat;
  const uint32_t* feat_off;
  const uint32_t* feat_items;
  float4* faces;
  float4* table;
};
void launch_sdf_table(hipStream_t s, const SdfTableArgs& a);

// n points (p | max_dist) -> ident and closest as NearestArgs', and sd (N | signed distance); any of the three may be null.
// grid != 0: the points are origin + (float)(i, j, k) * spacing over dims (x fastest), max_dist for all, n = dims.x dims.y dims.z, and
// only grid_sd (one float per point) is written.
struct SignedArgs {
  const float4* points;
  uint32_t n;
  uint4* ident;
  float4* closest;
  float4* sd;
  const float4* table;
  uint32_t* overflow;
  uint32_t* spill;
  uint32_t grid;
  float origin[3], spacing[3], max_dist;
  uint32_t dims[3];
  float* grid_sd;
};
void launch_signed(hipStream_t s, const DScene& sc, const SignedArgs& a, const Knobs& k);

}  // namespace pb
