// query_kernels.h -- launch interface of the query kernels (query.hip): ray and nearest-point queries answered from device memory
// (pbrhip_trace_closest_device, pbrhip_trace_any_device, pbrhip_nearest_point*).  DESIGN.md §19.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

// n rays (two 16-byte words each: org | tmin, dir | tmax) through the production traversal (dtrace_pv.h::trace_pv), the <CURVES, WIDE>
// instance the render of this scene walks.  occ != null: any-hit, n occlusion bytes, ident and hits are not used; else closest-hit:
// ident (4 words per ray: slot, bits of u, v, t; a miss (kNone, 0, 0, 0)) and / or hits (HookHit), either may be null.  An inactive ray
// (dtrace.h::ray_active) is a miss / not occluded.  counts: kCntNum zeroed words (queue head + overflow flag); spill: kSpillWords.
struct RayQueryArgs {
  const float4* rays;
  uint32_t n;
  uint4* ident;
  HookHit* hits;
  uint8_t* occ;
  uint32_t* counts;
  uint32_t* spill;
};
void launch_ray_query(hipStream_t s, const DScene& sc, const RayQueryArgs& a, const Knobs& k);

// n points (one 16-byte word each: p | max_dist) against every primitive of the scene: ident (slot, bits of u, v, sqrtf(D2); a miss
// (kNone, 0, 0, 0)) and / or closest (q | D2; a miss zeros), either may be null.  overflow: one zeroed word; spill: kSpillWords.
struct NearestArgs {
  const float4* points;
  uint32_t n;
  uint4* ident;
  float4* closest;
  uint32_t* overflow;
  uint32_t* spill;
};
void launch_nearest(hipStream_t s, const DScene& sc, const NearestArgs& a, const Knobs& k);

}  // namespace pb
