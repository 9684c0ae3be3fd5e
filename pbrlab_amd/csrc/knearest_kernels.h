// knearest_kernels.h -- launch interface of the k-nearest kernel (knearest.hip): the K nearest primitives of a point within its radius
// and their count (pbrhip_k_nearest, pbrhip_k_nearest_device).  DESIGN.md §22.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

constexpr uint32_t kKNearestMax = 32u;  // PBRHIP_K_NEAREST_MAX

// n queries (one 16-byte word each: point | max_dist) against every unit of the scene, on the <CURVES, WIDE> tree the render of this scene
// walks.  count (null: not wanted): per query the number of units with D2 <= max_dist^2, not capped.  ident (null: a pure count; k
// entries of 4 words per query, k <= kKNearestMax, n * k < 2^31): the first min(count, k) units in the order (D2, gid, sub) as slot, bits
// of u, v, sqrt(D2); the remaining entries (kNone, 0, 0, 0).  closest (null: not wanted; requires ident; the same k entries): the closest
// point | D2 of every listed entry, zeros past them.  count or ident is given.  An inactive query (dnearest.h::point_active) has count 0
// and rows of misses.  overflow: one zeroed word; spill: kSpillWords.
struct KNearestArgs {
  const float4* points;
  uint32_t n;
  uint32_t k;
  uint32_t* count;
  uint4* ident;
  float4* closest;
  uint32_t* overflow;
  uint32_t* spill;
};
void launch_k_nearest(hipStream_t s, const DScene& sc, const KNearestArgs& a, const Knobs& k);

}  // namespace pb
