// allhits_kernels.h -- launch interface of the all-hits kernel (allhits.hip): the K nearest accepted hits of a ray and their count
// (pbrhip_trace_all, pbrhip_trace_all_device).  DESIGN.md §21.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dscene.h"
#include "kernels.h"
#include "knobs.h"

namespace pb {

constexpr uint32_t kAllHitsMax = 32u;  // PBRHIP_ALL_HITS_MAX

// n rays (two 16-byte words each: org | tmin, dir | tmax) against every unit of the scene, on the <CURVES, WIDE> tree the render of this
// scene walks.  count (null: not wanted): per ray the number of accepted hits in (tmin, tmax], not capped.  ident (null: a pure count; k
// entries of 4 words per ray, k <= kAllHitsMax, n * k < 2^31): the first min(count, k) hits in the order (t, gid, u) as slot, bits of u,
// v, t; the remaining entries (kNone, 0, 0, 0).  One of the two is given.  An inactive ray (dtrace.h::ray_active) has count 0 and a row
// of misses.  overflow: one zeroed word; spill: kSpillWords.
struct AllHitsArgs {
  const float4* rays;
  uint32_t n;
  uint32_t k;
  uint32_t* count;
  uint4* ident;
  uint32_t* overflow;
  uint32_t* spill;
};
void launch_all_hits(hipStream_t s, const DScene& sc, const AllHitsArgs& a, const Knobs& k);

}  // namespace pb
