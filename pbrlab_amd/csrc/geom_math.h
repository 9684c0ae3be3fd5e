// geom_math.h -- the two position-dependent expressions of a slot that the host staging (commit.cpp::slot_and_shade, prim_boxes,
// scene_bounds) and the device staging (geom_gpu.hip::k_dg_stage) both evaluate: written once, compiled for both sides with the
// library's flags (IEEE single precision, no contraction), so that either side derives the same bits from the same positions.
#pragma once

#include "dmath.h"

namespace pb {

// What the raytracer sees of an instance (raytracer_impl.cc:61-81: the transform goes to Embree and nowhere else):
// v' = v * M with the translation row, in this order of operations (the checker uses the same expression).
PB_HD V3 xf_point(const float* m, V3 v) {
  return V3(m[0] * v.x + m[4] * v.y + m[8] * v.z + m[12], m[1] * v.x + m[5] * v.y + m[9] * v.z + m[13],
            m[2] * v.x + m[6] * v.y + m[10] * v.z + m[14]);
}

// End points of linear piece `sub` of a cubic Bezier (control points xyzr): B(sub/4) and B((sub+1)/4), evaluated with
// the arithmetic of the intersection contract (Bernstein weights, products summed left to right, single precision,
// no contraction) so that every back end tests the same segment.
PB_HD void curve_piece(const float* cp, uint32_t sub, float a[4], float b[4]) {
#pragma unroll
  for (uint32_t e = 0; e < 2; e++) {
    const float u = (float)(sub + e) * 0.25f, s = 1.0f - u;
    const float b0 = s * s * s, b1 = 3.0f * u * s * s, b2 = 3.0f * u * u * s, b3 = u * u * u;
#pragma unroll
    for (int k = 0; k < 4; k++) (e ? b : a)[k] = ((cp[k] * b0 + cp[4 + k] * b1) + cp[8 + k] * b2) + cp[12 + k] * b3;
  }
}

}  // namespace pb
