// sdf.hip -- signed distance on top of the nearest-point queries (pbrhip_signed_distance, pbrhip_signed_distance_device,
// pbrhip_signed_distance_grid_device, pbrhip_scene_signed_distance_info).
//
//   k_sdf_faces / k_sdf_rows   the angle-weighted pseudonormal table (Baerentzen & Aanaes 2005) of the scene's triangles, computed from
//                              the slots as they are -- so it serves the host path and device geometry mode alike --: per slot the unit
//                              face normal and the three corner angles, then per (slot, row) the sum over the feature's incidence
//                              list (sdf_topology.h), in ascending canonical id of the contributing face, normalised.
//   k_signed_query             k_query_nearest (query.hip) with the winning feature kept in the best-so-far record and one fetch from
//                              the table in the epilogue: s = dot(p - q, N), the distance negative when s < 0.  The contract, its
//                              traversal and the launch class are dnearest.h's and query.hip's; <.., GRID = true> makes its points in
//                              registers (origin + (float)(i, j, k) * spacing, x fastest) and writes the signed distance alone.
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction; the arctangent
// is denv.h::env_atan2, the same bits on the host and the device.
#include <type_traits>

#include "denv.h"
#include "dnearest.h"
#include "sdf_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ the table
// the angle at corner x of a triangle, between its edges to y and to z: atan2(|e1 x e2|, e1 . e2)
__device__ __forceinline__ float corner_angle(V3 x, V3 y, V3 z) {
  const V3 e1 = y - x, e2 = z - x, k = cross(e1, e2);
  return env_atan2(sqrtf(dot(k, k)), dot(e1, e2));
}
// N / sqrtf(dot(N, N)), or zero when that length is not > 0
__device__ __forceinline__ V3 unit_or_zero(V3 n, bool* has = nullptr) {
  const float len = sqrtf(dot(n, n));
  if (has) *has = len > 0.0f;
  return len > 0.0f ? n / len : V3(0.0f);
}

__global__ __launch_bounds__(kBlock) void k_sdf_faces(SdfTableArgs a) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= a.ns) return;
  float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
  if (a.slot_feat[6 * (size_t)s] != kNone) {  // a triangle
    const float4* g = a.slots + (size_t)s * 4;
    const V3 va = ld3(g[0]), vb = ld3(g[1]), vc = ld3(g[2]);
    const V3 n = cross(vb - va, vc - va);
    const float nn = dot(n, n);
    if (nn > 0.0f) {  // (a face without a normal contributes nothing)
      const V3 u = n / sqrtf(nn);
      f0 = make_float4(u.x, u.y, u.z, 1.0f);
      f1 = make_float4(corner_angle(va, vb, vc), corner_angle(vb, vc, va), corner_angle(vc, va, vb), 0.f);
    }
  }
  a.faces[2 * (size_t)s] = f0, a.faces[2 * (size_t)s + 1] = f1;
}

__global__ __launch_bounds__(kBlock) void k_sdf_rows(SdfTableArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.ns * kSdfRows) return;
  const uint32_t s = i / kSdfRows, row = i % kSdfRows;
  V3 n(0.0f);
  if (row == kFeatFace) {
    n = ld3(a.faces[2 * (size_t)s]);
  } else {
    const uint32_t f = a.slot_feat[6 * (size_t)s + row];
    if (f != kNone) {
      for (uint32_t j = a.feat_off[f]; j < a.feat_off[f + 1]; j++) {
        const uint32_t item = a.feat_items[j], from = item >> 2, corner = item & 3u;
        const float4 u = a.faces[2 * (size_t)from];
        if (u.w == 0.0f) continue;
        if (corner == 3u) {
          n = n + ld3(u);
        } else {
          const float4 ang = a.faces[2 * (size_t)from + 1];
          n = n + (corner == 0u ? ang.x : corner == 1u ? ang.y : ang.z) * ld3(u);
        }
      }
      n = unit_or_zero(n);
    }
  }
  a.table[i] = make_float4(n.x, n.y, n.z, 0.f);
}

void launch_sdf_table(hipStream_t s, const SdfTableArgs& a) {
  if (!a.ns) return;
  hipLaunchKernelGGL(k_sdf_faces, dim3((a.ns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(k_sdf_rows, dim3((a.ns * kSdfRows + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
}

// ------------------------------------------------------------------ the signed query
template <bool CURVES, bool WIDE, bool GRID>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_signed_query(DScene sc, SignedArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  uint32_t overflow = 0u;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    float4 pt;
    if (GRID) {  // multiply, then add, each rounded once
      const uint32_t ix = i % a.dims[0], rest = i / a.dims[0], iy = rest % a.dims[1], iz = rest / a.dims[1];
      pt = make_float4(a.origin[0] + (float)ix * a.spacing[0], a.origin[1] + (float)iy * a.spacing[1], a.origin[2] + (float)iz * a.spacing[2], a.max_dist);
    } else {
      pt = a.points[i];
    }
    const V3 p(pt.x, pt.y, pt.z);
    Nearest best = nearest_none(pt);
    if (point_active(pt)) nearest_traverse<CURVES, WIDE>(sc, p, best, stk + threadIdx.x, kBlock, &overflow, a.spill + blockIdx.x * kBlock + threadIdx.x,
                                                         gridDim.x * kBlock);
    const bool found = best.slot != kNone;
    // the sign: the winning feature's pseudonormal against p - q; a curve piece has none and is outside
    float4 sd = make_float4(0.f, 0.f, 0.f, 0.f);
    if (found) {
      V3 n(0.0f);
      if (best.feat != kFeatCurve) n = ld3(a.table[(size_t)best.slot * kSdfRows + best.feat]);
      const float s = dot(p - best.q, n), d = sqrtf(best.d2);
      sd = make_float4(n.x, n.y, n.z, s < 0.0f ? -d : d);
    }
    if (GRID) {
      a.grid_sd[i] = sd.w;
      continue;
    }
    nearest_store(best, i, a.ident, a.closest);
    if (a.sd) a.sd[i] = sd;
  }
  if (overflow) *a.overflow = 1u;
}

// k_query_nearest's launch class (256 lanes, the LDS stack plus the spill area, at most kFeatureGridCap blocks); the instance is the
// hooks' (variants.h::with_hook_tree): the answer does not depend on the tree
void launch_signed(hipStream_t s, const DScene& sc, const SignedArgs& a, const Knobs& k) {
  if (!a.n) return;
  const uint32_t g = feature_grid<kBlock>(a.n);
  with_hook_tree([&](auto c, auto w) {
    if (a.grid) hipLaunchKernelGGL((k_signed_query<c, w, true>), dim3(g), dim3(kBlock), 0, s, sc, a);
    else hipLaunchKernelGGL((k_signed_query<c, w, false>), dim3(g), dim3(kBlock), 0, s, sc, a);
  }, sc, k);
}

}  // namespace pb
