// query.hip -- ray and nearest-point queries answered from device memory (pbrhip_trace_closest_device, pbrhip_trace_any_device,
// pbrhip_nearest_point, pbrhip_nearest_point_device).
//
//   k_query_closest / k_query_any   the production traversal (dtrace_pv.h::trace_pv) fed from the caller's ray array through a sink of
//                                   its own (kernels.hip::HookSink is the pattern): k_hook_pv's shape -- persistent waves, one queue
//                                   head, the phase-voting loop --, so the hits are pbrhip_trace_closest's bit for bit.  An inactive ray
//                                   (dtrace.h::ray_active) is replaced by a certain miss before it is traced.
//   k_query_nearest                 one query per lane, k_features' shape (256 lanes, kSimpleLdsStack stack entries per lane in LDS, the
//                                   rest in the spill area, four blocks per CU): a traversal by distance, children in ascending order of
//                                   the squared distance L from the point to their stored box, a box skipped only when L exceeds the
//                                   best D2 so far.  The contract makes D2 >= L for every stored box above a primitive,
//                                   so the answer is a property of (point, primitive set) alone: builder, tree, refit and visiting order
//                                   do not show.  The contract, the leaf tests and the traversal are dnearest.h's, which
//                                   sdf.hip's signed queries include as well.
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction.
#include <type_traits>

#include "dnearest.h"
#include "dshade.h"
#include "dtrace_pv.h"
#include "feature_kernels.h"
#include "query_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ ray queries
// An inactive ray becomes rays.hip's certain miss: tmin = FLT_MAX > tmax = 0 fails every primitive test (t > tmin && t <= tmax) and every
// slab test of a finite box (exit >= tmin); whatever the traversal returns for it, done() reports a miss.
struct QuerySink {
  static constexpr bool kWalk = false, kSplit = false, kSuspend = false;
  const DScene& sc;
  const float4* rays;
  uint4* ident;
  HookHit* hits;
  uint8_t* occ;
  __device__ __forceinline__ bool load(uint32_t idx, uint32_t& tag, V3& o, V3& d, float& tmin, float& tmax) const {
    tag = idx;
    const float4 o4 = rays[2 * idx], d4 = rays[2 * idx + 1];
    if (ray_active(o4, d4)) o = ld3(o4), d = ld3(d4), tmin = o4.w, tmax = fminf(d4.w, INFINITY);  // raytracer_impl.cc:256
    else o = V3(0.0f, 0.0f, 0.0f), d = V3(0.0f, 0.0f, 1.0f), tmin = kFltMax, tmax = 0.0f;
    return occ != nullptr;
  }
  __device__ __forceinline__ void done(uint32_t i, const Hit& h, bool occluded) const {
    const float4 o4 = rays[2 * i], d4 = rays[2 * i + 1];
    const bool active = ray_active(o4, d4);
    if (occ) {
      occ[i] = (active && occluded) ? 1 : 0;
      return;
    }
    Hit r = h;
    if (!active) r.slot = kNone;
    if (ident) ident[i] = r.slot != kNone ? make_uint4(r.slot & kHitSlotMask, __float_as_uint(r.u), __float_as_uint(r.v), __float_as_uint(r.t)) : make_uint4(kNone, 0u, 0u, 0u);
    if (hits) hits[i] = hook_result(sc, ld3(o4), ld3(d4), r);
  }
};
template <bool ANY, bool CURVES, bool WIDE>  // CURVES / WIDE: the variant k_trace runs for this scene
__global__ __launch_bounds__(kBlock) void k_query_pv(DScene sc, RayQueryArgs a) {
  __shared__ uint32_t stk[pv_lds_stack<CURVES, WIDE>() * kBlock];
  __shared__ float frm[CURVES ? 10 * kBlock : 1];
  TravStats st = {};
  uint32_t overflow = 0u;
  QuerySink sink = {sc, a.rays, a.ident, a.hits, a.occ};
  trace_pv<ANY ? 1 : 0, false, CURVES, WIDE>(sc, a.n, &a.counts[kCntHead], sink, stk + threadIdx.x, kBlock, a.spill + blockIdx.x * kBlock + threadIdx.x,
                                             gridDim.x * kBlock, st, &overflow, CURVES ? frm + threadIdx.x : nullptr);
  if (overflow) a.counts[kCntOverflow] = 1u;
}

// ------------------------------------------------------------------ nearest point: the contract and its traversal are dnearest.h's
template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_query_nearest(DScene sc, NearestArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  uint32_t overflow = 0u;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock) {
    const float4 pt = a.points[i];
    Nearest best = nearest_none(pt);
    if (point_active(pt)) nearest_traverse<CURVES, WIDE>(sc, V3(pt.x, pt.y, pt.z), best, stk + threadIdx.x, kBlock, &overflow,
                                                         a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
    nearest_store(best, i, a.ident, a.closest);
  }
  if (overflow) *a.overflow = 1u;
}

// ------------------------------------------------------------------ launches
// the <CURVES, WIDE> of the tree the render of this scene walks (kernels.hip::launch_trace): PBRHIP_WIDE=0 selects the binary tree, and
// unlike the hooks' a binary tree without curves has an instance without the curve code: all four combinations (variants.h::with_flags)

void launch_ray_query(hipStream_t s, const DScene& sc, const RayQueryArgs& a, const Knobs& k) {
  if (!a.n) return;
  uint32_t g = (a.n + kBlock - 1) / kBlock;
  g = g < kTraceGridCap ? g : kTraceGridCap;  // (k_hook_pv's grid: the spill area is sized by it)
  with_flags([&](auto any, auto c, auto w) { hipLaunchKernelGGL((k_query_pv<any, c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, a.occ != nullptr,
             sc.num_curves != 0, use_wide(sc, k));
}

void launch_nearest(hipStream_t s, const DScene& sc, const NearestArgs& a, const Knobs& k) {
  if (!a.n) return;
  const uint32_t g = feature_grid<kBlock>(a.n);
  with_flags([&](auto c, auto w) { hipLaunchKernelGGL((k_query_nearest<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, sc.num_curves != 0, use_wide(sc, k));
}

}  // namespace pb
