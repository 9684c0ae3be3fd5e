// query.hip -- ray and nearest-point queries answered from device memory (pbrhip_trace_closest_device, pbrhip_trace_any_device,
// pbrhip_nearest_point, pbrhip_nearest_point_device).
//
//   k_query_closest / k_query_any   the production traversal (dtrace_pv.h::trace_pv) fed from the caller's ray array through a sink of
//                                   its own (kernels.hip::HookSink is the pattern): k_hook_pv's shape -- persistent waves, one queue
//                                   head, the phase-voting loop --, so the hits are pbrhip_trace_closest's bit for bit.  An inactive ray
//                                   (ray_active, rays.hip's predicate restated) is replaced by a certain miss before it is traced.
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

// rays.hip::ray_active, restated: eight numbers, none NaN, origin and direction finite, a direction other than zero, 0 <= tmin <= tmax
// (tmax may be +inf)
__device__ __forceinline__ bool ray_active(const float4& o, const float4& d) {
  const bool finite = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z);
  const bool nonzero = d.x != 0.0f || d.y != 0.0f || d.z != 0.0f;
  return finite && nonzero && o.w >= 0.0f && d.w >= o.w;  // (a NaN tmin or tmax fails both comparisons)
}

// ------------------------------------------------------------------ ray queries
// kernels.hip::hook_result: TraceResult of a hit (raytracer.h:9-17), its defaults for a miss
__device__ __forceinline__ HookHit query_result(const DScene& sc, V3 o, V3 d, const Hit& h) {
  HookHit r;
  r.ng[0] = 1.f, r.ng[1] = 0.f, r.ng[2] = 0.f, r.t = 1.f, r.u = 0.f, r.v = 0.f;
  r.instance_id = r.geom_id = r.prim_id = kNone;
  if (h.slot != kNone) {
    Surface s = make_surface(sc, o, d, h);
    const ShadeRec& sr = sc.shade[h.slot & kHitSlotMask];
    r.ng[0] = s.n_g.x, r.ng[1] = s.n_g.y, r.ng[2] = s.n_g.z;
    r.t = h.t, r.u = h.u, r.v = h.v;
    r.instance_id = sr.instance_id, r.geom_id = sr.geom_id, r.prim_id = sr.prim_id;
  }
  return r;
}
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
    if (hits) hits[i] = query_result(sc, ld3(o4), ld3(d4), r);
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
    Nearest best;
    best.d2 = pt.w * pt.w, best.u = 0.0f, best.v = 0.0f, best.q = V3(0.0f), best.slot = kNone, best.feat = kFeatCurve;
    const bool active = point_active(pt);
    if (active) nearest_traverse<CURVES, WIDE>(sc, V3(pt.x, pt.y, pt.z), best, stk + threadIdx.x, kBlock, &overflow,
                                               a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
    const bool found = best.slot != kNone;
    if (a.ident) a.ident[i] = found ? make_uint4(best.slot, __float_as_uint(best.u), __float_as_uint(best.v), __float_as_uint(sqrtf(best.d2))) : make_uint4(kNone, 0u, 0u, 0u);
    if (a.closest) a.closest[i] = found ? make_float4(best.q.x, best.q.y, best.q.z, best.d2) : make_float4(0.f, 0.f, 0.f, 0.f);
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

static_assert((size_t)(kStackDepth - kSimpleLdsStack) * kFeatureGridCap * kBlock <= kSpillWords, "k_query_nearest's spill area (one stack per thread of its grid)");
void launch_nearest(hipStream_t s, const DScene& sc, const NearestArgs& a, const Knobs& k) {
  if (!a.n) return;
  uint32_t g = (a.n + kBlock - 1) / kBlock;
  g = g < kFeatureGridCap ? g : kFeatureGridCap;
  with_flags([&](auto c, auto w) { hipLaunchKernelGGL((k_query_nearest<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, sc.num_curves != 0, use_wide(sc, k));
}

}  // namespace pb
