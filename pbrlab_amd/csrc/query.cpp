// query.cpp -- the query entry points of the C ABI: ray queries on device memory and nearest-point queries, host and
// device variants.  Host C++ only; the kernels are query.hip's.
#include "query_checks.h"
#include "query_kernels.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_hit) == sizeof(HookHit), "hit layout");
static_assert(sizeof(pbrhip_ray) == 32, "ray layout");
static_assert(sizeof(pbrhip_point) == 16, "point layout");

// (what every query checks before anything touches a device or the scene -- check_query, check_aligned, check_state --: query_checks.h;
// wait_for_caller_stream in front of a caller's device array, prepare_traversal and finish_traversal around the launch: scene_impl.h)

// ------------------------------------------------------------------ ray queries on device memory
static int ray_query_device(const char* who, pbrhip_scene* s, const void* d_rays, size_t n, void* stream, uint32_t* d_ident, pbrhip_hit* d_hits,
                            uint8_t* d_occ) {
  if (int rc = check_query(who, s, d_rays, n, d_occ ? static_cast<void*>(d_occ) : static_cast<void*>(d_ident), d_occ ? nullptr : d_hits)) return rc;
  if (int rc = check_aligned(who, d_rays, d_ident, nullptr)) return rc;
  if (reinterpret_cast<uintptr_t>(d_hits) & 3u) return fail(PBRHIP_EINVAL, "%s: d_hits is not 4-byte aligned", who);
  if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  if (int rc = wait_for_caller_stream(s, stream)) return rc;
  if (int rc = prepare_traversal(s)) return rc;
  RayQueryArgs a{};
  a.rays = static_cast<const float4*>(d_rays), a.n = (uint32_t)n;
  a.ident = reinterpret_cast<uint4*>(d_ident), a.hits = reinterpret_cast<HookHit*>(d_hits), a.occ = d_occ;
  a.counts = s->counts.p, a.spill = s->spill.p;
  launch_ray_query(s->stream, s->dscene, a, k);
  return finish_traversal(s);
}

extern "C" int pbrhip_trace_closest_device(pbrhip_scene* s, const void* d_rays, size_t n, void* stream, uint32_t* d_ident, pbrhip_hit* d_hits) {
  return guarded([&]() -> int { return ray_query_device("trace_closest_device", s, d_rays, n, stream, d_ident, d_hits, nullptr); });
}

extern "C" int pbrhip_trace_any_device(pbrhip_scene* s, const void* d_rays, size_t n, void* stream, uint8_t* d_occluded) {
  return guarded([&]() -> int { return ray_query_device("trace_any_device", s, d_rays, n, stream, nullptr, nullptr, d_occluded); });
}

// ------------------------------------------------------------------ nearest-point queries
// the launch on the scene's stream; device pointers on the scene's device, either output may be null
static int nearest_impl(pbrhip_scene* s, const void* d_points, size_t n, uint32_t* d_ident, float* d_closest) {
  const Knobs k = read_knobs();
  if (int rc = prepare_traversal(s)) return rc;
  NearestArgs a{};
  a.points = static_cast<const float4*>(d_points), a.n = (uint32_t)n;
  a.ident = reinterpret_cast<uint4*>(d_ident), a.closest = reinterpret_cast<float4*>(d_closest);
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  launch_nearest(s->stream, s->dscene, a, k);
  return finish_traversal(s);
}

extern "C" int pbrhip_nearest_point_device(pbrhip_scene* s, const void* d_points, size_t n, void* stream, uint32_t* d_ident, float* d_closest) {
  return guarded([&]() -> int {
    if (int rc = check_query("nearest_point_device", s, d_points, n, d_ident, d_closest)) return rc;
    if (int rc = check_aligned("nearest_point_device", d_points, d_ident, d_closest)) return rc;
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    return nearest_impl(s, d_points, n, d_ident, d_closest);
  });
}

extern "C" int pbrhip_nearest_point(pbrhip_scene* s, const pbrhip_point* points, size_t n, uint32_t* ident, float* closest) {
  return guarded([&]() -> int {
    if (int rc = check_query("nearest_point", s, points, n, ident, closest)) return rc;
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    DevBuf<float4> d_pts, d_cl;
    DevBuf<uint32_t> d_id;
    HIPCHK(d_pts.reserve(n));
    if (ident) HIPCHK(d_id.reserve(4 * n));
    if (closest) HIPCHK(d_cl.reserve(n));
    HIPCHK(hipMemcpyAsync(d_pts.p, points, n * sizeof(pbrhip_point), hipMemcpyHostToDevice, s->stream));
    if (int rc = nearest_impl(s, d_pts.p, n, d_id.p, reinterpret_cast<float*>(d_cl.p))) return rc;
    if (ident) HIPCHK(hipMemcpyAsync(ident, d_id.p, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (closest) HIPCHK(hipMemcpyAsync(closest, d_cl.p, 4 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}
