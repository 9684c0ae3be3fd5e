// knearest.cpp -- the k-nearest entry points of the C ABI: pbrhip_k_nearest (host arrays) and pbrhip_k_nearest_device.
// Host C++ only; the kernel is knearest.hip's.
#include "knearest_kernels.h"
#include "query_checks.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_point) == 16, "point layout");
static_assert(PBRHIP_K_NEAREST_MAX == kKNearestMax, "the list's capacity");

// what both variants check before anything touches a device or the scene: pointers and the count (check_query), then max_k and closest
static int check_knn(const char* who, const pbrhip_scene* s, const void* points, size_t n, uint32_t max_k, const uint32_t* count, const uint32_t* ident,
                     const float* closest) {
  if (int rc = check_query(who, s, points, n, count, ident)) return rc;
  if (max_k && closest && !ident) return fail(PBRHIP_EINVAL, "%s: closest with a NULL ident (the list lives in the ident rows)", who);
  if (max_k > PBRHIP_K_NEAREST_MAX) return fail(PBRHIP_EINVAL, "%s: max_k is %u (at most %u)", who, max_k, PBRHIP_K_NEAREST_MAX);
  if (n && !max_k && !count) return fail(PBRHIP_EINVAL, "%s: NULL count with max_k == 0", who);
  if ((uint64_t)n * max_k >= (1ull << 31)) return fail(PBRHIP_EINVAL, "%s: too many list entries (n * max_k = %llu; fewer than 2^31)", who, (unsigned long long)n * max_k);
  return PBRHIP_OK;
}
// ... then the scene's state: check_state's, and a replica is refused (no multi-GPU twin: ask the source scene)
static int check_knn_state(const pbrhip_scene* s, size_t n) {
  if (s->replica) return fail(PBRHIP_ESTATE, "k-nearest: a replica is refused (ask the source scene)");
  return check_state(s, n);
}

// the launch on the scene's stream; device pointers on the scene's device, any output may be null (closest only beside ident)
static int knn_impl(pbrhip_scene* s, const void* d_points, size_t n, uint32_t max_k, uint32_t* d_count, uint32_t* d_ident, float* d_closest) {
  const Knobs k = read_knobs();
  if (int rc = prepare_traversal(s)) return rc;
  KNearestArgs a{};
  a.points = static_cast<const float4*>(d_points), a.n = (uint32_t)n, a.k = max_k;
  a.count = d_count, a.ident = max_k ? reinterpret_cast<uint4*>(d_ident) : nullptr;
  a.closest = a.ident ? reinterpret_cast<float4*>(d_closest) : nullptr;
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  launch_k_nearest(s->stream, s->dscene, a, k);
  return finish_traversal(s);
}

extern "C" int pbrhip_k_nearest_device(pbrhip_scene* s, const void* d_points, size_t n, uint32_t max_k, void* stream, uint32_t* d_count, uint32_t* d_ident,
                                       float* d_closest) {
  return guarded([&]() -> int {
    const char* who = "k_nearest_device";
    if (int rc = check_knn(who, s, d_points, n, max_k, d_count, d_ident, d_closest)) return rc;
    if (int rc = check_aligned(who, d_points, max_k ? d_ident : nullptr, max_k ? d_closest : nullptr)) return rc;
    if (reinterpret_cast<uintptr_t>(d_count) & 3u) return fail(PBRHIP_EINVAL, "%s: d_count is not 4-byte aligned", who);
    if (int rc = check_knn_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    return knn_impl(s, d_points, n, max_k, d_count, d_ident, d_closest);
  });
}

extern "C" int pbrhip_k_nearest(pbrhip_scene* s, const pbrhip_point* points, size_t n, uint32_t max_k, uint32_t* count, uint32_t* ident, float* closest) {
  return guarded([&]() -> int {
    if (int rc = check_knn("k_nearest", s, points, n, max_k, count, ident, closest)) return rc;
    if (int rc = check_knn_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (!max_k) ident = nullptr, closest = nullptr;
    const size_t words = 4 * n * max_k;
    DevBuf<float4> d_pts;
    DevBuf<uint32_t> d_cnt, d_id;
    DevBuf<float> d_cl;
    HIPCHK(d_pts.reserve(n));
    if (count) HIPCHK(d_cnt.reserve(n));
    if (ident) HIPCHK(d_id.reserve(words));
    if (closest) HIPCHK(d_cl.reserve(words));
    HIPCHK(hipMemcpyAsync(d_pts.p, points, n * sizeof(pbrhip_point), hipMemcpyHostToDevice, s->stream));
    if (int rc = knn_impl(s, d_pts.p, n, max_k, d_cnt.p, d_id.p, d_cl.p)) return rc;
    if (count) HIPCHK(hipMemcpyAsync(count, d_cnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (ident) HIPCHK(hipMemcpyAsync(ident, d_id.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (closest) HIPCHK(hipMemcpyAsync(closest, d_cl.p, words * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}
