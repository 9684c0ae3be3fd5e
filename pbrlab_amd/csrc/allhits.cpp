// allhits.cpp -- the all-hits entry points of the C ABI: pbrhip_trace_all (host arrays) and pbrhip_trace_all_device.
// Host C++ only; the kernel is allhits.hip's.
#include "allhits_kernels.h"
#include "query_checks.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_ray) == 32, "ray layout");
static_assert(PBRHIP_ALL_HITS_MAX == kAllHitsMax, "the list's capacity");

// what both variants check before anything touches a device or the scene: pointers and the count (check_query), then max_hits
static int check_all(const char* who, const pbrhip_scene* s, const void* rays, size_t n, uint32_t max_hits, const uint32_t* count, const uint32_t* ident) {
  if (int rc = check_query(who, s, rays, n, count, ident)) return rc;
  if (max_hits > PBRHIP_ALL_HITS_MAX) return fail(PBRHIP_EINVAL, "%s: max_hits is %u (at most %u)", who, max_hits, PBRHIP_ALL_HITS_MAX);
  if (n && !max_hits && !count) return fail(PBRHIP_EINVAL, "%s: NULL count with max_hits == 0", who);
  if ((uint64_t)n * max_hits >= (1ull << 31)) return fail(PBRHIP_EINVAL, "%s: too many list entries (n * max_hits = %llu; fewer than 2^31)", who, (unsigned long long)n * max_hits);
  return PBRHIP_OK;
}

// the launch on the scene's stream; device pointers on the scene's device, either output may be null
static int all_impl(pbrhip_scene* s, const void* d_rays, size_t n, uint32_t max_hits, uint32_t* d_count, uint32_t* d_ident) {
  const Knobs k = read_knobs();
  if (int rc = prepare_traversal(s)) return rc;
  AllHitsArgs a{};
  a.rays = static_cast<const float4*>(d_rays), a.n = (uint32_t)n, a.k = max_hits;
  a.count = d_count, a.ident = max_hits ? reinterpret_cast<uint4*>(d_ident) : nullptr;
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  launch_all_hits(s->stream, s->dscene, a, k);
  return finish_traversal(s);
}

extern "C" int pbrhip_trace_all_device(pbrhip_scene* s, const void* d_rays, size_t n, uint32_t max_hits, void* stream, uint32_t* d_count, uint32_t* d_ident) {
  return guarded([&]() -> int {
    const char* who = "trace_all_device";
    if (int rc = check_all(who, s, d_rays, n, max_hits, d_count, d_ident)) return rc;
    if (int rc = check_aligned(who, d_rays, max_hits ? d_ident : nullptr, nullptr)) return rc;
    if (reinterpret_cast<uintptr_t>(d_count) & 3u) return fail(PBRHIP_EINVAL, "%s: d_count is not 4-byte aligned", who);
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    return all_impl(s, d_rays, n, max_hits, d_count, d_ident);
  });
}

extern "C" int pbrhip_trace_all(pbrhip_scene* s, const pbrhip_ray* rays, size_t n, uint32_t max_hits, uint32_t* count, uint32_t* ident) {
  return guarded([&]() -> int {
    if (int rc = check_all("trace_all", s, rays, n, max_hits, count, ident)) return rc;
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (!max_hits) ident = nullptr;
    const size_t words = 4 * n * max_hits;
    DevBuf<float4> d_rays;
    DevBuf<uint32_t> d_cnt, d_id;
    HIPCHK(d_rays.reserve(2 * n));
    if (count) HIPCHK(d_cnt.reserve(n));
    if (ident) HIPCHK(d_id.reserve(words));
    HIPCHK(hipMemcpyAsync(d_rays.p, rays, n * sizeof(pbrhip_ray), hipMemcpyHostToDevice, s->stream));
    if (int rc = all_impl(s, d_rays.p, n, max_hits, d_cnt.p, d_id.p)) return rc;
    if (count) HIPCHK(hipMemcpyAsync(count, d_cnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (ident) HIPCHK(hipMemcpyAsync(ident, d_id.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}
