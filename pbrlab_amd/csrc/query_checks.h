// query_checks.h -- what every query entry point (query.cpp, sdf.cpp) checks before anything touches a device or the scene.
#pragma once

#include "scene_impl.h"

namespace pb {

// pointers, then the count
inline int check_query(const char* who, const pbrhip_scene* s, const void* in, size_t n, const void* out_a, const void* out_b) {
  if (!s) return fail(PBRHIP_EINVAL, "%s: NULL scene", who);
  if (n && !in) return fail(PBRHIP_EINVAL, "%s: NULL input array", who);
  if (n && !out_a && !out_b) return fail(PBRHIP_EINVAL, "%s: NULL output", who);
  if (n >= (1ull << 31)) return fail(PBRHIP_EINVAL, "%s: too many queries (%zu; fewer than 2^31)", who, n);
  return PBRHIP_OK;
}
// the kernels move 16 bytes at a time: a device pointer that is not 16-byte aligned is refused (null: not wanted)
inline int check_aligned(const char* who, const void* a, const void* b, const void* c, const void* d = nullptr) {
  for (const void* p : {a, b, c, d})
    if (reinterpret_cast<uintptr_t>(p) & 15u) return fail(PBRHIP_EINVAL, "%s: a device pointer is not 16-byte aligned", who);
  return PBRHIP_OK;
}
// ... then the scene's state.  Returns 1 for "nothing to do" (n == 0 on a scene that could answer).
inline int check_state(const pbrhip_scene* s, size_t n) {
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  return n ? PBRHIP_OK : 1;
}

}  // namespace pb
