// sdf.cpp -- the signed-distance entry points of the C ABI: the topology lists and the pseudonormal table of a committed
// scene, the signed nearest-point queries (host, device and grid variants) and the table's test hook.  Host C++ only; the kernels are
// sdf.hip's, the adjacency sdf_topology.cpp's.
#include <chrono>

#include "query_checks.h"
#include "scene_impl.h"
#include "sdf_kernels.h"
#include "sdf_topology.h"

using namespace pb;

static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The lists, once per commit: the model's position indices in canonical (instance, geom, prim, sub) order -- commit.cpp::flatten_prims'
// order, the index is the gid -- against the committed slot order.
static int ensure_topology(pbrhip_scene* s) {
  SdfState& d = s->sdf;
  if (d.topology) return PBRHIP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t ns = s->tree.num_slots;
  std::vector<uint32_t> object, vid;
  uint32_t nobjects = 0;
  for (uint32_t i = 0; i < s->instances.size(); i++)
    for (uint32_t g = 0; g < s->instances[i].material_ids.size(); g++, nobjects++) {
      const HostMesh& m = *inst_mesh(s, i, g);
      for (uint32_t p = 0; p < m.num_prims(); p++) {
        if (m.kind == 0) {
          object.push_back(nobjects);
          for (int c = 0; c < 3; c++) vid.push_back(m.vid[3 * (size_t)p + c]);
        } else {
          object.insert(object.end(), 4, kSdfNone);  // four pieces per cubic
          vid.insert(vid.end(), 12, 0u);
        }
      }
    }
  if (object.size() != ns || s->slot_gid.size() != ns) return fail(PBRHIP_ESTATE, "signed distance: the model no longer has the committed topology");
  SdfTopology topo;
  if (!build_sdf_topology(ns, s->slot_gid.data(), object.data(), vid.data(), &topo)) return fail(PBRHIP_ESTATE, "signed distance: the committed slot order is no permutation of the model's primitives");
  HIPCHK(d.slot_feat.upload(topo.slot_feat, s->stream));
  HIPCHK(d.feat_off.upload(topo.feat_off, s->stream));
  HIPCHK(d.feat_items.upload(topo.feat_items, s->stream));
  HIPCHK(d.faces.reserve(2 * (size_t)ns));
  HIPCHK(d.table.reserve(kSdfRows * (size_t)ns));
  HIPCHK(hipStreamSynchronize(s->stream));  // (topo's vectors go out of scope)
  d.info = pbrhip_sd_info{};
  d.info.triangles = topo.report.triangles, d.info.vertices = topo.report.vertices;
  d.info.edges_manifold = topo.report.edges_manifold, d.info.edges_boundary = topo.report.edges_boundary;
  d.info.edges_nonmanifold = topo.report.edges_nonmanifold, d.info.edges_inconsistent = topo.report.edges_inconsistent;
  d.info.table_bytes = 4ull * (topo.slot_feat.size() + topo.feat_off.size() + topo.feat_items.size()) + 16ull * (2 + kSdfRows) * ns;
  d.info.topology_ms = ms_since(t0);
  d.topology = true, d.table_valid = false;
  return PBRHIP_OK;
}

// The table, once per commit or refit, from the slots as the device holds them.  The caller has checked that the scene is committed and
// not stale and has selected its device.
static int ensure_table(pbrhip_scene* s) {
  if (s->replica) return fail(PBRHIP_ESTATE, "signed distance: a replica holds no geometry (ask the source scene)");
  if (int rc = ensure_topology(s)) return rc;
  SdfState& d = s->sdf;
  if (d.table_valid) return PBRHIP_OK;
  HIPCHK(hipStreamSynchronize(s->stream));
  const auto t0 = std::chrono::steady_clock::now();
  SdfTableArgs a{};
  a.slots = s->dscene.slots, a.ns = s->tree.num_slots;
  a.slot_feat = d.slot_feat.p, a.feat_off = d.feat_off.p, a.feat_items = d.feat_items.p;
  a.faces = d.faces.p, a.table = d.table.p;
  launch_sdf_table(s->stream, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  d.info.table_ms = ms_since(t0);
  d.table_valid = true;
  return PBRHIP_OK;
}

// the launch on the scene's stream; device pointers on the scene's device
static int signed_impl(pbrhip_scene* s, SignedArgs a) {
  const Knobs k = read_knobs();
  if (int rc = ensure_table(s)) return rc;
  if (int rc = prepare_traversal(s)) return rc;
  a.table = s->sdf.table.p;
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  launch_signed(s->stream, s->dscene, a, k);
  return finish_traversal(s);
}
static SignedArgs point_args(const void* d_points, size_t n, uint32_t* d_ident, float* d_closest, float* d_sd) {
  SignedArgs a{};
  a.points = static_cast<const float4*>(d_points), a.n = (uint32_t)n;
  a.ident = reinterpret_cast<uint4*>(d_ident), a.closest = reinterpret_cast<float4*>(d_closest), a.sd = reinterpret_cast<float4*>(d_sd);
  return a;
}

extern "C" int pbrhip_scene_signed_distance_info(pbrhip_scene* s, pbrhip_sd_info* out) {
  return guarded([&]() -> int {
    if (!s || !out) return fail(PBRHIP_EINVAL, "scene_signed_distance_info: NULL %s", s ? "output" : "scene");
    if (int rc = check_state(s, 1)) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = ensure_table(s)) return rc;
    *out = s->sdf.info;
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_signed_distance_device(pbrhip_scene* s, const void* d_points, size_t n, void* stream, uint32_t* d_ident, float* d_closest, float* d_sd) {
  return guarded([&]() -> int {
    const char* who = "signed_distance_device";
    if (int rc = check_query(who, s, d_points, n, d_ident ? static_cast<void*>(d_ident) : static_cast<void*>(d_closest), d_sd)) return rc;
    if (int rc = check_aligned(who, d_points, d_ident, d_closest, d_sd)) return rc;
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    if (s->replica) return fail(PBRHIP_ESTATE, "signed distance: a replica holds no geometry (ask the source scene)");
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    return signed_impl(s, point_args(d_points, n, d_ident, d_closest, d_sd));
  });
}

extern "C" int pbrhip_signed_distance(pbrhip_scene* s, const pbrhip_point* points, size_t n, uint32_t* ident, float* closest, float* sd) {
  return guarded([&]() -> int {
    if (int rc = check_query("signed_distance", s, points, n, ident ? static_cast<void*>(ident) : static_cast<void*>(closest), sd)) return rc;
    if (int rc = check_state(s, n)) return rc < 0 ? rc : PBRHIP_OK;
    if (s->replica) return fail(PBRHIP_ESTATE, "signed distance: a replica holds no geometry (ask the source scene)");
    HIPCHK(hipSetDevice(s->device));
    DevBuf<float4> d_pts, d_cl, d_sd;
    DevBuf<uint32_t> d_id;
    HIPCHK(d_pts.reserve(n));
    if (ident) HIPCHK(d_id.reserve(4 * n));
    if (closest) HIPCHK(d_cl.reserve(n));
    if (sd) HIPCHK(d_sd.reserve(n));
    HIPCHK(hipMemcpyAsync(d_pts.p, points, n * sizeof(pbrhip_point), hipMemcpyHostToDevice, s->stream));
    if (int rc = signed_impl(s, point_args(d_pts.p, n, d_id.p, reinterpret_cast<float*>(d_cl.p), reinterpret_cast<float*>(d_sd.p)))) return rc;
    if (ident) HIPCHK(hipMemcpyAsync(ident, d_id.p, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (closest) HIPCHK(hipMemcpyAsync(closest, d_cl.p, 4 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (sd) HIPCHK(hipMemcpyAsync(sd, d_sd.p, 4 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_signed_distance_grid_device(pbrhip_scene* s, const float* origin, const float* spacing, const uint32_t* dims, float max_dist,
                                                  void* stream, float* d_sd) {
  return guarded([&]() -> int {
    const char* who = "signed_distance_grid_device";
    if (!s) return fail(PBRHIP_EINVAL, "%s: NULL scene", who);
    if (!origin || !spacing || !dims) return fail(PBRHIP_EINVAL, "%s: NULL origin, spacing or dims", who);
    uint64_t n = 1;
    for (int a = 0; a < 3; a++) {
      n *= dims[a];
      if (n >= (1ull << 31)) return fail(PBRHIP_EINVAL, "%s: too many grid points (fewer than 2^31)", who);
    }
    if (n && !d_sd) return fail(PBRHIP_EINVAL, "%s: NULL output", who);
    if (reinterpret_cast<uintptr_t>(d_sd) & 3u) return fail(PBRHIP_EINVAL, "%s: d_sd is not 4-byte aligned", who);
    if (int rc = check_state(s, (size_t)n)) return rc < 0 ? rc : PBRHIP_OK;
    if (s->replica) return fail(PBRHIP_ESTATE, "signed distance: a replica holds no geometry (ask the source scene)");
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;  // (d_sd may still be read by what the caller's stream holds)
    SignedArgs a{};
    a.n = (uint32_t)n, a.grid = 1u, a.max_dist = max_dist, a.grid_sd = d_sd;
    for (int k = 0; k < 3; k++) a.origin[k] = origin[k], a.spacing[k] = spacing[k], a.dims[k] = dims[k];
    return signed_impl(s, a);
  });
}

extern "C" int pbrhip_scene_read_pseudonormals(pbrhip_scene* s, float* out, uint32_t* num_slots) {
  return guarded([&]() -> int {
    if (!s) return fail(PBRHIP_EINVAL, "scene_read_pseudonormals: scene is NULL");
    if (int rc = check_state(s, 1)) return rc;
    const uint32_t ns = s->tree.num_slots;
    if (num_slots) *num_slots = ns;
    if (!out) return PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = ensure_table(s)) return rc;
    if (ns) HIPCHK(hipMemcpyAsync(out, s->sdf.table.p, (size_t)ns * kSdfRows * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}
