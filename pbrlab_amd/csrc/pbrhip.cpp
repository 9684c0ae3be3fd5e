// pbrhip.cpp -- C ABI (include/pbrhip.h): host scene store, model edits, getters, environment, camera and the wavefront render loop
// that drives kernels.hip.  Commit and refit live in commit.cpp, the test hooks in hooks.cpp, the image-space entry points (features,
// filters, motion, emission) in image.cpp, the queries in query.cpp.  Host C++ only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "env_tables.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_principled_param) == sizeof(PrincipledParam), "param layout");
static_assert(sizeof(pbrhip_hair_param) == sizeof(HairParam), "param layout");

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int g_device = 0;

int pb::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int pb::current_device() { return g_device; }

extern "C" const char* pbrhip_last_error(void) { return g_err.c_str(); }
extern "C" uint32_t pbrhip_abi_version(void) { return PBRHIP_ABI_VERSION; }
extern "C" uint32_t pbrhip_math_mode(void) { return pb::kMathMode; }
extern "C" size_t pbrhip_sizeof_render_stats(void) { return sizeof(pbrhip_render_stats); }

extern "C" int pbrhip_device_count(int* count) {
  if (!count) return fail(PBRHIP_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(PBRHIP_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return PBRHIP_OK;
}
extern "C" int pbrhip_set_device(int device) {
  int n = 0;
  int rc = pbrhip_device_count(&n);
  if (rc) return rc;
  if (device < 0 || device >= n) return fail(PBRHIP_EINVAL, "device %d out of range (%d devices)", device, n);
  g_device = device;
  return PBRHIP_OK;
}

// ------------------------------------------------------------------ knobs (knobs.h)
Knobs pb::read_knobs() {
  auto env = [](const char* name) -> const char* { return getenv(name); };
  auto u32 = [&](const char* name, uint32_t dflt) { const char* e = env(name); return e ? (uint32_t)strtoul(e, nullptr, 10) : dflt; };
  auto not_zero = [&](const char* name) { const char* e = env(name); return !(e && atoi(e) == 0); };  // (atoi: a non-number is 0 too)
  Knobs k;
  if (const char* e = env("PBRHIP_BVH")) k.bvh = strcmp(e, "gpu-wide") == 0 ? PBRHIP_BVH_GPU_LBVH_WIDE : (strcmp(e, "gpu") == 0 ? PBRHIP_BVH_GPU_LBVH : PBRHIP_BVH_HOST_SAH);
  k.wide = not_zero("PBRHIP_WIDE");
  k.bvh_reinsert = u32("PBRHIP_BVH_REINSERT", 1u) != 0u;
  k.bvh_reinsert_top = u32("PBRHIP_BVH_REINSERT_TOP", kReinsertTop);
  k.bvh_cost = u32("PBRHIP_BVH_COST", 1u) != 0u;
  k.sss_entry = u32("PBRHIP_SSS_ENTRY", 1u) != 0u;
  k.sss_foreign = u32("PBRHIP_SSS_FOREIGN", 3u);
  k.shadow_grid = std::min(u32("PBRHIP_SHADOW_GRID", 64u), kShaftMaxRes);
  k.shadow_grid_list = std::min(u32("PBRHIP_SHADOW_GRID_LIST", kShaftMaxList), kShaftMaxList);
  k.debug = env("PBRHIP_DEBUG") != nullptr;
  k.pixel_tile = u32("PBRHIP_PIXEL_TILE", 8u);
  k.patch_shuffle = u32("PBRHIP_PATCH_SHUFFLE", 1u) != 0u;
  if (const char* e = env("PBRHIP_PASS_RUN")) k.pass_run = std::max(1u, (uint32_t)strtoul(e, nullptr, 10));
  k.groups = env("PBRHIP_GROUPS");
  if (const char* e = env("PBRHIP_TAIL_PATHS")) k.tail_paths = (uint32_t)strtoul(e, nullptr, 10);
  if (const char* e = env("PBRHIP_STREAMS")) k.streams = (uint32_t)atoi(e);
  k.window = std::max(1u, u32("PBRHIP_WINDOW", k.groups ? 1u : (uint32_t)kMaxGroups));
  k.bulk_div = u32("PBRHIP_BULK_DIV", 0u);
  k.pipe_depth = std::min(std::max(1u, u32("PBRHIP_PIPE_DEPTH", 2u)), kRingSlots - 1u);
  k.pipe_depth_small = std::min(std::max(1u, u32("PBRHIP_PIPE_DEPTH_SMALL", 8u)), kRingSlots - 1u);
  if (const char* e = env("PBRHIP_PIPE_STOP")) k.pipe_stop = atof(e);
  k.trace_sched = env("PBRHIP_TRACE_SCHED") != nullptr;
  k.wave_log = env("PBRHIP_WAVE_LOG");
  k.pv_stats = env("PBRHIP_PV_STATS") != nullptr;
  k.susp_turns = u32("PBRHIP_SUSP_TURNS", 24u);
  k.shadow_first = u32("PBRHIP_SHADOW_FIRST", 1u);
  k.first_direct = u32("PBRHIP_FIRST_DIRECT", 1u) != 0u;
  k.direct = u32("PBRHIP_DIRECT", 1u) != 0u;
  k.sss_walk = u32("PBRHIP_SSS_WALK", 1u) != 0u;
  k.wide_walk = not_zero("PBRHIP_WIDE_WALK");
  k.rays_per_wave = u32("PBRHIP_RAYS_PER_WAVE", 4u);
  k.trace_blocks = u32("PBRHIP_TRACE_BLOCKS", 0u);
  if (const char* e = env("PBRHIP_TRACE_BLOCKS_SMALL")) {  // (present at all: the built-in caps are off, even for "0,0")
    char* end = nullptr;
    k.small_caps = false;
    k.small_blocks = (uint32_t)strtoul(e, &end, 10);
    k.small_rays = (end && *end == ',') ? (uint32_t)strtoul(end + 1, nullptr, 10) : 0u;
  }
  k.quad_rays = u32("PBRHIP_QUAD_RAYS", PB_QUAD_RAYS);
  if (const char* e = env("PBRHIP_QUAD")) k.quad = e[0] == '1';
  k.simple_traversal = env("PBRHIP_SIMPLE_TRAVERSAL") != nullptr;
  return k;
}

// ------------------------------------------------------------------ scene construction
extern "C" int pbrhip_scene_create(pbrhip_scene** out) {
  return guarded([&]() -> int {
  if (!out) return fail(PBRHIP_EINVAL, "out is NULL");
  int n = 0;
  int rc = pbrhip_device_count(&n);
  if (rc) return rc;
  if (n <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
  HIPCHK(hipSetDevice(g_device));
  std::unique_ptr<pbrhip_scene> s(new pbrhip_scene());
  s->device = g_device;
  HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIPCHK(hipHostMalloc((void**)&s->h_counts, sizeof(uint32_t) * kCntNum * kMaxGroups, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&s->h_ring, sizeof(uint32_t) * 4 * kRingSlots * kMaxGroups, hipHostMallocDefault));
  memset(s->h_ring, 0, sizeof(uint32_t) * 4 * kRingSlots * kMaxGroups);
  HIPCHK(hipHostGetDevicePointer((void**)&s->d_ring, s->h_ring, 0));
  memset(&s->dscene, 0, sizeof(s->dscene));
  *out = s.release();
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_destroy(pbrhip_scene* s) {
  return guarded([&]() -> int {
  if (!s) return PBRHIP_OK;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (hipEvent_t e : s->events) (void)hipEventDestroy(e);
  for (hipStream_t g : s->group_streams) (void)hipStreamDestroy(g);
  if (s->h_counts) (void)hipHostFree(s->h_counts);
  if (s->h_ring) (void)hipHostFree(s->h_ring);
  hipStream_t st = s->stream;
  delete s;
  if (st) (void)hipStreamDestroy(st);
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_add_triangle_mesh(pbrhip_scene* s, const float* vertices_xyzw, uint32_t num_vertices,
                                              const float* normals_xyzw, uint32_t num_normals,
                                              const float* texcoords_uv, uint32_t num_texcoords,
                                              const uint32_t* vertex_ids, const uint32_t* normal_ids,
                                              const uint32_t* texcoord_ids, const uint32_t* material_ids,
                                              uint32_t num_faces, uint32_t* mesh_id) {
  return guarded([&]() -> int {
  if (!s || !mesh_id || (!vertices_xyzw && num_vertices) || (!vertex_ids && num_faces))
    return fail(PBRHIP_EINVAL, "add_triangle_mesh: NULL argument");
  if (s->committed) return fail(PBRHIP_ESTATE, "scene already committed");
  for (size_t i = 0; i < (size_t)num_faces * 3; i++)
    if (vertex_ids[i] >= num_vertices) return fail(PBRHIP_EINVAL, "vertex id %u out of range", vertex_ids[i]);
  if (normal_ids)
    for (size_t i = 0; i < (size_t)num_faces * 3; i++)
      if (normal_ids[i] != kNone && normal_ids[i] >= num_normals)
        return fail(PBRHIP_EINVAL, "normal id %u out of range", normal_ids[i]);
  if (texcoord_ids)
    for (size_t i = 0; i < (size_t)num_faces * 3; i++)
      if (texcoord_ids[i] != kNone && texcoord_ids[i] >= num_texcoords)
        return fail(PBRHIP_EINVAL, "texcoord id %u out of range", texcoord_ids[i]);
  HostMesh m;
  m.kind = 0;
  m.nfaces = num_faces;
  m.vertices.assign(vertices_xyzw, vertices_xyzw + (size_t)num_vertices * 4);
  if (num_normals) m.normals.assign(normals_xyzw, normals_xyzw + (size_t)num_normals * 4);
  if (num_texcoords) m.texcoords.assign(texcoords_uv, texcoords_uv + (size_t)num_texcoords * 2);
  m.vid.assign(vertex_ids, vertex_ids + (size_t)num_faces * 3);
  // mesh/triangle-mesh.cc:33-55: missing id arrays become all -1
  if (normal_ids) m.nid.assign(normal_ids, normal_ids + (size_t)num_faces * 3);
  else m.nid.assign((size_t)num_faces * 3, kNone);
  if (texcoord_ids) m.tid.assign(texcoord_ids, texcoord_ids + (size_t)num_faces * 3);
  else m.tid.assign((size_t)num_faces * 3, kNone);
  if (material_ids) m.mat.assign(material_ids, material_ids + num_faces);
  else m.mat.assign(num_faces, kNone);
  *mesh_id = (uint32_t)s->meshes.size();
  s->meshes.push_back(std::move(m));
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_add_curve_mesh(pbrhip_scene* s, const float* vertices_xyzr, uint32_t num_vertices,
                                           const uint32_t* indices, const uint32_t* material_ids,
                                           uint32_t num_segments, uint32_t* mesh_id) {
  return guarded([&]() -> int {
  if (!s || !mesh_id || (!vertices_xyzr && num_vertices) || (!indices && num_segments))
    return fail(PBRHIP_EINVAL, "add_curve_mesh: NULL argument");
  if (s->committed) return fail(PBRHIP_ESTATE, "scene already committed");
  for (uint32_t i = 0; i < num_segments; i++)
    if ((uint64_t)indices[i] + 4 > num_vertices) return fail(PBRHIP_EINVAL, "curve index %u out of range", indices[i]);
  HostMesh m;
  m.kind = 1;
  m.cverts.assign(vertices_xyzr, vertices_xyzr + (size_t)num_vertices * 4);
  m.cidx.assign(indices, indices + num_segments);
  if (material_ids) m.cmat.assign(material_ids, material_ids + num_segments);
  else m.cmat.assign(num_segments, kNone);
  *mesh_id = (uint32_t)s->meshes.size();
  s->meshes.push_back(std::move(m));
  return PBRHIP_OK;
  });
}

// texture ids are validated at commit (pc/pc-common.cc:116-139 adds materials first, textures after)
static int check_tex(const pbrhip_principled_param*) { return PBRHIP_OK; }
// Scene::AddTexture (scene.h:46-51) with Texture(pixels, width, height, channels) (texture.cc:10-21)
extern "C" int pbrhip_scene_add_texture(pbrhip_scene* s, const float* pixels, uint32_t width, uint32_t height,
                                        uint32_t channels, uint32_t* texture_id) {
  return guarded([&]() -> int {
  if (!s || !pixels || !texture_id) return fail(PBRHIP_EINVAL, "add_texture: NULL argument");
  if (width == 0 || height == 0 || channels == 0 || channels > 4) return fail(PBRHIP_EINVAL, "add_texture: bad shape");
  if (s->committed) return fail(PBRHIP_ESTATE, "scene already committed");
  size_t n = (size_t)width * height * channels;
  if (s->tex_pixels.size() + n >= (1ull << 32)) return fail(PBRHIP_EUNSUPPORTED, "texture pool exceeds 2^32 floats");
  TexDesc t = {(uint32_t)s->tex_pixels.size(), width, height, channels};
  s->tex_pixels.insert(s->tex_pixels.end(), pixels, pixels + n);
  *texture_id = (uint32_t)s->tex_descs.size();
  s->tex_descs.push_back(t);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_add_principled_material(pbrhip_scene* s, const pbrhip_principled_param* p, uint32_t* id) {
  return guarded([&]() -> int {
  if (!s || !p || !id) return fail(PBRHIP_EINVAL, "add_principled_material: NULL argument");
  if (int rc = check_tex(p)) return rc;
  HostMaterial m;
  m.kind = kMatPrincipled;
  memcpy(&m.pr, p, sizeof(m.pr));
  memset(&m.hr, 0, sizeof(m.hr));
  *id = (uint32_t)s->materials.size();
  s->materials.push_back(m);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_add_hair_material(pbrhip_scene* s, const pbrhip_hair_param* p, uint32_t* id) {
  return guarded([&]() -> int {
  if (!s || !p || !id) return fail(PBRHIP_EINVAL, "add_hair_material: NULL argument");
  HostMaterial m;
  m.kind = kMatHair;
  memset(&m.pr, 0, sizeof(m.pr));
  memcpy(&m.hr, p, sizeof(m.hr));
  *id = (uint32_t)s->materials.size();
  s->materials.push_back(m);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_add_area_light(pbrhip_scene* s, const float emission[3], uint32_t* id) {
  return guarded([&]() -> int {
  if (!s || !emission || !id) return fail(PBRHIP_EINVAL, "add_area_light: NULL argument");
  *id = (uint32_t)s->light_params.size();
  s->light_params.push_back(V3(emission[0], emission[1], emission[2]));
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_create_local_scene(pbrhip_scene* s, uint32_t* id) {
  return guarded([&]() -> int {
  if (!s || !id) return fail(PBRHIP_EINVAL, "create_local_scene: NULL argument");
  *id = (uint32_t)s->locals.size();
  s->locals.emplace_back();
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_add_mesh_to_local_scene(pbrhip_scene* s, uint32_t local_scene_id, uint32_t mesh_id,
                                                    uint32_t* geom_id) {
  return guarded([&]() -> int {
  if (!s || !geom_id) return fail(PBRHIP_EINVAL, "add_mesh_to_local_scene: NULL argument");
  if (local_scene_id >= s->locals.size() || mesh_id >= s->meshes.size())
    return fail(PBRHIP_EINVAL, "local scene %u / mesh %u out of range", local_scene_id, mesh_id);
  *geom_id = (uint32_t)s->locals[local_scene_id].size();
  s->locals[local_scene_id].push_back(mesh_id);
  return PBRHIP_OK;
  });
}
static const float kIdentity4x4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// raytracer_impl.cc:49-84 hands the matrix to Embree (row-vector convention, v' = v * M, translation in the last
// row); everything above the raytracer keeps working in the instance's local space (scene.cc:217,237 "TODO
// transform").  A matrix that is not invertible has no such instance.
static int check_transform(const float* m, const char* who) {
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(m[k])) return fail(PBRHIP_EINVAL, "%s: the transform has a non-finite entry", who);
  const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[1] * ((double)m[4] * m[10] - (double)m[6] * m[8]) +
                     (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
  if (!(det != 0.0)) return fail(PBRHIP_EINVAL, "%s: the transform is singular", who);
  return PBRHIP_OK;
}
extern "C" int pbrhip_scene_create_instance(pbrhip_scene* s, uint32_t local_scene_id, const float* transform,
                                            uint32_t* instance_id) {
  return guarded([&]() -> int {
  if (!s || !instance_id) return fail(PBRHIP_EINVAL, "create_instance: NULL argument");
  if (local_scene_id >= s->locals.size()) return fail(PBRHIP_EINVAL, "local scene %u out of range", local_scene_id);
  HostInstance in;
  in.local_scene = local_scene_id;
  memcpy(in.xf, transform ? transform : kIdentity4x4, sizeof(kIdentity4x4));
  in.identity = memcmp(in.xf, kIdentity4x4, sizeof(kIdentity4x4)) == 0;
  if (!in.identity)
    if (int rc = check_transform(in.xf, "create_instance")) return rc;
  // scene.cc:119-143: material ids are copied from the meshes when the instance is created
  for (uint32_t mid : s->locals[local_scene_id]) {
    const HostMesh& m = s->meshes[mid];
    in.material_ids.push_back(m.kind == 0 ? m.mat : m.cmat);
    in.light_ids.emplace_back();
  }
  *instance_id = (uint32_t)s->instances.size();
  s->instances.push_back(std::move(in));
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_attach_light_ids(pbrhip_scene* s, uint32_t instance_id, uint32_t geom_id,
                                             const uint32_t* ids, uint32_t n) {
  return guarded([&]() -> int {
  if (!s || (!ids && n)) return fail(PBRHIP_EINVAL, "attach_light_ids: NULL argument");
  if (instance_id >= s->instances.size() || geom_id >= s->instances[instance_id].light_ids.size())
    return fail(PBRHIP_EINVAL, "instance %u / geom %u out of range", instance_id, geom_id);
  if (n != 0 && n != inst_mesh(s, instance_id, geom_id)->num_prims()) return fail(PBRHIP_ESIZE, "light param error");
  for (uint32_t i = 0; i < n; i++)
    if (ids[i] != kNone && ids[i] >= s->light_params.size()) return fail(PBRHIP_EINVAL, "light id %u out of range", ids[i]);
  s->instances[instance_id].light_ids[geom_id].assign(ids, ids + n);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_attach_material_ids(pbrhip_scene* s, uint32_t instance_id, uint32_t geom_id,
                                                const uint32_t* ids, uint32_t n) {
  return guarded([&]() -> int {
  if (!s || (!ids && n)) return fail(PBRHIP_EINVAL, "attach_material_ids: NULL argument");
  if (instance_id >= s->instances.size() || geom_id >= s->instances[instance_id].material_ids.size())
    return fail(PBRHIP_EINVAL, "instance %u / geom %u out of range", instance_id, geom_id);
  if (n != inst_mesh(s, instance_id, geom_id)->num_prims()) return fail(PBRHIP_ESIZE, "material param error");
  s->instances[instance_id].material_ids[geom_id].assign(ids, ids + n);
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_wide_info(const pbrhip_scene* s, uint64_t* wide_nodes, uint32_t* stack_need, int* built_on_gpu) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  if (wide_nodes) *wide_nodes = s->dscene.wide_nodes;
  if (stack_need) *stack_need = s->wide_stack_need;
  if (built_on_gpu) *built_on_gpu = s->wide_built_on_gpu ? 1 : 0;
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_set_bvh_builder(pbrhip_scene* s, int builder) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  if (builder != PBRHIP_BVH_HOST_SAH && builder != PBRHIP_BVH_GPU_LBVH && builder != PBRHIP_BVH_GPU_LBVH_WIDE) return fail(PBRHIP_EINVAL, "unknown BVH builder %d", builder);
  if (s->committed) return fail(PBRHIP_ESTATE, "scene already committed");
  s->bvh_builder = builder;
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_aabb(const pbrhip_scene* s, float bmin[3], float bmax[3]) {
  return guarded([&]() -> int {
  if (!s || !bmin || !bmax) return fail(PBRHIP_EINVAL, "scene_aabb: NULL argument");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  memcpy(bmin, s->bmin, 12), memcpy(bmax, s->bmax, 12);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_info(const pbrhip_scene* s, uint64_t* num_nodes, uint64_t* num_slots, uint32_t* depth,
                                 uint64_t* device_bytes) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  if (num_nodes) *num_nodes = s->dscene.num_nodes;
  if (num_slots) *num_slots = s->dscene.num_slots;
  if (depth) *depth = s->bvh_depth;
  if (device_bytes) *device_bytes = s->device_bytes();
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_shadow_grid_info(pbrhip_scene* s, pbrhip_shadow_grid_info* out) {
  return guarded([&]() -> int {
  if (!s || !out) return fail(PBRHIP_EINVAL, "scene_shadow_grid_info: NULL argument");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  if (int rc = ensure_shadow_grid(s, read_knobs())) return rc;
  const ShaftState& g = s->shaft;
  memset(out, 0, sizeof(*out));
  out->resolution = g.n, out->num_lights = g.n ? g.num_lights : 0u, out->max_list = g.n ? g.max_list : 0u;
  out->bytes = g.cells.n * sizeof(uint32_t), out->build_ms = g.build_ms;
  out->culled_shadow_rays = g.culled, out->clear_cell_rays = g.clear_rays, out->leaf_tests = g.pair_tests;
  if (g.n) {
    std::vector<uint32_t> h((size_t)g.n * g.n * g.n * g.num_lights * kShaftCellWords);
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpy(h.data(), g.cells.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < h.size(); c += kShaftCellWords) {
      if (h[c] == kShaftUnknown) out->unknown_cells++;
      else out->clear_cells++, out->empty_cells += h[c] == 0u, out->listed_leaves += h[c];
    }
  }
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_read_shadow_grid(pbrhip_scene* s, uint32_t* cells, size_t num_words) {
  return guarded([&]() -> int {
  if (!s || !cells) return fail(PBRHIP_EINVAL, "scene_read_shadow_grid: NULL argument");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  if (int rc = ensure_shadow_grid(s, read_knobs())) return rc;
  const ShaftState& g = s->shaft;
  const size_t words = (size_t)g.n * g.n * g.n * (g.n ? g.num_lights : 0u) * kShaftCellWords;
  if (num_words != words) return fail(PBRHIP_EINVAL, "scene_read_shadow_grid: the grid has %zu words, the buffer %zu", words, num_words);
  HIPCHK(hipSetDevice(s->device));
  if (words) HIPCHK(hipMemcpy(cells, g.cells.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_update_principled_material(pbrhip_scene* s, uint32_t id, const pbrhip_principled_param* p) {
  return guarded([&]() -> int {
  if (!s || !p) return fail(PBRHIP_EINVAL, "update_material: NULL argument");
  if (int rc = check_tex(p)) return rc;
  HostMaterial m;
  m.kind = kMatPrincipled;
  memcpy(&m.pr, p, sizeof(m.pr));
  memset(&m.hr, 0, sizeof(m.hr));
  return update_material(s, id, m);
  });
}
extern "C" int pbrhip_scene_update_hair_material(pbrhip_scene* s, uint32_t id, const pbrhip_hair_param* p) {
  return guarded([&]() -> int {
  if (!s || !p) return fail(PBRHIP_EINVAL, "update_material: NULL argument");
  HostMaterial m;
  m.kind = kMatHair;
  memset(&m.pr, 0, sizeof(m.pr));
  memcpy(&m.hr, p, sizeof(m.hr));
  return update_material(s, id, m);
  });
}

// ------------------------------------------------------------------ geometry edits and the refit ("The refit, exactly")
static bool all_finite(const float* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}
// after an edit of the host model: on a committed scene every instance that shows the mesh (mesh_id) or the one instance is dirty
static void mark_dirty(pbrhip_scene* s, uint32_t mesh_id, uint32_t instance_id) {
  if (!s->committed) return;
  s->dirty_inst.resize(s->instances.size(), 0);
  for (uint32_t i = 0; i < s->instances.size(); i++) {
    bool hit = i == instance_id;
    if (mesh_id != kNone)
      for (uint32_t m : s->locals[s->instances[i].local_scene]) hit = hit || m == mesh_id;
    if (hit) s->dirty_inst[i] = 1, s->stale = true;
  }
}
static int check_mesh_update(const pbrhip_scene* s, uint32_t mesh_id, int kind, const char* who) {
  if (s->replica) return fail(PBRHIP_ESTATE, "%s: a replica holds no geometry (refit the source scene and replicate it again)", who);
  if (mesh_id >= s->meshes.size()) return fail(PBRHIP_EINVAL, "%s: mesh %u out of range", who, mesh_id);
  if (s->meshes[mesh_id].kind != kind) return fail(PBRHIP_EINVAL, "%s: mesh %u is of the other kind", who, mesh_id);
  return PBRHIP_OK;
}
extern "C" int pbrhip_scene_update_triangle_mesh(pbrhip_scene* s, uint32_t mesh_id, const float* vertices_xyzw, uint32_t num_vertices,
                                                 const float* normals_xyzw, uint32_t num_normals) {
  return guarded([&]() -> int {
  if (!s || (!vertices_xyzw && num_vertices)) return fail(PBRHIP_EINVAL, "update_triangle_mesh: NULL argument");
  if (int rc = check_mesh_update(s, mesh_id, 0, "update_triangle_mesh")) return rc;
  HostMesh& m = s->meshes[mesh_id];
  if ((size_t)num_vertices * 4 != m.vertices.size()) return fail(PBRHIP_ESIZE, "update_triangle_mesh: %u vertices, the mesh has %zu", num_vertices, m.vertices.size() / 4);
  if (normals_xyzw && (size_t)num_normals * 4 != m.normals.size()) return fail(PBRHIP_ESIZE, "update_triangle_mesh: %u normals, the mesh has %zu", num_normals, m.normals.size() / 4);
  if (!all_finite(vertices_xyzw, (size_t)num_vertices * 4) || (normals_xyzw && !all_finite(normals_xyzw, (size_t)num_normals * 4)))
    return fail(PBRHIP_EINVAL, "update_triangle_mesh: a value is not finite");
  m.vertices.assign(vertices_xyzw, vertices_xyzw + (size_t)num_vertices * 4);
  if (normals_xyzw) m.normals.assign(normals_xyzw, normals_xyzw + (size_t)num_normals * 4);
  mark_dirty(s, mesh_id, kNone);
  return refresh_mesh_device(s, mesh_id);  // (device geometry mode: the device copy follows the model)
  });
}
extern "C" int pbrhip_scene_update_curve_mesh(pbrhip_scene* s, uint32_t mesh_id, const float* vertices_xyzr, uint32_t num_vertices) {
  return guarded([&]() -> int {
  if (!s || (!vertices_xyzr && num_vertices)) return fail(PBRHIP_EINVAL, "update_curve_mesh: NULL argument");
  if (int rc = check_mesh_update(s, mesh_id, 1, "update_curve_mesh")) return rc;
  HostMesh& m = s->meshes[mesh_id];
  if ((size_t)num_vertices * 4 != m.cverts.size()) return fail(PBRHIP_ESIZE, "update_curve_mesh: %u vertices, the mesh has %zu", num_vertices, m.cverts.size() / 4);
  if (!all_finite(vertices_xyzr, (size_t)num_vertices * 4)) return fail(PBRHIP_EINVAL, "update_curve_mesh: a value is not finite");
  m.cverts.assign(vertices_xyzr, vertices_xyzr + (size_t)num_vertices * 4);
  mark_dirty(s, mesh_id, kNone);
  return refresh_mesh_device(s, mesh_id);
  });
}
// `bytes` at p: device memory of the scene's device (hipPointerGetAttributes; a host pointer has no attributes or is "unregistered") and,
// where the runtime knows the allocation's range, all of it inside that allocation
static int check_device_array(const pbrhip_scene* s, const void* p, size_t bytes, const char* who) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PBRHIP_EINVAL, "%s: the array is not device memory", who);
  }
  if (at.type != hipMemoryTypeDevice) return fail(PBRHIP_EINVAL, "%s: the array is not device memory", who);
  if (at.device != s->device) return fail(PBRHIP_EINVAL, "%s: the array is on device %d, the scene on device %d", who, at.device, s->device);
  void* base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, const_cast<void*>(p)) == hipSuccess) {
    const size_t at_byte = (size_t)((const char*)p - (const char*)base);
    if (at_byte > size || bytes > size - at_byte) return fail(PBRHIP_ESIZE, "%s: the array ends %zu bytes past its device allocation", who, at_byte + bytes - size);
  } else {
    (void)hipGetLastError();  // (memory mapped through the virtual-memory calls has no such range: its attributes are what is known of it)
  }
  if ((uintptr_t)p % 16) return fail(PBRHIP_EINVAL, "%s: the array is not 16-byte aligned", who);
  return PBRHIP_OK;
}
extern "C" int pbrhip_scene_update_triangle_mesh_device(pbrhip_scene* s, uint32_t mesh_id, const void* d_vertices_xyzw, uint32_t num_vertices,
                                                        const void* d_normals_xyzw, uint32_t num_normals, void* stream) {
  return guarded([&]() -> int {
  const char* who = "update_triangle_mesh_device";
  if (!s || (!d_vertices_xyzw && num_vertices)) return fail(PBRHIP_EINVAL, "%s: NULL argument", who);
  if (int rc = check_mesh_update(s, mesh_id, 0, who)) return rc;
  const HostMesh& m = s->meshes[mesh_id];
  if ((size_t)num_vertices * 4 != m.vertices.size()) return fail(PBRHIP_ESIZE, "%s: %u vertices, the mesh has %zu", who, num_vertices, m.vertices.size() / 4);
  if (d_normals_xyzw && (size_t)num_normals * 4 != m.normals.size()) return fail(PBRHIP_ESIZE, "%s: %u normals, the mesh has %zu", who, num_normals, m.normals.size() / 4);
  HIPCHK(hipSetDevice(s->device));
  if (num_vertices)
    if (int rc = check_device_array(s, d_vertices_xyzw, (size_t)num_vertices * 16, who)) return rc;
  if (d_normals_xyzw && num_normals)
    if (int rc = check_device_array(s, d_normals_xyzw, (size_t)num_normals * 16, who)) return rc;
  if (int rc = update_mesh_device(s, mesh_id, d_vertices_xyzw, num_normals ? d_normals_xyzw : nullptr, stream, who)) return rc;
  mark_dirty(s, mesh_id, kNone);
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_update_curve_mesh_device(pbrhip_scene* s, uint32_t mesh_id, const void* d_vertices_xyzr, uint32_t num_vertices, void* stream) {
  return guarded([&]() -> int {
  const char* who = "update_curve_mesh_device";
  if (!s || (!d_vertices_xyzr && num_vertices)) return fail(PBRHIP_EINVAL, "%s: NULL argument", who);
  if (int rc = check_mesh_update(s, mesh_id, 1, who)) return rc;
  const HostMesh& m = s->meshes[mesh_id];
  if ((size_t)num_vertices * 4 != m.cverts.size()) return fail(PBRHIP_ESIZE, "%s: %u vertices, the mesh has %zu", who, num_vertices, m.cverts.size() / 4);
  HIPCHK(hipSetDevice(s->device));
  if (num_vertices)
    if (int rc = check_device_array(s, d_vertices_xyzr, (size_t)num_vertices * 16, who)) return rc;
  if (int rc = update_mesh_device(s, mesh_id, d_vertices_xyzr, nullptr, stream, who)) return rc;
  mark_dirty(s, mesh_id, kNone);
  return PBRHIP_OK;
  });
}
// test hook: the committed scene's slots (64 B each, leaf order) and ShadeRecs (128 B each) as the device holds them
extern "C" int pbrhip_scene_read_slots(pbrhip_scene* s, void* slots_out, void* shade_out, uint32_t* num_slots) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene_read_slots: scene is NULL");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  const uint32_t ns = s->tree.num_slots;
  if (num_slots) *num_slots = ns;
  if ((slots_out || shade_out) && ns) {
    HIPCHK(hipSetDevice(s->device));
    if (slots_out) HIPCHK(hipMemcpyAsync(slots_out, s->dscene.slots, (size_t)ns * 64, hipMemcpyDeviceToHost, s->stream));
    if (shade_out) HIPCHK(hipMemcpyAsync(shade_out, s->dscene.shade, (size_t)ns * sizeof(ShadeRec), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
  }
  return PBRHIP_OK;
  });
}
extern "C" int pbrhip_scene_update_instance_transform(pbrhip_scene* s, uint32_t instance_id, const float* transform) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "update_instance_transform: scene is NULL");
  if (s->replica) return fail(PBRHIP_ESTATE, "update_instance_transform: a replica holds no geometry (refit the source scene and replicate it again)");
  if (instance_id >= s->instances.size()) return fail(PBRHIP_EINVAL, "update_instance_transform: instance %u out of range", instance_id);
  const float* m = transform ? transform : kIdentity4x4;
  const bool identity = memcmp(m, kIdentity4x4, sizeof(kIdentity4x4)) == 0;
  if (!identity)
    if (int rc = check_transform(m, "update_instance_transform")) return rc;
  HostInstance& in = s->instances[instance_id];
  memcpy(in.xf, m, sizeof(in.xf));
  in.identity = identity;
  mark_dirty(s, kNone, instance_id);
  return PBRHIP_OK;
  });
}

// ------------------------------------------------------------------ environment light
namespace pb {
int set_environment(pbrhip_scene* s, const float* rgb, uint32_t width, uint32_t height, float scale, const float* world_to_env) {
  float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  EnvTables t;
  if (rgb) {
    if (width == 0 || height == 0) return fail(PBRHIP_EINVAL, "set_environment: zero size (%u x %u)", width, height);
    if (world_to_env) {
      for (int i = 0; i < 9; i++) {
        if (!isfinite(world_to_env[i])) return fail(PBRHIP_EINVAL, "set_environment: world_to_env is not finite");
        m[i] = world_to_env[i];
      }
      for (int i = 0; i < 3; i++)  // a rotation: M M^T = I
        for (int j = 0; j < 3; j++) {
          const double d = (double)m[3 * i] * m[3 * j] + (double)m[3 * i + 1] * m[3 * j + 1] + (double)m[3 * i + 2] * m[3 * j + 2];
          if (fabs(d - (i == j ? 1.0 : 0.0)) > 1e-4) return fail(PBRHIP_EINVAL, "set_environment: world_to_env is not a rotation");
        }
    }
    if (build_env_tables(rgb, width, height, scale, &t))
      return fail(PBRHIP_EINVAL, "set_environment: a texel or the scale is negative, NaN or infinite, or the map is too large (%u x %u)", width, height);
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (a render in flight still reads the old tables)
  DScene& d = s->dscene;
  // no environment until the new tables are on the device (a failed upload leaves none, not freed memory)
  d.env_texels = nullptr, d.env_alias = nullptr, d.env_w = d.env_h = 0;
  s->env_rgb.clear(), s->env_w = s->env_h = 0;
  if (!t.present) {  // no map, or an all-black one: no environment -- the scene runs the kernels it ran without one
    s->d_env_texels.release(), s->d_env_alias.release();
    return PBRHIP_OK;
  }
  const size_t n = (size_t)width * height;
  std::vector<float4> texels(n);
  std::vector<uint2> alias(n);
  for (size_t i = 0; i < n; i++) {
    texels[i] = make_float4(t.texels[4 * i], t.texels[4 * i + 1], t.texels[4 * i + 2], t.texels[4 * i + 3]);
    alias[i] = make_uint2(t.keep[i], t.alias[i]);
  }
  HIPCHK(s->d_env_texels.upload(texels, s->stream));
  HIPCHK(s->d_env_alias.upload(alias, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->env_rgb.assign(rgb, rgb + 3 * n), s->env_w = width, s->env_h = height, s->env_scale = scale;
  memcpy(s->env_m, m, sizeof(m));
  d.env_texels = s->d_env_texels.p, d.env_alias = s->d_env_alias.p, d.env_w = width, d.env_h = height;
  memcpy(d.env_m, m, sizeof(m));
  return PBRHIP_OK;
}
}  // namespace pb
extern "C" int pbrhip_scene_set_environment(pbrhip_scene* s, const float* rgb, uint32_t width, uint32_t height, float scale,
                                            const float world_to_env[9]) {
  return guarded([&]() -> int {
    if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
    return set_environment(s, rgb, width, height, scale, world_to_env);
  });
}

// ------------------------------------------------------------------ look-at camera
namespace pb {
int set_camera(pbrhip_scene* s, const float* eye, const float* lookat, const float* up, float vfov, float lens_radius, float focus_distance) {
  if (!eye) {
    s->cam_set = false;
    return PBRHIP_OK;
  }
  if (!lookat || !up) return fail(PBRHIP_EINVAL, "set_camera: lookat or up is NULL");
  for (int k = 0; k < 3; k++)
    if (!isfinite(eye[k]) || !isfinite(lookat[k]) || !isfinite(up[k])) return fail(PBRHIP_EINVAL, "set_camera: eye, lookat or up is not finite");
  if (!isfinite(vfov) || !isfinite(lens_radius) || !isfinite(focus_distance)) return fail(PBRHIP_EINVAL, "set_camera: a parameter is not finite");
  if (!(vfov > 0.0f && vfov < 180.0f)) return fail(PBRHIP_EINVAL, "set_camera: vfov %g is not in (0, 180)", (double)vfov);
  if (lens_radius < 0.0f) return fail(PBRHIP_EINVAL, "set_camera: lens_radius %g < 0", (double)lens_radius);
  if (focus_distance < 0.0f) return fail(PBRHIP_EINVAL, "set_camera: focus_distance %g < 0", (double)focus_distance);
  const double fx = (double)lookat[0] - eye[0], fy = (double)lookat[1] - eye[1], fz = (double)lookat[2] - eye[2];
  const double fl = sqrt(fx * fx + fy * fy + fz * fz), ul = sqrt((double)up[0] * up[0] + (double)up[1] * up[1] + (double)up[2] * up[2]);
  if (!(fl > 0.0)) return fail(PBRHIP_EINVAL, "set_camera: eye == lookat");
  // sin of the angle between up and the view direction
  const double cx = fy * up[2] - fz * up[1], cy = fz * up[0] - fx * up[2], cz = fx * up[1] - fy * up[0];
  if (!(ul > 0.0) || sqrt(cx * cx + cy * cy + cz * cz) <= 1e-6 * fl * ul) return fail(PBRHIP_EINVAL, "set_camera: up is parallel to the view direction");
  memcpy(s->cam_eye, eye, sizeof(s->cam_eye)), memcpy(s->cam_lookat, lookat, sizeof(s->cam_lookat)), memcpy(s->cam_up, up, sizeof(s->cam_up));
  s->cam_vfov = vfov, s->cam_lens = lens_radius, s->cam_focus = focus_distance, s->cam_set = true;
  return PBRHIP_OK;
}
}  // namespace pb
extern "C" int pbrhip_scene_set_camera(pbrhip_scene* s, const float eye[3], const float lookat[3], const float up[3], float vfov_degrees,
                                       float lens_radius, float focus_distance) {
  return guarded([&]() -> int {
    if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
    return set_camera(s, eye, lookat, up, vfov_degrees, lens_radius, focus_distance);
  });
}
// the frame of the scene's user camera for a width x height image, in double, rounded once (dscene.h::UserCamera)
PoseCamera pb::pose_camera(const pbrhip_scene* s) {
  PoseCamera c;
  c.set = s->cam_set;
  memcpy(c.eye, s->cam_eye, sizeof(c.eye)), memcpy(c.lookat, s->cam_lookat, sizeof(c.lookat)), memcpy(c.up, s->cam_up, sizeof(c.up));
  c.vfov = s->cam_vfov, c.lens = s->cam_lens, c.focus = s->cam_focus;
  memcpy(c.bmin, s->bmin, sizeof(c.bmin)), memcpy(c.bmax, s->bmax, sizeof(c.bmax));
  return c;
}
UserCamera pb::make_user_camera(const pbrhip_scene* s, uint32_t width, uint32_t height) { return make_user_camera(pose_camera(s), width, height); }
UserCamera pb::make_user_camera(const PoseCamera& pc, uint32_t width, uint32_t height) {
  double f[3], r[3], u[3], up[3];
  for (int k = 0; k < 3; k++) f[k] = (double)pc.lookat[k] - pc.eye[k], up[k] = pc.up[k];
  const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  for (int k = 0; k < 3; k++) f[k] /= fl;
  r[0] = f[1] * up[2] - f[2] * up[1], r[1] = f[2] * up[0] - f[0] * up[2], r[2] = f[0] * up[1] - f[1] * up[0];
  const double rl = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int k = 0; k < 3; k++) r[k] /= rl;
  u[0] = r[1] * f[2] - r[2] * f[1], u[1] = r[2] * f[0] - r[0] * f[2], u[2] = r[0] * f[1] - r[1] * f[0];
  UserCamera c;
  for (int k = 0; k < 3; k++) c.eye[k] = pc.eye[k], c.f[k] = (float)f[k], c.r[k] = (float)r[k], c.u[k] = (float)u[k];
  const double h = tan((double)pc.vfov * M_PI / 360.0);
  c.h = (float)h, c.ha = (float)(h * width / height);
  c.lens = pc.lens, c.focus = pc.focus > 0.0f ? pc.focus : (float)fl;
  return c;
}

// ------------------------------------------------------------------ tiles (render-tile.cc:29-41)
extern "C" int pbrhip_create_tiles(uint32_t width, uint32_t height, uint32_t* out, uint32_t* num_tiles) {
  return guarded([&]() -> int {
  if (!num_tiles) return fail(PBRHIP_EINVAL, "num_tiles is NULL");
  const uint32_t kTile = 64;
  uint32_t n = 0;
  for (uint32_t i = 0; i < height; i += kTile)
    for (uint32_t j = 0; j < width; j += kTile) {
      if (out) {
        out[4 * n + 0] = j, out[4 * n + 1] = std::min(j + kTile, width);
        out[4 * n + 2] = i, out[4 * n + 3] = std::min(i + kTile, height);
      }
      n++;
    }
  *num_tiles = n;
  return PBRHIP_OK;
  });
}

// camera of RenderingTile (render.cc:132-158)
Camera pb::make_camera(const pbrhip_scene* s, uint32_t width, uint32_t height) { return make_camera(pose_camera(s), width, height); }
Camera pb::make_camera(const PoseCamera& pc, uint32_t width, uint32_t height) {
  const float *bmin = pc.bmin, *bmax = pc.bmax;
  float hs, vs;
  if (bmax[0] - bmin[0] > bmax[1] - bmin[1]) {
    hs = bmax[0] - bmin[0];
    vs = hs * float(height) / float(width);
  } else {
    vs = bmax[1] - bmin[1];
    hs = vs * float(width) / float(height);
  }
  Camera c;
  c.org[0] = (bmax[0] + bmin[0]) * 0.5f;
  c.org[1] = (bmax[1] + bmin[1]) * 0.5f;
  c.org[2] = bmax[2] + hs * 0.5f * sqrtf(3.f);
  c.x_corner = (bmax[0] + bmin[0]) * 0.5f - hs * 0.5f;
  c.y_corner = (bmax[1] + bmin[1]) * 0.5f + vs * 0.5f;
  c.z_corner = bmax[2];
  c.dx = hs / float(width);
  c.dy = vs / float(height);
  return c;
}

// ------------------------------------------------------------------ render
static constexpr uint64_t kBytesPerPath = 64 + 32 + 2 * 16 + 5 * 16 + 16 + 7 * 4;  // ensure_paths(): rec, srec, L + hit, sss, sh_e, queues
namespace {
struct Timer {
  pbrhip_scene* s;
  bool on;
  hipStream_t stream;
  std::vector<hipEvent_t> events;  // owned by the scene's pool once collected
  size_t used = 0;
  struct Rec {
    size_t ev;
    double* acc;
  };
  std::vector<Rec> recs;
  // first / last event of every enqueued iteration of the group: the gaps between them are the time the stream sat empty
  std::vector<std::pair<size_t, size_t>> iters;
  double* idle_acc = nullptr;
  const double* only = nullptr;  // PBRHIP_RENDER_TIMING_TRACE: only the launches that report into this accumulator are timed
  bool skipped = false;
  void iteration_begins() {
    if (on && !only) iters.push_back({used, used});
  }
  void iteration_ends() {
    if (on && !only && !iters.empty() && used >= 1) iters.back().second = used - 1;
  }
  hipError_t begin(double* acc) {
    if (!on) return hipSuccess;
    skipped = only && acc != only;
    if (skipped) return hipSuccess;
    while (events.size() < used + 2) {
      hipEvent_t e;
      if (!s->events.empty()) {
        e = s->events.back();
        s->events.pop_back();
      } else {
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
      }
      events.push_back(e);
    }
    recs.push_back({used, acc});
    return hipEventRecord(events[used], stream);
  }
  hipError_t end() {
    if (!on || skipped) return hipSuccess;
    hipError_t rc = hipEventRecord(events[used + 1], stream);
    used += 2;
    return rc;
  }
  // call after a stream sync
  hipError_t collect() {
    if (!on) return hipSuccess;
    for (const Rec& r : recs) {
      float ms = 0.f;
      hipError_t rc = hipEventElapsedTime(&ms, events[r.ev], events[r.ev + 1]);
      if (rc != hipSuccess) return rc;
      *r.acc += (double)ms;
    }
    recs.clear();
    for (size_t i = 1; i < iters.size() && idle_acc; i++) {
      float ms = 0.f;
      if (iters[i - 1].second >= iters[i].first || iters[i].first >= used) continue;
      hipError_t rc = hipEventElapsedTime(&ms, events[iters[i - 1].second], events[iters[i].first]);
      if (rc != hipSuccess) return rc;
      *idle_acc += (double)ms;
    }
    iters.clear();
    used = 0;
    for (hipEvent_t e : events) s->events.push_back(e);  // back to the scene's pool
    events.clear();
    return hipSuccess;
  }
};
}  // namespace

void pb::shard_pixels(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t block, std::vector<uint32_t>* out) {
  if (block == 0) block = 64;  // CreateTiles' tile (pbrhip_create_tiles enumerates the same blocks in the same order)
  out->clear();
  uint32_t t = 0;
  for (uint32_t by = 0; by < h; by += block)
    for (uint32_t bx = 0; bx < w; bx += block, t++) {
      if (t % world != rank) continue;  // interleaved block -> GPU map
      for (uint32_t y = by; y < std::min(by + block, h); y++)
        for (uint32_t x = bx; x < std::min(bx + block, w); x++) out->push_back(y * w + x);
    }
}

int pb::ensure_pixels(pbrhip_scene* s, const Knobs& k, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t block) {
  if (block == 0) block = 64;
  uint32_t pt = k.pixel_tile;
  const bool shuffle = k.patch_shuffle;
  pt |= shuffle ? 0x80000000u : 0u;  // (part of the cache key below)
  if (s->pk_w == w && s->pk_h == h && s->pk_rank == rank && s->pk_world == world && s->pk_block == block && s->pk_tile == pt && s->pix_index.p) return PBRHIP_OK;
  std::vector<uint32_t> pix;
  shard_pixels(w, h, rank, world, block, &pix);
  // The order the paths of a pass are laid out in (path j of a pass = pixel pix[j]): the rank's blocks in shard_pixels' order, and
  // inside a block sub-blocks of PBRHIP_PIXEL_TILE x PBRHIP_PIXEL_TILE pixels (default 8) instead of rows -- a wave's 64 camera
  // rays are an 8 x 8 patch, not a 64 x 1 strip: they share more of the tree, and so do their later bounces.  A permutation of
  // the list: every value is a function of (pixel, pass) alone, images do not change.
  HIPCHK(s->pix_index.upload(pix, s->stream));  // (the shard's own order: what the exchange packs and unpacks by, multi.cpp)
  const uint32_t pt_key = pt;
  pt &= 0x7FFFFFFFu;
  if (pt > 1u && pt < block) {
    std::vector<uint32_t> ordered;
    ordered.reserve(pix.size());
    std::vector<std::pair<uint32_t, uint32_t>> patches;  // (first entry, entries) of every patch in `ordered`
    uint32_t t = 0;
    for (uint32_t by = 0; by < h; by += block)
      for (uint32_t bx = 0; bx < w; bx += block, t++) {
        if (t % world != rank) continue;
        const uint32_t ey = std::min(by + block, h), ex = std::min(bx + block, w);
        for (uint32_t sy = by; sy < ey; sy += pt)
          for (uint32_t sx = bx; sx < ex; sx += pt) {
            const uint32_t at = (uint32_t)ordered.size();
            for (uint32_t y = sy; y < std::min(sy + pt, ey); y++)
              for (uint32_t x = sx; x < std::min(sx + pt, ex); x++) ordered.push_back(y * w + x);
            patches.push_back({at, (uint32_t)ordered.size() - at});
          }
      }
    // Round 6: the patches in a SCATTERED order (patch i of the list = patch i x K mod M of the image order, K ~ 0.38 M, coprime to
    // M).  k_trace's waves take rays from the queue in batches of up to 512 = eight patches, a wave takes only five or six batches
    // per launch, and in image order a batch is ONE image region: the batches over dense geometry cost several times the batches over
    // the walls, the waves that drew them found the queue empty up to 0.46 ms after the first wave had (per-wave timeline:
    // profiles/README.md), and every launch ended with the chip half empty for that long.  Scattered, a batch is eight regions and
    // consecutive batches are unrelated: the batches cost about the same.  A permutation: the image does not depend on it.
    if (shuffle && patches.size() > 2) {
      const uint64_t M = patches.size();
      uint64_t K = (uint64_t)((double)M * 0.381966) | 1ull;
      auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t r = a % b; a = b, b = r; } return a; };
      while (gcd(K, M) != 1) K += 2;
      std::vector<uint32_t> scattered;
      scattered.reserve(ordered.size());
      for (uint64_t i = 0; i < M; i++) {
        const auto& pch = patches[(size_t)((i * K) % M)];
        scattered.insert(scattered.end(), ordered.begin() + pch.first, ordered.begin() + pch.first + pch.second);
      }
      ordered.swap(scattered);
    }
    pix.swap(ordered);
  }
  HIPCHK(s->path_pix.upload(pix, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->pk_w = w, s->pk_h = h, s->pk_rank = rank, s->pk_world = world, s->pk_block = block, s->pk_tile = pt_key, s->pk_npix = (uint32_t)pix.size();
  return PBRHIP_OK;
}

static int ensure_groups(pbrhip_scene* s, uint32_t groups) {
  while (s->group_streams.size() + 1 < groups) {
    hipStream_t g;
    HIPCHK(hipStreamCreateWithFlags(&g, hipStreamNonBlocking));
    s->group_streams.push_back(g);
  }
  HIPCHK(s->counts.reserve(kCntNum * kMaxGroups));
  HIPCHK(s->spill.reserve((size_t)groups * kSpillWords));
  return PBRHIP_OK;
}

static int ensure_paths(pbrhip_scene* s, size_t n) {
  HIPCHK(s->rec.reserve(4 * n));   // ray_o | ray_d | thr | rng (kernels.h::PathState)
  HIPCHK(s->srec.reserve(2 * n));  // sh_d | sh_c
  HIPCHK(s->L.reserve(n));
  HIPCHK(s->hit.reserve(n));
  HIPCHK(s->ssrec.reserve(4 * n));  // sss_sigt | sss_sigs | sss_thr | sss_ez
  HIPCHK(s->sss_A.reserve(n));
  HIPCHK(s->sh_e.reserve(n));
  for (auto& b : s->q) HIPCHK(b.reserve(n));
  HIPCHK(s->counts.reserve(kCntNum * kMaxGroups));
  HIPCHK(s->stats.reserve(kStatNum));
  return PBRHIP_OK;
}

// PathState::pass_run of a group of `npass` passes: 1 for scenes of surfaces; scenes with curves: the largest power of two <= 64 that
// divides npass.  PBRHIP_PASS_RUN=R forces a run length (when it divides npass; 1 = off): A/B and tests.
static uint32_t pass_run_for(const Knobs& k, uint32_t npass, bool curves) {
  const uint32_t want = k.pass_run ? k.pass_run : (curves ? 64u : 1u);
  uint32_t r = 1u;
  while (r * 2u <= want && npass % (r * 2u) == 0u) r *= 2u;
  return r;
}

// How the passes of a chunk are split into path groups (each group = its own queues, counters and HIP stream; path
// slots stay global and passes are accumulated in ascending order, so the image does not depend on the split: GPU test).
// The scheduler (ChunkRun) starts groups in order while fewer than `window` of them are in their bulk phase (default:
// all at once).  PBRHIP_GROUPS="56,8" (passes per group, started one after the other: PBRHIP_WINDOW defaults to 1 then)
// and pbrhip_render_desc.num_streams = n (n equal groups at once) override the default plan; the pipelined plans that
// were tried (geometric sizes, big-then-small pairs) all lost to it, see profiles/README.md.
static std::vector<uint32_t> plan_groups(const Knobs& k, uint32_t np, uint32_t npix, uint32_t want_groups) {
  std::vector<uint32_t> g;
  if (const char* e = k.groups) {  // explicit passes per group, e.g. "32,16,8,4,2,1,1" (the rest joins the last)
    uint32_t left = np;
    for (const char* p = e; *p && left;) {
      uint32_t v = (uint32_t)strtoul(p, (char**)&p, 10);
      if (*p == ',') p++;
      v = std::max(1u, std::min(v, left));
      g.push_back(v), left -= v;
    }
    if (left) {
      if (g.empty()) g.push_back(left);
      else g.back() += left;
    }
    return g;
  }
  if (want_groups) {  // pbrhip_render_desc.num_streams: that many equal groups
    const uint32_t ng = std::min(std::min(want_groups, (uint32_t)kMaxGroups * 2u), np);
    for (uint32_t k = 0; k < ng; k++) g.push_back((uint32_t)((uint64_t)np * (k + 1) / ng) - (uint32_t)((uint64_t)np * k / ng));
    return g;
  }
  // default (A/B on C2, scripts/sched_ab.py, profiles/README.md): two equal groups, both started at once, when the chunk
  // holds at least 96 Mi paths (the whole 132.7 M-path frame: 60.4 -> 58.9 ms; one group's launch-bound drains and its
  // k_tail overlap the other's bulk work); one group below that (a half / quarter / eighth of the frame: 32.6 / 19.7 /
  // 12.1 ms with one group against 32.2 / 19.9 / 12.8 with two -- every extra group adds its own latency-bound launches)
  // Round 4, after the shading kernels got faster: two groups also pay for a half and a quarter of the frame (27.1-27.2 / 16.0-16.4 ms
  // against 27.9-28.2 / 16.6-16.7 with one), not for an eighth (10.0-10.2 either way): the threshold was 24 Mi paths.
  // Round 5 (kernels 5-8 % faster, the launches' drains the same): an eighth of the frame (15.8 Mi paths) 9.50-9.57 ms with one group,
  // 9.13-9.15 with two, 9.19-9.33 with three: the threshold is 12 Mi paths.
  if ((uint64_t)np * npix >= (12ull << 20) && np >= 2) g.push_back(np / 2), g.push_back(np - np / 2);
  else g.push_back(np);
  return g;
}

int pb::check_render_desc(const pbrhip_scene* s, const pbrhip_render_desc* d) {
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  if (d->width == 0 || d->height == 0) return fail(PBRHIP_EINVAL, "empty image");
  if ((uint64_t)d->width * d->height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "image too large");
  const uint32_t world = d->tile_world ? d->tile_world : 1;
  if (d->tile_rank >= world) return fail(PBRHIP_EINVAL, "tile_rank %u >= tile_world %u", d->tile_rank, world);
  if (d->shard_block > 4096) return fail(PBRHIP_EINVAL, "shard_block %u is not a sensible block edge", d->shard_block);
  return PBRHIP_OK;
}

// Passes per chunk.  Default: as many paths in flight as 60 % of the free HBM holds (288 GB: a whole 1080p x 64 spp frame,
// 132.7 M paths x 244 B, is one chunk) -- fewer, larger launches and one tail instead of many
static int chunk_passes_for(const pbrhip_scene* s, const pbrhip_render_desc* d, const Knobs& k, uint32_t npix, uint32_t* out) {
  uint64_t max_paths = d->max_paths_in_flight;
  if (!max_paths) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // what this scene already holds for path state counts as available
    size_t have = (s->rec.n + s->srec.n + s->ssrec.n + s->L.n + s->hit.n + s->sh_e.n + s->sss_A.n) * 16;
    for (auto& b : s->q) have += b.n * 4;
    max_paths = std::min<uint64_t>(kMaxPathsInFlight,
                                   std::max<uint64_t>(1ull << 20, (uint64_t)((free_b + have) * 0.6) / kBytesPerPath));
  }
  if (max_paths > kMaxPathsInFlight) max_paths = kMaxPathsInFlight;
  if (k.debug) {
    size_t fb = 0, tb = 0;
    (void)hipMemGetInfo(&fb, &tb);
    fprintf(stderr, "pbrhip: free %.1f GB total %.1f GB max_paths %llu npix %u\n", fb / 1e9, tb / 1e9, (unsigned long long)max_paths, npix);
  }
  if (npix > kMaxPathsInFlight) return fail(PBRHIP_EUNSUPPORTED, "more than 2^28 pixels per rank");
  uint32_t chunk_passes = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(d->num_sample, max_paths / npix));
  if ((uint64_t)chunk_passes * npix >= (1ull << 32)) chunk_passes = (uint32_t)(((1ull << 32) - 1) / npix);
  // A working set that is nearly large enough is used as it is: growing it means freeing and re-allocating every path-state
  // array (65 GB at the largest chunk: 1.3 s), and the chunk size does not change the image.  (An eighth of the C5 frame asks
  // for 258 passes = 267.5 M paths where the whole frame had allocated 265.4 M.)
  if (s->hit.n < (size_t)chunk_passes * npix && s->hit.n / npix >= 1 && (double)(s->hit.n / npix) >= 0.75 * chunk_passes)
    chunk_passes = (uint32_t)(s->hit.n / npix);
  *out = chunk_passes;
  return PBRHIP_OK;
}

// The path state every group of a render starts from: the scene's working set (ensure_paths), before a group takes its slice
static PathState base_path_state(const pbrhip_scene* s, bool want_stats) {
  PathState P;
  P.pass_run = 1u;
  P.ray_o.base = s->rec.p, P.ray_d.base = s->rec.p + 1, P.thr.base = s->rec.p + 2, P.L = s->L.p, P.hit = s->hit.p;
  P.rng.base = reinterpret_cast<uint64_t*>(s->rec.p + 3);
  P.hold.base = reinterpret_cast<uint32_t*>(s->rec.p + 3) + 2;
  P.rng4.base = reinterpret_cast<uint4*>(s->rec.p + 3);
  P.sss_sigt.base = s->ssrec.p, P.sss_sigs.base = s->ssrec.p + 1, P.sss_thr.base = s->ssrec.p + 2;
  P.sss_ez.base = s->ssrec.p + 3, P.sss_A = s->sss_A.p;
  P.q_in = s->q[0].p, P.q_out = s->q[1].p, P.q_principled = s->q[2].p, P.q_hair = s->q[3].p, P.q_sss = s->q[4].p, P.q_shadow = s->q[5].p, P.q_shadow_in = s->q[6].p;
  P.sh_d.base = s->srec.p, P.sh_c.base = s->srec.p + 1, P.sh_e = s->sh_e.p;
  P.counts = s->counts.p, P.stats = want_stats ? s->stats.p : nullptr, P.spill = s->spill.p;
  P.first = 0u, P.direct = 0u, P.cam_org[0] = P.cam_org[1] = P.cam_org[2] = 0.f;
  P.heads = nullptr;
  P.susp_turns = 0u, P.susp_out = nullptr, P.susp_in = nullptr, P.shadow_first = 0u;
  P.no_medium = s->has_sss ? 0u : 1u;
  P.wave_log = nullptr, P.wave_log_launch = 0;
  return P;
}

namespace {
struct Group {
  PathState P;
  uint32_t n0, first_pass, npass, slot0;  // paths at the start, pass range, first path slot
  uint32_t n = 0, iters = 0;
  int lane = -1;  // stream / counter / spill slot while active
  bool started = false, finished = false;
  uint32_t enq = 0, seen = 0;     // iterations enqueued / heard of (ring stamps)
  uint32_t stamps[kRingSlots];    // stamp of enqueued iteration i at [i % kRingSlots]
  bool tail_enqueued = false;
  Timer tm;
};

// The chunks of one render, one after the other.  A chunk's passes are split into path groups (plan_groups), and a group runs
// on a lane (stream + counters + spill area + suspend area) while it is active.  Resumable rays and the pipelined host loop
// (round 6; kernels.h::PathState::susp_turns, scene_impl.h::h_ring): every enqueued iteration ends with k_advance, which tells
// the host (ring) what is left; iterations are enqueued ahead of what the host has heard of, their launches sized by the last
// count it saw (live paths only ever decrease: an upper bound).
struct ChunkRun {
  pbrhip_scene* s;
  const pbrhip_render_desc* d;
  const Knobs& k;
  const PathState& P;  // base_path_state
  pbrhip_render_stats& S;
  const volatile unsigned char* cancel;
  size_t* finish_pass;
  float* d_rgba;
  uint32_t* d_count;
  std::chrono::steady_clock::time_point t_begin;
  const uint32_t* pix;  // the pixels the paths of a pass are laid out over: ensure_pixels' list, or the caller's (render_impl)
  uint32_t npix;
  const RaySource* rays;  // the caller's first rays, or null: the scene's camera
  const DScene& sc = s->dscene;
  const bool want_stats = (d->flags & PBRHIP_RENDER_STATS) != 0;
  const bool trace_timing_only = (d->flags & PBRHIP_RENDER_TIMING) == 0 && (d->flags & PBRHIP_RENDER_TIMING_TRACE) != 0;
  const bool want_timing = (d->flags & (PBRHIP_RENDER_TIMING | PBRHIP_RENDER_TIMING_TRACE)) != 0;
  const Camera cam = make_camera(s, d->width, d->height);
  // a user camera: k_generate_camera stores each path's first ray and the first bounce is an ordinary one (PathState::first = 0)
  // ... and so does a ray source: k_generate_rays stores the caller's rays in the same places
  const bool user_cam = s->cam_set && !rays;
  const UserCamera ucam = user_cam ? make_user_camera(s, d->width, d->height) : UserCamera{};
  const uint64_t rng_inc = (d->seed_seq << 1u) | 1u;  // pcg32_srandom (rng.h:30-36)
  const uint32_t tail_paths = k.tail_paths.value_or(d->tail_paths == 0xFFFFFFFFu ? 0u : (d->tail_paths ? d->tail_paths : 262144u));
  const uint32_t want_groups = k.streams.value_or(d->num_streams);
  uint32_t lanes = 1;  // reserve_lanes
  uint32_t wave_log_launches = 0;
  bool stop = false;  // cancelled: what is in flight is dropped, no further chunk starts
  // the chunk in flight
  std::vector<Group> G;
  bool lane_busy[kMaxGroups];
  uint32_t next_start, acc_prefix, active, acc_passes, idle_polls;
  bool cancelled() const { return cancel && __atomic_load_n(cancel, __ATOMIC_RELAXED) != 0; }
  hipStream_t lane_stream(int lane) const { return lane == 0 ? s->stream : s->group_streams[lane - 1]; }
  static size_t ring_slot(int lane, uint32_t i) { return (size_t)(lane * kRingSlots + i % kRingSlots) * 4u; }
  bool reported(const Group& gr, uint32_t i) const {  // has the k_advance of gr's enqueued iteration i written its stamp?
    const volatile uint32_t* slot = s->h_ring + ring_slot(gr.lane, i);
    return __atomic_load_n(&slot[3], __ATOMIC_ACQUIRE) == gr.stamps[i % kRingSlots];
  }
  // lanes for the groups this call can have in flight: the first chunk is the largest, so its plan has the most groups
  int reserve_lanes(uint32_t chunk_passes) {
    const size_t ng = plan_groups(k, std::min(chunk_passes, d->num_sample), npix, want_groups).size();
    lanes = std::max(1u, std::min<uint32_t>((uint32_t)kMaxGroups, (uint32_t)ng));
    if (int rc = ensure_groups(s, lanes)) return rc;
    HIPCHK(s->heads.reserve((size_t)kMaxGroups * kTraceHeads * kHeadStride));
    HIPCHK(s->susp.reserve((size_t)lanes * 2u * kSuspRecords * kSuspWords));  // (2 x 113 MB per lane)
    return PBRHIP_OK;
  }
  // Passes done .. done + np: groups start in order while fewer than k.window of them are in their bulk phase; a group whose
  // oldest enqueued iteration has reported gets more work enqueued behind what is still running; a finished group frees its
  // lane; passes are accumulated (ascending, on the main stream) as soon as every earlier group of the chunk is complete, and
  // *finish_pass follows.  *cancel is read on every turn.  *passes: the passes accumulated.
  int run(uint32_t done, uint32_t np, uint32_t* passes) {
    HIPCHK(hipStreamSynchronize(s->stream));  // clears / the previous chunk's accumulates are done before groups start
    const std::vector<uint32_t> plan = plan_groups(k, np, npix, want_groups);
    G.assign(plan.size(), Group());
    for (uint32_t g = 0, p0 = 0; g < plan.size(); p0 += plan[g], g++) init_group(G[g], done, p0, plan[g]);
    std::fill(lane_busy, lane_busy + kMaxGroups, false);
    next_start = acc_prefix = active = acc_passes = idle_polls = 0;
    for (;;) {
      if (!stop && cancelled()) stop = true;
      if (int rc = start_groups()) return rc;
      if (active == 0) break;
      bool progressed = false;
      for (Group& gr : G)
        if (int rc = poll(gr, &progressed)) return rc;
      if (int rc = accumulate_prefix(done)) return rc;
      if (progressed) {
        idle_polls = 0;
        continue;
      }
      std::this_thread::yield();
      if ((++idle_polls & 1023u) == 0u)
        if (int rc = check_idle_streams()) return rc;
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    *passes = acc_passes;
    return PBRHIP_OK;
  }
  void init_group(Group& gr, uint32_t done, uint32_t p0, uint32_t npass) {
    gr.P = P, gr.n0 = npass * npix, gr.first_pass = d->first_pass + done + p0, gr.npass = npass, gr.slot0 = p0 * npix;
    const size_t off = gr.slot0;
    gr.P.q_in += off, gr.P.q_out += off, gr.P.q_principled += off, gr.P.q_hair += off, gr.P.q_sss += off, gr.P.q_shadow += off, gr.P.q_shadow_in += off;
    for (int a = 0; a < 3; a++) gr.P.cam_org[a] = cam.org[a];
    gr.P.cam = cam, gr.P.pix_index = pix, gr.P.npix = npix, gr.P.width = d->width, gr.P.first_pass = gr.first_pass;
    gr.P.slot0 = gr.slot0, gr.P.seed_seq = d->seed_seq;
    gr.P.pass_run = pass_run_for(k, gr.npass, sc.num_curves != 0);
    gr.P.shadow_first = k.shadow_first, gr.P.susp_turns = 0u;
    gr.tm = Timer{s, want_timing, nullptr};
    gr.tm.only = trace_timing_only ? &S.ms_trace_closest : nullptr;
    gr.tm.idle_acc = &S.ms_host_idle;
  }
  // start groups while the window allows: a group is in its bulk phase until it has handed its remaining paths to k_tail (or,
  // with PBRHIP_BULK_DIV = k, until fewer than 1/k of its paths are alive)
  int start_groups() {
    while (!stop && next_start < G.size()) {
      uint32_t bulk = 0;
      for (const Group& gr : G)
        if (gr.started && !gr.finished && gr.n > std::max<uint64_t>(tail_paths, k.bulk_div ? gr.n0 / k.bulk_div : 0u)) bulk++;
      const int lane = (int)(std::find(lane_busy, lane_busy + lanes, false) - lane_busy);
      if (bulk >= k.window || lane == (int)lanes) break;
      if (int rc = start(G[next_start], lane)) return rc;
      next_start++, active++;
    }
    return PBRHIP_OK;
  }
  int start(Group& gr, int lane) {
    gr.lane = lane, gr.started = true, gr.n = gr.n0, lane_busy[lane] = true;
    hipStream_t gst = lane_stream(lane);
    gr.tm.stream = gst;
    gr.P.counts = s->counts.p + lane * kCntNum;
    gr.P.spill = s->spill.p + (size_t)lane * kSpillWords;
    gr.P.heads = s->heads.p + (size_t)lane * kTraceHeads * kHeadStride;
    HIPCHK(hipMemsetAsync(gr.P.heads, 0, sizeof(uint32_t) * kTraceHeads * kHeadStride, gst));
    uint32_t* hc = s->h_counts + lane * kCntNum;
    memset(hc, 0, sizeof(uint32_t) * kCntNum);
    hc[kCntIn] = gr.n0;
    HIPCHK(hipMemcpyAsync(gr.P.counts, hc, sizeof(uint32_t) * kCntNum, hipMemcpyHostToDevice, gst));
    HIPCHK(gr.tm.begin(&S.ms_generate));
    if (rays) launch_generate_rays(gst, gr.P, *rays, gr.n0);
    else if (user_cam) launch_generate_camera(gst, gr.P, ucam, d->height, gr.n0);
    else launch_generate(gst, gr.P, gr.n0);
    HIPCHK(gr.tm.end());
    return feed(gr);
  }
  // keeps group gr's stream fed: k.pipe_depth iterations ahead of the counts the host has seen (gr.n = the last count heard: an
  // upper bound for every later iteration).  Close to the hand-over to k_tail (live paths <= k.pipe_stop x tail_paths) nothing is
  // enqueued ahead: the hand-over is decided on exact counts (an iteration enqueued ahead would run as a full wavefront iteration
  // on what k_tail finishes faster).
  int feed(Group& gr) {
    if (gr.tail_enqueued) return PBRHIP_OK;
    const uint32_t depth = gr.n < (1u << 18) ? k.pipe_depth_small : k.pipe_depth;
    while (gr.enq - gr.seen < depth) {
      const bool exact = gr.enq == gr.seen;  // the host knows this iteration's input counts
      if (gr.n <= tail_paths) {
        if (int rc = enqueue_iteration(gr, gr.n, true)) return rc;
        break;
      }
      if (!exact && tail_paths && (double)gr.n <= k.pipe_stop * (double)tail_paths) break;
      if (int rc = enqueue_iteration(gr, gr.n, false)) return rc;
    }
    return PBRHIP_OK;
  }
  // one iteration of group gr, its launches sized for at most n_upper live paths (and as many pending shadow rays)
  int enqueue_iteration(Group& gr, uint32_t n_upper, bool to_tail) {
    hipStream_t gst = lane_stream(gr.lane);
    const uint32_t n = std::max(n_upper, 1u);
    gr.P.first = gr.iters++ == 0 && !user_cam && !rays ? 1u : 0u;
    // the launch's suspend records: written by this k_trace, read by the next (alternating halves of the lane's area)
    uint32_t* const susp_lane = s->susp.p + (size_t)gr.lane * 2u * kSuspRecords * kSuspWords;
    gr.P.susp_out = susp_lane + (size_t)(gr.iters & 1u) * kSuspRecords * kSuspWords;
    gr.P.susp_in = susp_lane + (size_t)((gr.iters & 1u) ^ 1u) * kSuspRecords * kSuspWords;
    gr.P.susp_turns = to_tail ? 0u : k.susp_turns;  // (k_tail takes every path to its end: the rays in front of it all finish)
    gr.tm.iteration_begins();
    HIPCHK(gr.tm.begin(&S.ms_trace_closest));
    gr.P.wave_log_launch = wave_log_launches++;
    launch_trace(gst, gr.P, sc, 2 * n, want_stats, k);  // this bounce's closest rays + last bounce's shadow rays
    HIPCHK(gr.tm.end());
    S.n_trace_closest++, S.iterations++;
    if (to_tail) {
      // few live paths: after this bounce's trace (and the pending shadow rays) every path is finished in one launch
      HIPCHK(gr.tm.begin(&S.ms_tail));
      launch_tail(gst, gr.P, sc, n, rng_inc, want_stats, s->has_sss, s->has_textured, k);
      HIPCHK(gr.tm.end());
      S.n_tail++;
      gr.tm.iteration_ends();
      advance(gr, gst);  // nothing was queued: both "in" counts become 0
      gr.tail_enqueued = true;
      return PBRHIP_OK;
    }
    // a first bounce in a scene without hair needs no routing -- every hit takes the principled shader --: the shading kernel
    // walks the group's paths itself (PathState::direct); so does every bounce of a scene of principled surfaces only (no hair,
    // no media: C2 frame -3 %)
    // (media do not matter to a first bounce: no path is inside one before its first shading)
    const bool direct = !s->has_hair && ((gr.P.first && k.first_direct) || (!s->has_sss && k.direct));
    gr.P.direct = direct ? 1u : 0u;
    if (!direct) {
      HIPCHK(gr.tm.begin(&S.ms_surface));
      launch_classify(gst, gr.P, sc, n);
      HIPCHK(gr.tm.end());
      S.n_surface++;
    }
    HIPCHK(gr.tm.begin(&S.ms_shade_principled));
    launch_shade_principled(gst, gr.P, sc, n, rng_inc, s->has_sss, s->has_textured);
    HIPCHK(gr.tm.end());
    if (s->has_hair) {
      HIPCHK(gr.tm.begin(&S.ms_shade_hair));
      launch_shade_hair(gst, gr.P, sc, n, rng_inc);
      HIPCHK(gr.tm.end());
      S.n_shade_hair++;
    }
    if (s->has_sss) {
      HIPCHK(gr.tm.begin(&S.ms_sss_step));
      if (k.sss_walk) launch_sss_walk(gst, gr.P, sc, n, rng_inc, want_stats, k);  // every walk forward to its last event ...
      launch_sss_step(gst, gr.P, sc, n, rng_inc);                                  // ... which the step kernel handles
      HIPCHK(gr.tm.end());
      S.n_sss_step++;
    }
    HIPCHK(gr.tm.begin(&S.ms_compact));
    launch_compact(gst, gr.P, n);
    HIPCHK(gr.tm.end());
    S.n_shade_principled++;
    gr.tm.iteration_ends();
    advance(gr, gst);
    std::swap(gr.P.q_in, gr.P.q_out);
    std::swap(gr.P.q_shadow, gr.P.q_shadow_in);
    return PBRHIP_OK;
  }
  void advance(Group& gr, hipStream_t gst) {
    const uint32_t stamp = ++s->ring_stamp ? s->ring_stamp : ++s->ring_stamp;  // (never 0: the rings start zeroed)
    gr.stamps[gr.enq % kRingSlots] = stamp;
    launch_advance(gst, gr.P, s->d_ring + ring_slot(gr.lane, gr.enq), stamp);
    gr.enq++;
  }
  // what group gr's ring says: the iterations that have reported, then whether the group is complete -- or abandoned: a
  // cancelled render drops what is in flight --, else more work for it
  int poll(Group& gr, bool* progressed) {
    if (!gr.started || gr.finished) return PBRHIP_OK;
    while (gr.seen < gr.enq && reported(gr, gr.seen)) {
      const volatile uint32_t* slot = s->h_ring + ring_slot(gr.lane, gr.seen);
      *progressed = true;
      if (slot[2]) return fail(PBRHIP_EOVERFLOW, "BVH traversal stack overflow");
      gr.n = std::max(slot[0], slot[1]);  // pending shadow rays need one more trace
      gr.seen++;
      if (k.trace_sched)
        fprintf(stderr, "sched %8.3f ms  group %d (passes %u)  iter %u of %u enqueued  live %u\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                (int)(&gr - G.data()), gr.npass, gr.seen, gr.enq, gr.n);
    }
    if (gr.seen == gr.enq && (gr.n == 0 || stop)) {
      HIPCHK(hipStreamSynchronize(lane_stream(gr.lane)));  // (its last k_advance has written the stamp: the stream is about to be idle)
      HIPCHK(gr.tm.collect());
      gr.finished = gr.n == 0;
      if (!gr.finished) gr.started = false;
      lane_busy[gr.lane] = false, active--;
      *progressed = true;
      return PBRHIP_OK;
    }
    if (gr.n != 0 && !stop) return feed(gr);
    return PBRHIP_OK;
  }
  // accumulate the complete prefix of the chunk's groups
  int accumulate_prefix(uint32_t done) {
    hipStream_t st = s->stream;
    while (acc_prefix < G.size() && G[acc_prefix].finished) {
      const Group& gr = G[acc_prefix];
      PathState PA = P;
      PA.L = P.L + gr.slot0, PA.pass_run = gr.P.pass_run;
      Timer tm{s, want_timing, st};
      tm.only = trace_timing_only ? &S.ms_trace_closest : nullptr;
      HIPCHK(tm.begin(&S.ms_accumulate));
      launch_accumulate(st, PA, pix, npix, gr.npass, d_rgba, d_count);
      HIPCHK(tm.end());
      HIPCHK(hipGetLastError());
      if (want_timing && !trace_timing_only) {  // (trace-only timing has nothing to collect here and must not stall the host)
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(tm.collect());
      }
      acc_passes += gr.npass, acc_prefix++;
      S.samples += (uint64_t)gr.npass * npix;
      if (finish_pass) __atomic_store_n(finish_pass, (size_t)done + acc_passes, __ATOMIC_RELEASE);  // render.cc:224-231
    }
    return PBRHIP_OK;
  }
  // (now and then: a stream that failed, or went idle without its last stamp, must not leave the loop spinning)
  int check_idle_streams() {
    for (Group& gr : G) {
      if (!gr.started || gr.finished || gr.seen == gr.enq) continue;
      const hipError_t q = hipStreamQuery(lane_stream(gr.lane));
      if (q == hipErrorNotReady) continue;
      HIPCHK(q);
      if (!reported(gr, gr.enq - 1u)) return fail(PBRHIP_EHIP, "render: a path group's stream went idle without reporting its last iteration");
    }
    return PBRHIP_OK;
  }
};
}  // namespace

// PBRHIP_WAVE_LOG: the log of the render's k_trace waves, as the kernels wrote it (scripts/wave_log.py reads it)
static int write_wave_log(const DevBuf<unsigned long long>& log, const char* path) {
  std::vector<unsigned long long> h((size_t)kWaveLogLaunches * kWaveLogWaves * 4);
  HIPCHK(hipMemcpy(h.data(), log.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (FILE* f = fopen(path, "wb")) {
    fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
    fclose(f);
  }
  return PBRHIP_OK;
}

static double ratio(unsigned long long a, unsigned long long b) { return a / (double)std::max<unsigned long long>(1, b); }

// the device's statistics counters (PBRHIP_RENDER_STATS) into S; PBRHIP_PV_STATS prints the traversal's on stderr
static int read_render_stats(pbrhip_scene* s, const Knobs& k, pbrhip_render_stats* S) {
  unsigned long long hs[kStatNum];
  HIPCHK(hipMemcpy(hs, s->stats.p, sizeof(hs), hipMemcpyDeviceToHost));
  S->closest_rays = hs[kStatClosestRays] - hs[kStatSuspended] - hs[kStatHeld], S->closest_nodes = hs[kStatClosestNodes];  // (a suspended ray is counted by the launch that suspends it and by the one that resumes it)
  S->suspended_rays = hs[kStatSuspended] + hs[kStatSuspendedShadow];
  S->closest_tris = hs[kStatClosestTris], S->closest_curves = hs[kStatClosestCurves];
  S->shadow_rays = hs[kStatShadowRays] - hs[kStatSuspendedShadow], S->shadow_nodes = hs[kStatShadowNodes];
  S->tail_closest_rays = hs[kStatTailClosestRays], S->tail_shadow_rays = hs[kStatTailShadowRays];
  S->pruned_rays = hs[kStatPrunedRays];
  s->shaft.culled = hs[kStatCulledShadow], s->shaft.clear_rays = hs[kStatGridClearRays], s->shaft.pair_tests = hs[kStatGridPairTests];  // (pbrhip_scene_shadow_grid_info)
  S->shadow_tris = hs[kStatShadowTris], S->shadow_curves = hs[kStatShadowCurves];
  if (!k.pv_stats) return PBRHIP_OK;
  fprintf(stderr, "pv closest: it node %llu tri %llu curve %llu refill %llu | lanes/iter node %.1f tri %.1f curve %.1f\n",
          hs[kStatPvItNode], hs[kStatPvItTri], hs[kStatPvItCurve], hs[kStatPvItRefill],
          ratio(hs[kStatPvLnNode], hs[kStatPvItNode]), ratio(hs[kStatPvLnTri], hs[kStatPvItTri]), ratio(hs[kStatPvLnCurve], hs[kStatPvItCurve]));
  const unsigned long long cyc = hs[kStatCycNode] + hs[kStatCycTri] + hs[kStatCycCurve] + hs[kStatCycRefill];
  fprintf(stderr, "pv cycles per wave turn (shader clock, lane 0 of every wave, from one turn's start to the next's): node %.0f  triangle %.0f  curve %.0f  refill %.0f | share of the waves' time: %.3f %.3f %.3f %.3f\n",
          ratio(hs[kStatCycNode], hs[kStatPvItNode]), ratio(hs[kStatCycTri], hs[kStatPvItTri]),
          ratio(hs[kStatCycCurve], hs[kStatPvItCurve]), ratio(hs[kStatCycRefill], hs[kStatPvItRefill]),
          ratio(hs[kStatCycNode], cyc), ratio(hs[kStatCycTri], cyc), ratio(hs[kStatCycCurve], cyc), ratio(hs[kStatCycRefill], cyc));
  fprintf(stderr, "pv steps per closest-hit ray (<=16, 32, 64, 128, 256, 512, 1024, more):");
  for (int i = 0; i < 8; i++) fprintf(stderr, " %llu", hs[kStatStepHist0 + i]);
  fprintf(stderr, " | max %llu | most loop turns of one wave (whole render) %llu\n", hs[kStatMaxSteps], hs[kStatMaxWaveIters]);
  fprintf(stderr, "pv steps per shadow ray:");
  for (int i = 0; i < 8; i++) fprintf(stderr, " %llu", hs[kStatAnyHist0 + i]);
  fprintf(stderr, " | max %llu\n", hs[kStatAnyMaxSteps]);
  fprintf(stderr, "walk: nodes %llu prims %llu | wave turns: traversal %llu, step / refill %llu | cycles per traversal turn %.0f, per step / refill turn %.0f (share %.3f)\n", hs[kStatWalkNodes], hs[kStatWalkTris],
          hs[kStatWalkTurns], hs[kStatWalkSteps], ratio(hs[kStatWalkCycTrav], hs[kStatWalkTurns]), ratio(hs[kStatWalkCycStep], hs[kStatWalkSteps]),
          ratio(hs[kStatWalkCycStep], hs[kStatWalkCycStep] + hs[kStatWalkCycTrav]));
  return PBRHIP_OK;
}

int pb::render_impl(pbrhip_scene* s, const pbrhip_render_desc* d, const volatile unsigned char* cancel, float* d_rgba,
                    uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats, const uint32_t* d_pixels, uint32_t num_pixels,
                    const RaySource* rays) {
  const auto t_begin = std::chrono::steady_clock::now();
  if (int rc = check_render_desc(s, d)) return rc;
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t npx_img = (size_t)d->width * d->height;
  if (!(d->flags & PBRHIP_RENDER_NO_CLEAR)) {  // PrepareRendering: layer->Resize + Clear (render.cc:99-100)
    HIPCHK(hipMemsetAsync(d_rgba, 0, npx_img * 4 * sizeof(float), st));
    HIPCHK(hipMemsetAsync(d_count, 0, npx_img * sizeof(uint32_t), st));
  }
  if (finish_pass) __atomic_store_n(finish_pass, (size_t)0, __ATOMIC_RELEASE);
  pbrhip_render_stats S;
  memset(&S, 0, sizeof(S));
  if (int rc = ensure_pixels(s, k, d->width, d->height, d->tile_rank, d->tile_world ? d->tile_world : 1, d->shard_block)) return rc;
  if (int rc = ensure_shadow_grid(s, k)) return rc;  // (kept unless a refit, a replication or a knob asks for another)
  const uint32_t* const pix = d_pixels ? d_pixels : s->path_pix.p;
  const uint32_t npix = d_pixels ? num_pixels : s->pk_npix;
  const bool want_stats = (d->flags & PBRHIP_RENDER_STATS) != 0;
  uint32_t done = 0;  // passes accumulated into the layer
  if (npix > 0 && d->num_sample > 0) {
    uint32_t chunk_passes = 0;
    if (int rc = chunk_passes_for(s, d, k, npix, &chunk_passes)) return rc;
    if (int rc = ensure_paths(s, (size_t)chunk_passes * npix)) return rc;
    PathState P = base_path_state(s, want_stats);
    DevBuf<unsigned long long> wave_log;  // (PBRHIP_WAVE_LOG)
    if (k.wave_log) {
      HIPCHK(wave_log.reserve((size_t)kWaveLogLaunches * kWaveLogWaves * 4));
      HIPCHK(hipMemsetAsync(wave_log.p, 0, sizeof(unsigned long long) * kWaveLogLaunches * kWaveLogWaves * 4, st));
      P.wave_log = wave_log.p;
    }
    HIPCHK(hipMemsetAsync(s->stats.p, 0, sizeof(unsigned long long) * kStatNum, st));
    // the environment's share of NEE events: the light count is known once the scene is committed
    s->dscene.env_p = s->dscene.num_lights ? 0.5f : 1.0f;
    s->dscene.env_area_scale = 1.0f - s->dscene.env_p;
    RaySource src{};
    if (rays) src = *rays, src.base_pass = d->first_pass, src.height = d->height;
    ChunkRun run{s, d, k, P, S, cancel, finish_pass, d_rgba, d_count, t_begin, pix, npix, rays ? &src : nullptr};
    if (int rc = run.reserve_lanes(chunk_passes)) return rc;
    while (done < d->num_sample && !run.stop && !run.cancelled()) {  // render.cc:217
      uint32_t passes = 0;
      if (int rc = run.run(done, std::min(chunk_passes, d->num_sample - done), &passes)) return rc;
      done += passes;
      S.chunks++;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (k.wave_log)
      if (int rc = write_wave_log(wave_log, k.wave_log)) return rc;
    if (want_stats)
      if (int rc = read_render_stats(s, k, &S)) return rc;
  } else {
    HIPCHK(hipStreamSynchronize(st));
    done = d->num_sample;
    if (finish_pass) __atomic_store_n(finish_pass, (size_t)done, __ATOMIC_RELEASE);
  }
  S.passes_done = done;
  S.node_bytes = trace_uses_wide(s->dscene, k) ? sizeof(QNode) : sizeof(BvhNode);
  S.curve_bytes = trace_uses_wide(s->dscene, k) ? 32 : 64;
  S.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if (stats) *stats = S;
  return PBRHIP_OK;
}

extern "C" int pbrhip_render_device(pbrhip_scene* s, const pbrhip_render_desc* d, const volatile unsigned char* cancel,
                                    float* d_rgba, uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats) {
  return guarded([&]() -> int {
    if (!s || !d || !d_rgba || !d_count) return fail(PBRHIP_EINVAL, "render: NULL argument");
    return render_impl(s, d, cancel, d_rgba, d_count, finish_pass, stats);
  });
}

extern "C" int pbrhip_render(pbrhip_scene* s, const pbrhip_render_desc* d, const volatile unsigned char* cancel,
                             float* rgba, uint32_t* count, size_t* finish_pass, pbrhip_render_stats* stats) {
  return guarded([&]() -> int {
    if (!s || !d || !rgba || !count) return fail(PBRHIP_EINVAL, "render: NULL argument");
    auto t_begin = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(s->device));
    size_t npx = (size_t)d->width * d->height;
    HIPCHK(s->own_rgba.reserve(npx * 4));
    HIPCHK(s->own_count.reserve(npx));
    if (d->flags & PBRHIP_RENDER_NO_CLEAR) {
      HIPCHK(hipMemcpyAsync(s->own_rgba.p, rgba, npx * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
      HIPCHK(hipMemcpyAsync(s->own_count.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    }
    int rc = render_impl(s, d, cancel, s->own_rgba.p, s->own_count.p, finish_pass, stats);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(rgba, s->own_rgba.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(count, s->own_count.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (stats) stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return PBRHIP_OK;
  });
}

// ------------------------------------------------------------------ rendering along caller-supplied rays
// what the ray-list entry points check before anything touches a device: pointers, then the shape of the ray buffer, then the scene
int pb::check_ray_args(const char* who, const pbrhip_scene* s, const pbrhip_render_desc* d, const void* rays, uint32_t ray_passes,
                       uint32_t camera_draws) {
  if (!d || !rays) return fail(PBRHIP_EINVAL, "%s: NULL descriptor or rays", who);
  if (ray_passes != 1u && ray_passes != d->num_sample)
    return fail(PBRHIP_EINVAL, "%s: ray_passes %u is neither 1 nor num_sample %u", who, ray_passes, d->num_sample);
  if (camera_draws > kMaxCameraDraws) return fail(PBRHIP_EINVAL, "%s: camera_draws %u (at most %u)", who, camera_draws, kMaxCameraDraws);
  if (!s) return fail(PBRHIP_EINVAL, "%s: NULL scene", who);
  return PBRHIP_OK;
}

extern "C" int pbrhip_render_rays_device(pbrhip_scene* s, const pbrhip_render_desc* d, const void* d_rays, uint32_t ray_passes,
                                         uint32_t camera_draws, void* stream, const volatile unsigned char* cancel, float* d_rgba,
                                         uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats) {
  return guarded([&]() -> int {
    if (!d_rgba || !d_count) return fail(PBRHIP_EINVAL, "render_rays: NULL layer");
    if (int rc = check_ray_args("render_rays", s, d, d_rays, ray_passes, camera_draws)) return rc;
    if (int rc = check_render_desc(s, d)) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    RaySource src{};
    src.rays = static_cast<const float4*>(d_rays), src.ray_passes = ray_passes, src.camera_draws = camera_draws;
    return render_impl(s, d, cancel, d_rgba, d_count, finish_pass, stats, nullptr, 0, &src);
  });
}

extern "C" int pbrhip_render_rays(pbrhip_scene* s, const pbrhip_render_desc* d, const pbrhip_ray* rays, uint32_t ray_passes,
                                  uint32_t camera_draws, const volatile unsigned char* cancel, float* rgba, uint32_t* count,
                                  size_t* finish_pass, pbrhip_render_stats* stats) {
  return guarded([&]() -> int {
    if (!rgba || !count) return fail(PBRHIP_EINVAL, "render_rays: NULL layer");
    if (int rc = check_ray_args("render_rays", s, d, rays, ray_passes, camera_draws)) return rc;
    if (int rc = check_render_desc(s, d)) return rc;
    auto t_begin = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(s->device));
    const size_t npx = (size_t)d->width * d->height, nrays = npx * ray_passes;
    HIPCHK(s->own_rgba.reserve(npx * 4));
    HIPCHK(s->own_count.reserve(npx));
    HIPCHK(s->own_rays.reserve(2 * nrays));
    if (nrays) HIPCHK(hipMemcpyAsync(s->own_rays.p, rays, nrays * sizeof(pbrhip_ray), hipMemcpyHostToDevice, s->stream));
    if (d->flags & PBRHIP_RENDER_NO_CLEAR) {
      HIPCHK(hipMemcpyAsync(s->own_rgba.p, rgba, npx * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
      HIPCHK(hipMemcpyAsync(s->own_count.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    }
    RaySource src{};
    src.rays = s->own_rays.p, src.ray_passes = ray_passes, src.camera_draws = camera_draws;
    if (int rc = render_impl(s, d, cancel, s->own_rgba.p, s->own_count.p, finish_pass, stats, nullptr, 0, &src)) return rc;
    HIPCHK(hipMemcpyAsync(rgba, s->own_rgba.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(count, s->own_count.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (stats) stats->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return PBRHIP_OK;
  });
}
