// pbrhip.cpp -- C ABI (include/pbrhip.h): host scene store, commit (light tables, BVH, upload) and the
// wavefront render loop that drives kernels.hip.  Host C++ only; device code lives in kernels.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "env_tables.h"
#include "feature_kernels.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_principled_param) == sizeof(PrincipledParam), "param layout");
static_assert(sizeof(pbrhip_hair_param) == sizeof(HairParam), "param layout");
static_assert(sizeof(pbrhip_hit) == sizeof(HookHit), "hit layout");
static_assert(sizeof(pbrhip_ray) == 32, "ray layout");
static_assert(sizeof(LightRec) == 80, "light record layout");

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
  k.sss_entry = u32("PBRHIP_SSS_ENTRY", 1u) != 0u;
  k.sss_foreign = u32("PBRHIP_SSS_FOREIGN", 3u);
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
static const HostMesh* inst_mesh(const pbrhip_scene* s, uint32_t instance_id, uint32_t geom_id) {
  const HostInstance& in = s->instances[instance_id];
  return &s->meshes[s->locals[in.local_scene][geom_id]];
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

// ------------------------------------------------------------------ commit
static V3 mesh_vertex(const HostMesh& m, uint32_t prim, int k) {
  const float* p = m.vertices.data() + (size_t)m.vid[prim * 3 + k] * 4;
  return V3(p[0], p[1], p[2]);
}
// What the raytracer sees of an instance (raytracer_impl.cc:61-81: the transform goes to Embree and nowhere else):
// v' = v * M with the translation row, in this order of operations (the checker uses the same expression).
static V3 xf_point(const float* m, V3 v) {
  return V3(m[0] * v.x + m[4] * v.y + m[8] * v.z + m[12], m[1] * v.x + m[5] * v.y + m[9] * v.z + m[13],
            m[2] * v.x + m[6] * v.y + m[10] * v.z + m[14]);
}
static V3 world_vertex(const HostInstance& in, const HostMesh& m, uint32_t prim, int k) {
  const V3 v = mesh_vertex(m, prim, k);
  return in.identity ? v : xf_point(in.xf, v);
}
// control points xyzr of curve `prim` as the raytracer sees them (the radius is not scaled)
static void world_curve(const HostInstance& in, const HostMesh& m, uint32_t prim, float out[16]) {
  const float* cps = m.cverts.data() + (size_t)m.cidx[prim] * 4;
  for (int c = 0; c < 4; c++) {
    V3 v(cps[4 * c], cps[4 * c + 1], cps[4 * c + 2]);
    if (!in.identity) v = xf_point(in.xf, v);
    out[4 * c] = v.x, out[4 * c + 1] = v.y, out[4 * c + 2] = v.z, out[4 * c + 3] = cps[4 * c + 3];
  }
}
// TriangleMesh::FetchFaceArea (mesh/triangle-mesh.cc:113-124)
static float face_area(const HostMesh& m, uint32_t prim) {
  V3 p0 = mesh_vertex(m, prim, 0), p1 = mesh_vertex(m, prim, 1), p2 = mesh_vertex(m, prim, 2);
  return length(cross(p1 - p0, p2 - p0)) * 0.5f;
}

// LightManager::RegisterInstanceMesh (light-manager.cc:79-184)
static void register_lights(pbrhip_scene* s, uint32_t instance_id) {
  HostInstance& in = s->instances[instance_id];
  size_t ng = in.light_ids.size();
  in.has_area_light.assign(ng, 0);
  in.area_lights.assign(ng, HostAreaLight());
  for (size_t g = 0; g < ng; g++) {
    const std::vector<uint32_t>& ids = in.light_ids[g];
    if (ids.empty()) continue;
    const HostMesh& m = *inst_mesh(s, instance_id, (uint32_t)g);
    if (m.kind != 0) continue;
    uint32_t nf = m.nfaces;
    bool have = false;
    for (uint32_t f = 0; f < nf; f++) have = have || ids[f] != kNone;
    if (!have) continue;
    HostAreaLight& a = in.area_lights[g];
    in.has_area_light[g] = 1;
    a.light_param_ids = ids;
    a.choose_prob.assign(nf, 0.f);
    for (uint32_t f = 0; f < nf; f++) {
      float intensity = 0.0f;
      if (ids[f] != kNone) intensity = spectrum_norm(s->light_params[ids[f]]);
      a.choose_prob[f] = intensity * face_area(m, f);
    }
    a.intensity_sum = std::accumulate(a.choose_prob.begin(), a.choose_prob.end(), 0.0f);
    const float sum = a.intensity_sum;
    for (float& v : a.choose_prob) v = v / sum;
    a.cdf = a.choose_prob;
    for (uint32_t f = 0; nf > 0 && f < nf - 1u; f++) a.cdf[f + 1u] += a.cdf[f];
    a.area_pdf.assign(nf, 0.f);
    for (uint32_t f = 0; f < nf; f++)
      if (ids[f] != kNone) a.area_pdf[f] = 1.0f / face_area(m, f);
  }
}
// LightManager::Commit (light-manager.cc:29-77)
static void commit_lights(pbrhip_scene* s) {
  s->lights.clear();
  double intensity_sum = 0.0;
  for (uint32_t i = 0; i < s->instances.size(); i++) {
    HostInstance& in = s->instances[i];
    for (uint32_t g = 0; g < in.area_lights.size(); g++) {
      if (!in.has_area_light[g]) continue;
      in.area_lights[g].global_id = (uint32_t)s->lights.size();
      HostLight L;
      L.choose_prob = in.area_lights[g].intensity_sum;
      L.instance_id = i, L.geom_id = g;
      intensity_sum += (double)L.choose_prob;
      s->lights.push_back(L);
    }
  }
  for (HostLight& L : s->lights) L.choose_prob = (float)((double)L.choose_prob / intensity_sum);
  s->light_cdf.resize(s->lights.size());
  for (size_t l = 0; l < s->lights.size(); l++) s->light_cdf[l] = s->lights[l].choose_prob;
  for (size_t l = 0; !s->light_cdf.empty() && l < s->light_cdf.size() - 1u; l++) s->light_cdf[l + 1u] += s->light_cdf[l];
}

static Material make_material(const HostMaterial& hm) {
  Material m;
  memset(&m, 0, sizeof(m));
  m.kind = hm.kind;
  m.bsdf = default_bsdf();
  if (hm.kind == kMatPrincipled) {
    m.bsdf = param_to_bsdf(hm.pr);
    m.param = hm.pr;
    medium_coefficients(m.bsdf, m.sss_sigt, m.sss_sigs, m.sss_wthr);  // (only read when the subsurface closure is picked)
    m.textured = (hm.pr.base_color_tex_id != kNone || hm.pr.subsurface_color_tex_id != kNone) ? 1u : 0u;
  } else {
    m.hair = hair_param_to_bsdf(hm.hr);
  }
  return m;
}

// End points of linear piece `sub` of a cubic Bezier (control points xyzr): B(sub/4) and B((sub+1)/4), evaluated with
// the arithmetic of the intersection contract (Bernstein weights, products summed left to right, single precision,
// no contraction) so that every back end tests the same segment.
static void curve_piece(const float* cp, uint32_t sub, float a[4], float b[4]) {
  for (uint32_t e = 0; e < 2; e++) {
    const float u = (float)(sub + e) * 0.25f, s = 1.0f - u;
    const float b0 = s * s * s, b1 = 3.0f * u * s * s, b2 = 3.0f * u * u * s, b3 = u * u * u;
    for (int k = 0; k < 4; k++) (e ? b : a)[k] = ((cp[k] * b0 + cp[4 + k] * b1) + cp[8 + k] * b2) + cp[12 + k] * b3;
  }
}

// Flattens the primitives in canonical (instance, geom, prim, sub) order: the index is the gid.
static int flatten_prims(const pbrhip_scene* s, std::vector<PrimRef>* prims) {
  for (uint32_t i = 0; i < s->instances.size(); i++)
    for (uint32_t g = 0; g < s->instances[i].material_ids.size(); g++) {
      const HostMesh& m = *inst_mesh(s, i, g);
      if (s->instances[i].material_ids[g].size() != m.num_prims())
        return fail(PBRHIP_ESIZE, "material param error (instance %u geom %u)", i, g);
      for (uint32_t p = 0; p < m.num_prims(); p++)
        for (uint32_t sub = 0; sub < (m.kind == 1 ? 4u : 1u); sub++) prims->push_back({i, g, p, (uint32_t)m.kind, sub});
    }
  return PBRHIP_OK;
}

// Scene bounds (rtcGetSceneBounds, raytracer_impl.cc:199-202; they place the camera): the union of the instances'
// bounds.  An RTC_GEOMETRY_TYPE_INSTANCE (raytracer_impl.cc:61-81) reports the box of the transformed CORNERS of its local
// scene's box -- larger than the box of the transformed geometry under rotation or shear; an instance whose matrix is
// bit for bit the identity reports the local box.  Local box: triangles by their corners, curves by the hull of their
// control points widened by the largest control radius.  (The tree is built over the transformed primitives.)
static void scene_bounds(pbrhip_scene* s) {
  const float inf = std::numeric_limits<float>::infinity();
  float bmin[3] = {inf, inf, inf}, bmax[3] = {-inf, -inf, -inf};
  for (uint32_t i = 0; i < s->instances.size(); i++) {
    const HostInstance& inst = s->instances[i];
    float ll[3] = {inf, inf, inf}, lh[3] = {-inf, -inf, -inf};
    bool any = false;
    for (uint32_t g = 0; g < inst.material_ids.size(); g++) {
      const HostMesh& m = *inst_mesh(s, i, g);
      for (uint32_t p = 0; p < m.num_prims(); p++) {
        any = true;
        if (m.kind == 0) {
          for (int c = 0; c < 3; c++) {
            const V3 v = mesh_vertex(m, p, c);
            const float a[3] = {v.x, v.y, v.z};
            for (int k = 0; k < 3; k++) ll[k] = fminf(ll[k], a[k]), lh[k] = fmaxf(lh[k], a[k]);
          }
        } else {
          float r = 0.f, cl[3] = {inf, inf, inf}, ch[3] = {-inf, -inf, -inf};
          for (int c = 0; c < 4; c++) {
            const float* cp = m.cverts.data() + ((size_t)m.cidx[p] + c) * 4;
            r = fmaxf(r, fabsf(cp[3]));
            for (int k = 0; k < 3; k++) cl[k] = fminf(cl[k], cp[k]), ch[k] = fmaxf(ch[k], cp[k]);
          }
          for (int k = 0; k < 3; k++) ll[k] = fminf(ll[k], cl[k] - r), lh[k] = fmaxf(lh[k], ch[k] + r);
        }
      }
    }
    if (!any) continue;
    if (inst.identity) {
      for (int k = 0; k < 3; k++) bmin[k] = fminf(bmin[k], ll[k]), bmax[k] = fmaxf(bmax[k], lh[k]);
    } else {
      for (int c = 0; c < 8; c++) {
        const V3 v = xf_point(inst.xf, V3((c & 1) ? lh[0] : ll[0], (c & 2) ? lh[1] : ll[1], (c & 4) ? lh[2] : ll[2]));
        const float a[3] = {v.x, v.y, v.z};
        for (int k = 0; k < 3; k++) bmin[k] = fminf(bmin[k], a[k]), bmax[k] = fmaxf(bmax[k], a[k]);
      }
    }
  }
  memcpy(s->bmin, bmin, sizeof(bmin));
  memcpy(s->bmax, bmax, sizeof(bmax));
}

// The box (world space) and kind of every primitive: what the tree is built over.
static void prim_boxes(const pbrhip_scene* s, const std::vector<PrimRef>& prims, std::vector<float>* lo, std::vector<float>* hi,
                       std::vector<uint8_t>* kinds) {
  const float inf = std::numeric_limits<float>::infinity();
  const uint32_t np = (uint32_t)prims.size();
  lo->assign(3 * (size_t)np, 0.f), hi->assign(3 * (size_t)np, 0.f), kinds->assign(np, 0);
  for (uint32_t g = 0; g < np; g++) {
    const PrimRef& pr = prims[g];
    const HostMesh& m = *inst_mesh(s, pr.instance_id, pr.geom_id);
    const HostInstance& inst = s->instances[pr.instance_id];
    float l[3] = {inf, inf, inf}, h[3] = {-inf, -inf, -inf};
    (*kinds)[g] = (uint8_t)pr.kind;
    if (pr.kind == 0) {
      for (int c = 0; c < 3; c++) {
        V3 v = world_vertex(inst, m, pr.prim_id, c);
        float a[3] = {v.x, v.y, v.z};
        for (int k = 0; k < 3; k++) l[k] = std::min(l[k], a[k]), h[k] = std::max(h[k], a[k]);
      }
    } else {
      float cps[16];
      world_curve(inst, m, pr.prim_id, cps);
      // BVH box of this piece: its two end points widened by the larger end radius (the ribbon between them never
      // leaves that box, and a hit is reported at the depth of the axis point)
      float a[4], b[4];
      curve_piece(cps, pr.sub, a, b);
      const float r = std::max(fabsf(a[3]), fabsf(b[3]));
      for (int k = 0; k < 3; k++) l[k] = std::min(a[k], b[k]) - r, h[k] = std::max(a[k], b[k]) + r;
    }
    for (int k = 0; k < 3; k++) (*lo)[3 * g + k] = l[k], (*hi)[3 * g + k] = h[k];
  }
}

// Light records: one per (light, prim), concatenated; heads[l] is light l's stretch of them.
static void light_records(const pbrhip_scene* s, std::vector<LightHead>* heads, std::vector<LightRec>* lrecs,
                          std::vector<float>* lprim_cdf) {
  heads->resize(s->lights.size());
  for (size_t l = 0; l < s->lights.size(); l++) {
    const HostLight& L = s->lights[l];
    const HostAreaLight& a = s->instances[L.instance_id].area_lights[L.geom_id];
    const HostMesh& m = *inst_mesh(s, L.instance_id, L.geom_id);
    (*heads)[l].first = (uint32_t)lrecs->size();
    (*heads)[l].count = m.nfaces;
    for (uint32_t f = 0; f < m.nfaces; f++) {
      LightRec r;
      memset(&r, 0, sizeof(r));
      V3 p0 = mesh_vertex(m, f, 0), p1 = mesh_vertex(m, f, 1), p2 = mesh_vertex(m, f, 2);
      V3 n = vnormalize(cross(p1 - p0, p2 - p1));  // CalcGeometryNormal (triangle-mesh.cc:181-184)
      r.p0[0] = p0.x, r.p0[1] = p0.y, r.p0[2] = p0.z;
      r.p1[0] = p1.x, r.p1[1] = p1.y, r.p1[2] = p1.z;
      r.p2[0] = p2.x, r.p2[1] = p2.y, r.p2[2] = p2.z;
      r.normal[0] = n.x, r.normal[1] = n.y, r.normal[2] = n.z;
      // light-manager.h:68-70,149-150: choose_light * choose_prim * prim_area_pdf, in that order
      r.pdf = L.choose_prob * a.choose_prob[f] * a.area_pdf[f];
      if (a.light_param_ids[f] != kNone) {
        V3 e = s->light_params[a.light_param_ids[f]];
        r.emission[0] = e.x, r.emission[1] = e.y, r.emission[2] = e.z;
      }
      lrecs->push_back(r);
      lprim_cdf->push_back(a.cdf[f]);
    }
  }
}

// One slot: the four 16-byte words `sl` and the ShadeRec `sr` of primitive `pr` with canonical id g (what pbrhip_scene_commit stages
// for every slot and pbrhip_scene_refit for the dirty ones).
static int slot_and_shade(const pbrhip_scene* s, const PrimRef& pr, uint32_t g, const std::vector<LightHead>& heads, float4* sl, ShadeRec& sr) {
  {
    const HostInstance& in = s->instances[pr.instance_id];
    const HostMesh& m = *inst_mesh(s, pr.instance_id, pr.geom_id);
    uint32_t mat = in.material_ids[pr.geom_id][pr.prim_id];
    if (mat != kNone && (mat >= s->materials.size() || mat >= 0x00FFFFFFu)) return fail(PBRHIP_EINVAL, "material id %u out of range", mat);
    memset(&sr, 0, sizeof(sr));
    uint32_t flags = 0, lightrec = kNone;
    if (mat == kNone) flags |= kSlotMatNone;
    else if (s->materials[mat].kind == kMatHair) flags |= kSlotMatHair;
    for (int c = 0; c < 4; c++) sl[c] = make_float4(0, 0, 0, 0);
    if (pr.kind == 0) {
      for (int c = 0; c < 3; c++) {
        // traversal: what Embree sees (the transformed triangle); shading: the mesh's own corners -- the geometric normal
        // Embree reports for an instance is in the instance's local space and pbrlab uses it as it is
        const V3 w = world_vertex(in, m, pr.prim_id, c);
        sl[c] = make_float4(w.x, w.y, w.z, 0.f);
      }
      {
        // the two normals every hit on this triangle would otherwise compute from its corners (ShadeRec, dscene.h): the kernels'
        // own functions, evaluated here
        const V3 v0 = mesh_vertex(m, pr.prim_id, 0), v1 = mesh_vertex(m, pr.prim_id, 1), v2 = mesh_vertex(m, pr.prim_id, 2);
        const V3 ng = normalize_raw(cross(v1 - v0, v2 - v0));
        const V3 nf = vnormalize(cross(v1 - v0, v2 - v1));  // CalcGeometryNormal, triangle-mesh.cc:181-184
        sr.ng[0] = ng.x, sr.ng[1] = ng.y, sr.ng[2] = ng.z;
        sr.ns_flat[0] = nf.x, sr.ns_flat[1] = nf.y, sr.ns_flat[2] = nf.z;
      }
      uint32_t a = m.nid[pr.prim_id * 3 + 0], b = m.nid[pr.prim_id * 3 + 1], c = m.nid[pr.prim_id * 3 + 2];
      if (a != kNone && b != kNone && c != kNone) {  // triangle-mesh.cc:81-84
        flags |= kSlotHasNormals;
        const uint32_t idx[3] = {a, b, c};
        for (int q = 0; q < 3; q++) {
          const float* n = m.normals.data() + (size_t)idx[q] * 4;
          sr.n[3 * q + 0] = n[0], sr.n[3 * q + 1] = n[1], sr.n[3 * q + 2] = n[2];
        }
      }
      if (in.has_area_light[pr.geom_id]) {
        const HostAreaLight& al = in.area_lights[pr.geom_id];
        if (al.light_param_ids[pr.prim_id] != kNone) lightrec = heads[al.global_id].first + pr.prim_id;
      }
      uint32_t ta = m.tid[pr.prim_id * 3 + 0], tb = m.tid[pr.prim_id * 3 + 1], tc = m.tid[pr.prim_id * 3 + 2];
      if (ta != kNone && tb != kNone && tc != kNone) {  // triangle-mesh.cc:130-133
        flags |= kSlotHasUV;
        const uint32_t idx[3] = {ta, tb, tc};
        for (int q = 0; q < 3; q++) {
          sr.uv[2 * q + 0] = m.texcoords[(size_t)idx[q] * 2 + 0];
          sr.uv[2 * q + 1] = m.texcoords[(size_t)idx[q] * 2 + 1];
        }
      }
    } else {
      flags |= kSlotIsCurve;
      const float* cps = m.cverts.data() + (size_t)m.cidx[pr.prim_id] * 4;  // local: the tangent (= Ng) shading uses
      float wcps[16];
      world_curve(in, m, pr.prim_id, wcps);
      float a[4], b[4];
      curve_piece(wcps, pr.sub, a, b);
      sl[0] = make_float4(a[0], a[1], a[2], a[3]);
      sl[1] = make_float4(b[0], b[1], b[2], b[3]);
      sl[2] = make_float4(__builtin_bit_cast(float, pr.sub), 0.f, 0.f, 0.f);
      // shading needs the cubic itself (tangent = dP/du at the hit): control points xyzr in words 8..23 of the record
      float* w = reinterpret_cast<float*>(&sr);
      for (int c = 0; c < 16; c++) w[8 + c] = cps[c];
    }
    sr.gid = g, sr.lightrec = lightrec;
    sr.matflags = (mat == kNone ? 0x00FFFFFFu : mat) | (flags << 24);
    const uint32_t route = ((flags & kSlotMatHair) ? kHitHair : 0u) | ((flags & kSlotMatNone) ? kHitNoMaterial : 0u) |
                           (lightrec != kNone ? kHitLight : 0u) |
                           ((flags & (kSlotHasNormals | kSlotHasUV | kSlotIsCurve)) ? kHitMore : 0u);
    sl[2].w = __builtin_bit_cast(float, route);  // travels with the hit record (Hit::slot)
    sr.instance_id = pr.instance_id, sr.geom_id = pr.geom_id, sr.prim_id = pr.prim_id;
  }
  return PBRHIP_OK;
}
// Leaf-ordered slots (traversal geometry, 64 B each) + one 128-byte ShadeRec per slot (everything shading needs).
static int slots_and_shade(const pbrhip_scene* s, const std::vector<PrimRef>& prims, const std::vector<uint32_t>& slot_gid,
                           const std::vector<LightHead>& heads, std::vector<float4>* slots, std::vector<ShadeRec>* shade) {
  const uint32_t ns = (uint32_t)slot_gid.size();
  slots->resize(4 * (size_t)ns);
  shade->resize(ns);
  for (uint32_t k = 0; k < ns; k++)
    if (int rc = slot_and_shade(s, prims[slot_gid[k]], slot_gid[k], heads, &(*slots)[4 * (size_t)k], (*shade)[k])) return rc;
  return PBRHIP_OK;
}

// One box per light over all primitives of its mesh, packed two per node (an odd last one is stored twice).
static std::vector<BvhNode> light_boxes(const std::vector<LightHead>& heads, const std::vector<LightRec>& lrecs) {
  std::vector<BvhNode> boxes((heads.size() + 1) / 2);
  for (size_t l = 0; l < heads.size(); l++) {
    float lo3[3] = {INFINITY, INFINITY, INFINITY}, hi3[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t f = heads[l].first; f < heads[l].first + heads[l].count; f++)
      for (const float* p : {lrecs[f].p0, lrecs[f].p1, lrecs[f].p2})
        for (int a = 0; a < 3; a++) lo3[a] = std::min(lo3[a], p[a]), hi3[a] = std::max(hi3[a], p[a]);
    BvhNode& nd = boxes[l / 2];
    if (l % 2 == 0) memset(&nd, 0, sizeof(nd)), nd.set_box(1, lo3, hi3);
    nd.set_box(int(l % 2), lo3, hi3);
  }
  return boxes;
}

extern "C" int pbrhip_scene_commit(pbrhip_scene* s) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  for (uint32_t i = 0; i < s->instances.size(); i++) register_lights(s, i);
  commit_lights(s);

  std::vector<PrimRef> prims;
  if (int rc = flatten_prims(s, &prims)) return rc;
  uint32_t np = (uint32_t)prims.size();
  if (np >= (1u << 27)) return fail(PBRHIP_EUNSUPPORTED, "too many primitives (%u)", np);
  std::vector<float> lo, hi;
  std::vector<uint8_t> kinds;
  prim_boxes(s, prims, &lo, &hi, &kinds);
  scene_bounds(s);

  FlatBvh bvh;
  bool gpu_built = false;
  uint32_t num_nodes = 0;
  const int builder = k.bvh >= 0 ? k.bvh : s->bvh_builder;
  if ((builder == PBRHIP_BVH_GPU_LBVH || builder == PBRHIP_BVH_GPU_LBVH_WIDE) && np > 0) {
    HIPCHK(s->d_nodes.reserve(std::max<size_t>(np > 1 ? np - 1 : 1, 1) + np));  // nodes, then one 64-byte slot per primitive
    HIPCHK(build_bvh_gpu(s->stream, lo, hi, kinds, s->d_nodes.p, &bvh.slot_gid, &bvh.depth));
    if (bvh.depth > (uint32_t)kStackDepth) {
      // a Morton-order tree over badly distributed primitives can be deeper than the traversal stack: use the SAH tree
      fprintf(stderr, "pbrhip: GPU-built BVH is %u deep (stack %d): building on the host instead\n", bvh.depth, kStackDepth);
      bvh = FlatBvh();
    } else {
      gpu_built = true;
      num_nodes = np > 1 ? np - 1 : 1;
    }
  }
  if (!gpu_built) {
    build_bvh(lo, hi, kinds, &bvh);
    num_nodes = (uint32_t)bvh.nodes.size();
  }
  s->bvh_built_on_gpu = gpu_built;
  if (bvh.depth > (uint32_t)kStackDepth)
    return fail(PBRHIP_EOVERFLOW, "BVH depth %u exceeds the traversal stack (%d)", bvh.depth, kStackDepth);
  s->bvh_depth = bvh.depth;

  std::vector<LightHead> heads;
  std::vector<LightRec> lrecs;
  std::vector<float> lprim_cdf;
  light_records(s, &heads, &lrecs, &lprim_cdf);
  const uint32_t ns = (uint32_t)bvh.slot_gid.size();
  if (ns > kHitSlotMask) return fail(PBRHIP_EINVAL, "%u traversal primitives: at most %u are supported", ns, kHitSlotMask);
  std::vector<float4> slots;
  std::vector<ShadeRec> shade;
  if (int rc = slots_and_shade(s, prims, bvh.slot_gid, heads, &slots, &shade)) return rc;
  std::vector<Material> mats(s->materials.size());
  s->has_hair = s->has_sss = s->has_textured = false;
  for (size_t i = 0; i < mats.size(); i++) {
    const HostMaterial& hm = s->materials[i];
    if (hm.kind == kMatPrincipled)
      for (uint32_t t : {hm.pr.base_color_tex_id, hm.pr.subsurface_color_tex_id})
        if (t != kNone && t >= s->tex_descs.size()) return fail(PBRHIP_EINVAL, "material %zu: texture id %u out of range", i, t);
    mats[i] = make_material(s->materials[i]);
    if (mats[i].textured) s->has_sss = s->has_textured = true;  // a subsurface_color / base_color map can switch the SSS closure on per hit
    s->has_hair = s->has_hair || mats[i].kind == kMatHair;
    s->has_sss = s->has_sss || (mats[i].kind == kMatPrincipled && mats[i].bsdf.enable_subsurface);
  }

  hipStream_t st = s->stream;
  // nodes and primitive slots share one allocation (both are 64-byte items: the traversal addresses either as
  // base + index * 64, with slot k at index num_nodes + k)
  static_assert(sizeof(BvhNode) == 64 && sizeof(float4) == 16, "node / slot footprint");
  if (!gpu_built) {
    HIPCHK(s->d_nodes.reserve((size_t)num_nodes + ns));
    if (num_nodes) HIPCHK(hipMemcpyAsync(s->d_nodes.p, bvh.nodes.data(), (size_t)num_nodes * sizeof(BvhNode), hipMemcpyHostToDevice, st));
  }
  if (ns) HIPCHK(hipMemcpyAsync(s->d_nodes.p + num_nodes, slots.data(), (size_t)ns * 64, hipMemcpyHostToDevice, st));
  // The Q tree of the traversal kernels (host-built trees; PBRHIP_WIDE=0 at commit: none): the binary tree collapsed to four
  // children per node with quantised boxes (64 B per node), followed by its own compact triangle leaves and curve records
  // (bvh_build.cpp::build_qlayout, dscene.h::QNode).
  QLayout q;
  size_t q_tri_words = 0, q_pts = 0;
  if (!gpu_built && num_nodes && k.wide) {
    build_qlayout(bvh, slots, kinds, &q);
    q_tri_words = q.tri.size(), q_pts = q.pts.size();
    if (k.debug) fprintf(stderr, "pbrhip: commit: curve leaves of the Q tree (counted over the collapse's visits): %zu of one piece, %zu of two pieces\n", q.leaves_one, q.leaves_pair);
  }
  // PBRHIP_BVH_GPU_LBVH_WIDE: the GPU-built tree collapsed on the device (qtree_gpu.hip) straight into d_wide / d_qhit; the nodes come
  // back (64 B each) for the stack need and the random walks' entries.  A tree that cannot be kept is dropped for the binary one.
  bool wide_on_gpu = false;
  if (gpu_built && builder == PBRHIP_BVH_GPU_LBVH_WIDE && k.wide) {
    const bool tri_pairs = std::all_of(kinds.begin(), kinds.end(), [](uint8_t kd) { return kd == 0; });
    QCollapse qc;
    HIPCHK(hipStreamSynchronize(st));  // (the slots are on the device: what follows is the collapse's own time)
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    auto alloc = [&](size_t words, size_t hits, float4** w, uint32_t** h) -> hipError_t {
      hipError_t e = s->d_wide.reserve(words);
      if (e == hipSuccess) e = s->d_qhit.reserve(hits);
      *w = s->d_wide.p, *h = s->d_qhit.p;
      return e;
    };
    HIPCHK(collapse_qtree_gpu(st, s->d_nodes.p, ns, reinterpret_cast<const float4*>(s->d_nodes.p + num_nodes), tri_pairs, alloc, &qc));
    const double ms_collapse = ms_since(t_start);
    const char* why = !qc.fits ? "a record index overflows its reference" : (!qc.quantised ? "a node cannot be quantised" : nullptr);
    if (!why) {
      q.nodes.resize(qc.nodes);
      HIPCHK(hipMemcpyAsync(q.nodes.data(), s->d_wide.p, (size_t)qc.nodes * sizeof(QNode), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      q.stack_need = qtree_stack_need(q.nodes);
      if (q.stack_need > (uint32_t)kStackDepth) why = "its traversal needs more than the stack";
    }
    if (k.debug)
      fprintf(stderr, "pbrhip: commit: Q tree on the device: %u nodes in %u levels, collapse %.2f ms (of which allocation %.2f ms), download + stack need %.2f ms\n",
              qc.nodes, qc.levels, ms_collapse, qc.alloc_ms, ms_since(t_start) - ms_collapse);
    if (why) {
      fprintf(stderr, "pbrhip: the Q tree of the GPU-built BVH is dropped (%s): rendering the binary tree\n", why);
      q = QLayout();
    } else {
      wide_on_gpu = true;
      q_tri_words = qc.tri_words, q_pts = qc.pts;
    }
  }
  const std::vector<QNode>& wide = q.nodes;
  {  // the bounds of every instance's primitive boxes: what the random walks' entries are cut around (kept for pbrhip_scene_refit)
    const size_t ninst = s->instances.size();
    std::vector<float>&ilo = s->inst_lo, &ihi = s->inst_hi;
    ilo.assign(3 * ninst, INFINITY), ihi.assign(3 * ninst, -INFINITY);
    for (uint32_t g = 0; g < np; g++)
      for (size_t a = 0, i = prims[g].instance_id; a < 3; a++)
        ilo[3 * i + a] = std::min(ilo[3 * i + a], lo[3 * (size_t)g + a]), ihi[3 * i + a] = std::max(ihi[3 * i + a], hi[3 * (size_t)g + a]);
  }
  // Where the random walks' rays start (dscene.h::SssEntry): per instance, the cut of the Q tree around its bounds
  std::vector<SssEntry> sss_entries;
  if (!wide.empty() && k.sss_entry) {  // (whatever the materials are now: pbrhip_scene_update_* can switch subsurface on later)
    const std::vector<float>&ilo = s->inst_lo, &ihi = s->inst_hi;
    // (every foreign reference costs each walk ray a slab test: a deeper entry is only worth so many)
    const uint32_t max_foreign = std::min(k.sss_foreign, kSssMaxForeign);
    const auto t_entries = std::chrono::steady_clock::now();
    sss_entries = build_sss_entries(wide, ilo, ihi, max_foreign);
    if (k.debug) fprintf(stderr, "pbrhip: commit: random walks' entries over %zu wide nodes: %.2f ms\n", wide.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entries).count());
    for (size_t i = 0; i < sss_entries.size() && k.debug; i++)
      if (sss_entries[i].entry) fprintf(stderr, "pbrhip: commit: instance %zu: random walks start at Q node %u with %u foreign references\n", i, sss_entries[i].entry, sss_entries[i].nforeign);
  }
  if (sss_entries.empty()) s->d_sss_entries.release();
  else HIPCHK(s->d_sss_entries.upload(sss_entries, st));
  if (wide.empty()) s->d_wide.release(), s->d_qhit.release();
  if (k.debug) fprintf(stderr, "pbrhip: commit: %u binary nodes, %zu wide nodes, %zu slots, %zu triangle leaves + %zu points in the Q tree\n", num_nodes, wide.size(), (size_t)ns, q_tri_words / kTriPairWords, q_pts);
  if (!wide.empty() && !wide_on_gpu) {
    HIPCHK(s->d_wide.reserve(wide.size() * 4 + q.tri.size() + q.pts.size()));
    HIPCHK(hipMemcpyAsync(s->d_wide.p, wide.data(), wide.size() * sizeof(QNode), hipMemcpyHostToDevice, st));
    if (!q.tri.empty()) HIPCHK(hipMemcpyAsync(s->d_wide.p + wide.size() * 4, q.tri.data(), q.tri.size() * 16, hipMemcpyHostToDevice, st));
    if (!q.pts.empty()) HIPCHK(hipMemcpyAsync(s->d_wide.p + wide.size() * 4 + q.tri.size(), q.pts.data(), q.pts.size() * 16, hipMemcpyHostToDevice, st));
    HIPCHK(s->d_qhit.upload(q.hit, st));
  }
  HIPCHK(s->d_shade.upload(shade, st));
  HIPCHK(s->d_materials.upload(mats, st));
  HIPCHK(s->d_light_cdf.upload(s->light_cdf, st));
  HIPCHK(s->d_heads.upload(heads, st));
  HIPCHK(s->d_lprim_cdf.upload(lprim_cdf, st));
  HIPCHK(s->d_lrecs.upload(lrecs, st));
  HIPCHK(s->d_light_boxes.upload(light_boxes(heads, lrecs), st));
  HIPCHK(s->d_tex_pixels.upload(s->tex_pixels, st));
  HIPCHK(s->d_tex_descs.upload(s->tex_descs, st));
  HIPCHK(hipStreamSynchronize(st));
  DScene& d = s->dscene;
  d.nodes = s->d_nodes.p, d.slots = reinterpret_cast<const float4*>(s->d_nodes.p + num_nodes), d.shade = s->d_shade.p;
  d.materials = s->d_materials.p, d.light_cdf = s->d_light_cdf.p;
  d.light_heads = s->d_heads.p, d.lprim_cdf = s->d_lprim_cdf.p, d.lrecs = s->d_lrecs.p, d.light_boxes = s->d_light_boxes.p;
  d.num_nodes = num_nodes, d.num_slots = ns, d.num_lights = (uint32_t)s->lights.size(), d.num_lrecs = (uint32_t)lrecs.size();
  d.num_materials = (uint32_t)mats.size();
  d.tex_pixels = s->d_tex_pixels.p, d.textures = s->d_tex_descs.p, d.num_textures = (uint32_t)s->tex_descs.size();
  d.num_curves = 0;
  for (uint8_t kd : kinds) d.num_curves += kd ? 1u : 0u;
  d.wide = wide.empty() ? nullptr : s->d_wide.p, d.wide_nodes = (uint32_t)wide.size();
  d.q_tri0 = (uint32_t)wide.size() * 4u, d.q_pt0 = d.q_tri0 + (uint32_t)q_tri_words, d.q_hitcode = wide.empty() ? nullptr : s->d_qhit.p;
  d.top_nodes = gpu_built ? 0u : std::min<uint32_t>(num_nodes, (uint32_t)kTopNodes);
  d.wide_top_nodes = std::min<uint32_t>((uint32_t)wide.size(), (uint32_t)kTopNodes);
  // light sampling works on the meshes' local positions (light-manager.h:128-136 "TODO transform"), the raytracer on the
  // transformed ones: the doomed-path pretest against the light primitives (kernels.hip::misses_all_lights) is only the
  // traversal's own test when the two coincide
  d.sss_entries = sss_entries.empty() ? nullptr : s->d_sss_entries.p, d.num_sss_entries = (uint32_t)sss_entries.size();
  d.lights_transformed = 0;
  for (const HostLight& L : s->lights) d.lights_transformed |= s->instances[L.instance_id].identity ? 0u : 1u;
  s->wide_stack_need = wide.empty() ? 0u : q.stack_need, s->wide_built_on_gpu = wide_on_gpu;
  // what pbrhip_scene_refit needs of this commit; the device scene is the model's again
  s->slot_gid = std::move(bvh.slot_gid), s->light_heads = std::move(heads), s->q_points = wide.empty() ? 0 : q_pts;
  s->rf_plan.release();
  s->dirty_inst.assign(s->instances.size(), 0), s->stale = false;
  s->committed = true;
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

static int update_material(pbrhip_scene* s, uint32_t id, const HostMaterial& hm) {
  // validate everything first: a rejected call leaves the host material, has_sss and the device copy as they were
  if (id >= s->materials.size()) return fail(PBRHIP_EINVAL, "material id %u out of range", id);
  if (s->materials[id].kind != hm.kind) return fail(PBRHIP_EINVAL, "material %u is of the other kind", id);
  if (s->committed && hm.kind == kMatPrincipled)
    for (uint32_t t : {hm.pr.base_color_tex_id, hm.pr.subsurface_color_tex_id})
      if (t != kNone && t >= s->tex_descs.size()) return fail(PBRHIP_EINVAL, "texture id %u out of range", t);
  if (s->committed) {
    HIPCHK(hipSetDevice(s->device));
    const Material m = make_material(hm);
    HIPCHK(hipMemcpyAsync(s->d_materials.p + id, &m, sizeof(m), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->has_sss = s->has_sss || (m.kind == kMatPrincipled && (m.bsdf.enable_subsurface || m.textured));
    s->has_textured = s->has_textured || (m.kind == kMatPrincipled && m.textured);
  }
  s->materials[id] = hm;
  return PBRHIP_OK;
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
  return PBRHIP_OK;
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

// the tight box of a staged slot: what prim_boxes computes for its primitive, from the very numbers the slot holds
static void slot_tight_box(const float4* sl, bool curve, float lo[3], float hi[3]) {
  const float a[3] = {sl[0].x, sl[0].y, sl[0].z}, b[3] = {sl[1].x, sl[1].y, sl[1].z}, c[3] = {sl[2].x, sl[2].y, sl[2].z};
  const float r = std::max(fabsf(sl[0].w), fabsf(sl[1].w));
  for (int k = 0; k < 3; k++) {
    if (curve) lo[k] = std::min(a[k], b[k]) - r, hi[k] = std::max(a[k], b[k]) + r;
    else lo[k] = std::min(std::min(a[k], b[k]), c[k]), hi[k] = std::max(std::max(a[k], b[k]), c[k]);
  }
}

extern "C" int pbrhip_scene_refit(pbrhip_scene* s) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  if (s->replica) return fail(PBRHIP_ESTATE, "scene_refit: a replica holds no geometry (refit the source scene and replicate it again)");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  if (!s->stale) return PBRHIP_OK;
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  DScene& d = s->dscene;
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
  const auto t_host = now();
  const size_t ninst = s->instances.size();
  s->dirty_inst.resize(ninst, 0);
  // light tables: positions, areas and with them every probability (what commit runs, on the whole scene: the tables are small)
  bool lights_dirty = false;
  for (size_t i = 0; i < ninst; i++)
    if (s->dirty_inst[i])
      for (int has : s->instances[i].has_area_light) lights_dirty = lights_dirty || has != 0;
  std::vector<LightRec> lrecs;
  std::vector<float> lprim_cdf;
  if (lights_dirty) {
    for (uint32_t i = 0; i < ninst; i++) register_lights(s, i);
    commit_lights(s);
    light_records(s, &s->light_heads, &lrecs, &lprim_cdf);
  }
  // the dirty slots and their ShadeRecs, packed for one upload: index | 64 B | 128 B; the dirty instances' bounds from their new boxes
  std::vector<PrimRef> prims;
  if (int rc = flatten_prims(s, &prims)) return rc;
  const uint32_t ns = d.num_slots;
  if (s->slot_gid.size() != ns || prims.size() != ns) return fail(PBRHIP_ESTATE, "scene_refit: the model no longer has the committed topology");
  std::vector<uint32_t> dirty;
  for (uint32_t slot = 0; slot < ns; slot++)
    if (s->dirty_inst[prims[s->slot_gid[slot]].instance_id]) dirty.push_back(slot);
  const uint32_t m = (uint32_t)dirty.size();
  const size_t idx_words = ((size_t)m + 3) / 4;
  std::vector<float4> packed(idx_words + 12 * (size_t)m, make_float4(0, 0, 0, 0));
  std::vector<float> ilo = s->inst_lo, ihi = s->inst_hi;
  for (size_t i = 0; i < ninst; i++)
    if (s->dirty_inst[i])
      for (int a = 0; a < 3; a++) ilo[3 * i + a] = INFINITY, ihi[3 * i + a] = -INFINITY;
  for (uint32_t e = 0; e < m; e++) {
    const uint32_t g = s->slot_gid[dirty[e]];
    float4* sl = &packed[idx_words + 4 * (size_t)e];
    ShadeRec sr;
    if (int rc = slot_and_shade(s, prims[g], g, s->light_heads, sl, sr)) return rc;
    reinterpret_cast<uint32_t*>(packed.data())[e] = dirty[e];
    memcpy(&packed[idx_words + 4 * (size_t)m + 8 * (size_t)e], &sr, sizeof(sr));
    float lo[3], hi[3];
    slot_tight_box(sl, prims[g].kind != 0, lo, hi);
    for (size_t a = 0, i = prims[g].instance_id; a < 3; a++) ilo[3 * i + a] = std::min(ilo[3 * i + a], lo[a]), ihi[3 * i + a] = std::max(ihi[3 * i + a], hi[a]);
  }
  float keep_min[3], keep_max[3];  // (a failed refit leaves the scene as stale as it was)
  memcpy(keep_min, s->bmin, 12), memcpy(keep_max, s->bmax, 12);
  scene_bounds(s);
  const double ms_host = ms_since(t_host);

  const auto t_up = now();
  HIPCHK(s->rf_packed.upload(packed, st));
  HIPCHK(scatter_slots_gpu(st, s->rf_packed.p, m, ns, reinterpret_cast<float4*>(s->d_nodes.p + d.num_nodes), reinterpret_cast<float4*>(s->d_shade.p)));
  if (lights_dirty) {
    HIPCHK(s->d_light_cdf.upload(s->light_cdf, st));
    HIPCHK(s->d_heads.upload(s->light_heads, st));
    HIPCHK(s->d_lprim_cdf.upload(lprim_cdf, st));
    HIPCHK(s->d_lrecs.upload(lrecs, st));
    HIPCHK(s->d_light_boxes.upload(light_boxes(s->light_heads, lrecs), st));
  }
  if (k.debug) HIPCHK(hipStreamSynchronize(st));
  const double ms_upload = ms_since(t_up);

  RefitTree t;
  t.nodes = s->d_nodes.p, t.nb = d.num_nodes, t.ns = ns;
  if (d.wide) {
    t.q = reinterpret_cast<QNode*>(s->d_wide.p), t.nq = d.wide_nodes;
    t.tri = s->d_wide.p + d.q_tri0, t.tri_words = d.q_pt0 - d.q_tri0, t.tri_pairs = d.num_curves == 0;
    t.pts = s->d_wide.p + d.q_pt0, t.hit = s->d_qhit.p, t.npts = s->q_points;
  }
  RefitTimes rt;
  HIPCHK(refit_tree_gpu(st, t, k.debug, &s->rf_plan, &rt));
  if (rt.failed) {
    memcpy(s->bmin, keep_min, 12), memcpy(s->bmax, keep_max, 12);
    return fail(PBRHIP_EHIP, "scene_refit: %s; the scene stays stale (pbrhip_scene_commit rebuilds it)",
                (rt.failed & 1u) ? "a node of the Q tree cannot be quantised" : "the committed tree holds an index out of range");
  }
  // the random walks' entries: a cut is only sound for the bounds it was made for
  const auto t_entries = now();
  if (d.wide && d.sss_entries) {
    std::vector<QNode> wide(d.wide_nodes);
    HIPCHK(hipMemcpyAsync(wide.data(), s->d_wide.p, wide.size() * sizeof(QNode), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const std::vector<SssEntry> entries = build_sss_entries(wide, ilo, ihi, std::min(k.sss_foreign, kSssMaxForeign));
    HIPCHK(s->d_sss_entries.upload(entries, st));
    HIPCHK(hipStreamSynchronize(st));
    d.sss_entries = s->d_sss_entries.p, d.num_sss_entries = (uint32_t)entries.size();
  }
  HIPCHK(hipStreamSynchronize(st));
  if (k.debug)
    fprintf(stderr, "pbrhip: refit: %u of %u slots dirty: host staging %.2f ms, upload + scatter %.2f ms, plan %.2f ms, pack + trees %.2f ms (%u + %u levels), Q-node download + walk entries %.2f ms\n",
            m, ns, ms_host, ms_upload, rt.plan_ms, rt.trees_ms, rt.bin_levels, rt.q_levels, ms_since(t_entries));
  if (lights_dirty) {
    d.light_cdf = s->d_light_cdf.p, d.light_heads = s->d_heads.p, d.lprim_cdf = s->d_lprim_cdf.p, d.lrecs = s->d_lrecs.p, d.light_boxes = s->d_light_boxes.p;
    d.num_lights = (uint32_t)s->lights.size(), d.num_lrecs = (uint32_t)lrecs.size();
  }
  d.lights_transformed = 0;
  for (const HostLight& L : s->lights) d.lights_transformed |= s->instances[L.instance_id].identity ? 0u : 1u;
  s->inst_lo = std::move(ilo), s->inst_hi = std::move(ihi);
  s->dirty_inst.assign(ninst, 0), s->stale = false;
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
static UserCamera make_user_camera(const pbrhip_scene* s, uint32_t width, uint32_t height) {
  double f[3], r[3], u[3], up[3];
  for (int k = 0; k < 3; k++) f[k] = (double)s->cam_lookat[k] - s->cam_eye[k], up[k] = s->cam_up[k];
  const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  for (int k = 0; k < 3; k++) f[k] /= fl;
  r[0] = f[1] * up[2] - f[2] * up[1], r[1] = f[2] * up[0] - f[0] * up[2], r[2] = f[0] * up[1] - f[1] * up[0];
  const double rl = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int k = 0; k < 3; k++) r[k] /= rl;
  u[0] = r[1] * f[2] - r[2] * f[1], u[1] = r[2] * f[0] - r[0] * f[2], u[2] = r[0] * f[1] - r[1] * f[0];
  UserCamera c;
  for (int k = 0; k < 3; k++) c.eye[k] = s->cam_eye[k], c.f[k] = (float)f[k], c.r[k] = (float)r[k], c.u[k] = (float)u[k];
  const double h = tan((double)s->cam_vfov * M_PI / 360.0);
  c.h = (float)h, c.ha = (float)(h * width / height);
  c.lens = s->cam_lens, c.focus = s->cam_focus > 0.0f ? s->cam_focus : (float)fl;
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
static Camera make_camera(const pbrhip_scene* s, uint32_t width, uint32_t height) {
  const float *bmin = s->bmin, *bmax = s->bmax;
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

static int check_render_desc(const pbrhip_scene* s, const pbrhip_render_desc* d) {
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
  const DScene& sc = s->dscene;
  const uint32_t npix = s->pk_npix;
  const bool want_stats = (d->flags & PBRHIP_RENDER_STATS) != 0;
  const bool trace_timing_only = (d->flags & PBRHIP_RENDER_TIMING) == 0 && (d->flags & PBRHIP_RENDER_TIMING_TRACE) != 0;
  const bool want_timing = (d->flags & (PBRHIP_RENDER_TIMING | PBRHIP_RENDER_TIMING_TRACE)) != 0;
  const Camera cam = make_camera(s, d->width, d->height);
  // a user camera: k_generate_camera stores each path's first ray and the first bounce is an ordinary one (PathState::first = 0)
  const bool user_cam = s->cam_set;
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
    gr.P.cam = cam, gr.P.pix_index = s->path_pix.p, gr.P.npix = npix, gr.P.width = d->width, gr.P.first_pass = gr.first_pass;
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
    if (user_cam) launch_generate_camera(gst, gr.P, ucam, d->height, gr.n0);
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
    gr.P.first = gr.iters++ == 0 && !user_cam ? 1u : 0u;
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
      launch_accumulate(st, PA, s->path_pix.p, npix, gr.npass, d_rgba, d_count);
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
static int read_render_stats(const pbrhip_scene* s, const Knobs& k, pbrhip_render_stats* S) {
  unsigned long long hs[kStatNum];
  HIPCHK(hipMemcpy(hs, s->stats.p, sizeof(hs), hipMemcpyDeviceToHost));
  S->closest_rays = hs[kStatClosestRays] - hs[kStatSuspended] - hs[kStatHeld], S->closest_nodes = hs[kStatClosestNodes];  // (a suspended ray is counted by the launch that suspends it and by the one that resumes it)
  S->suspended_rays = hs[kStatSuspended] + hs[kStatSuspendedShadow];
  S->closest_tris = hs[kStatClosestTris], S->closest_curves = hs[kStatClosestCurves];
  S->shadow_rays = hs[kStatShadowRays] - hs[kStatSuspendedShadow], S->shadow_nodes = hs[kStatShadowNodes];
  S->tail_closest_rays = hs[kStatTailClosestRays], S->tail_shadow_rays = hs[kStatTailShadowRays];
  S->pruned_rays = hs[kStatPrunedRays];
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
                    uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats) {
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
  const uint32_t npix = s->pk_npix;
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
    ChunkRun run{s, d, k, P, S, cancel, finish_pass, d_rgba, d_count, t_begin};
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

// ------------------------------------------------------------------ feature buffers and denoiser
// What a first hit on a material adds to the albedo sum: rgb | the base-colour map's id (kNone: the rgb stands).  Principled: base_color.
// Hair: base_color when it is coloured by RGB; for melanin the colour whose sigma_a under hair_param_to_bsdf's RGB mapping
// (sigma_a = (log c / poly(beta_n))^2) is the material's: c = exp(-sqrt(sigma_a) poly(beta_n)), in double, rounded once.
static float4 feature_albedo(const HostMaterial& hm) {
  if (hm.kind == kMatPrincipled) return make_float4(hm.pr.base_color[0], hm.pr.base_color[1], hm.pr.base_color[2], __builtin_bit_cast(float, hm.pr.base_color_tex_id));
  const float none = __builtin_bit_cast(float, kNone);
  if (hm.hr.coloring_hair == 0) return make_float4(hm.hr.base_color[0], hm.hr.base_color[1], hm.hr.base_color[2], none);
  const V3 sa = hair_param_to_bsdf(hm.hr).sigma_a;
  const double bn = hm.hr.azimuthal_roughness;
  const double poly = 5.969 - 0.215 * bn + 2.532 * bn * bn - 10.73 * bn * bn * bn + 5.574 * bn * bn * bn * bn + 0.245 * bn * bn * bn * bn * bn;
  return make_float4((float)exp(-sqrt((double)sa.x) * poly), (float)exp(-sqrt((double)sa.y) * poly), (float)exp(-sqrt((double)sa.z) * poly), none);
}

// the body of pbrhip_render_features_device: device pointers on the scene's device, each may be null
static int features_impl(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_albedo_hits, float* d_normal_depth, uint32_t* d_count) {
  if (int rc = check_render_desc(s, d)) return rc;
  if (d->num_sample == 0) return fail(PBRHIP_EINVAL, "render_features: no samples");
  if ((uint64_t)d->first_pass + d->num_sample > (1ull << 32)) return fail(PBRHIP_EINVAL, "render_features: the passes do not fit 32 bits");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t npx_img = (size_t)d->width * d->height;
  if (!(d->flags & PBRHIP_RENDER_NO_CLEAR)) {
    if (d_albedo_hits) HIPCHK(hipMemsetAsync(d_albedo_hits, 0, npx_img * 4 * sizeof(float), st));
    if (d_normal_depth) HIPCHK(hipMemsetAsync(d_normal_depth, 0, npx_img * 4 * sizeof(float), st));
    if (d_count) HIPCHK(hipMemsetAsync(d_count, 0, npx_img * sizeof(uint32_t), st));
  }
  if (int rc = ensure_pixels(s, k, d->width, d->height, d->tile_rank, d->tile_world ? d->tile_world : 1, d->shard_block)) return rc;
  const uint32_t npix = s->pk_npix;
  if (npix == 0 || (!d_albedo_hits && !d_normal_depth && !d_count)) {
    HIPCHK(hipStreamSynchronize(st));
    return PBRHIP_OK;
  }
  std::vector<float4> albedo(std::max<size_t>(s->materials.size(), 1), make_float4(0.f, 0.f, 0.f, 0.f));
  for (size_t i = 0; i < s->materials.size(); i++) albedo[i] = feature_albedo(s->materials[i]);  // (from the host model: material updates are seen)
  HIPCHK(s->feat_albedo.upload(albedo, st));
  HIPCHK(s->counts.reserve(kCntNum * kMaxGroups));
  HIPCHK(hipMemsetAsync(s->counts.p, 0, sizeof(uint32_t) * kCntNum, st));
  HIPCHK(s->spill.reserve(kSpillWords));
  FeatureArgs a;
  a.user = s->cam_set ? 1u : 0u;
  a.ucam = s->cam_set ? make_user_camera(s, d->width, d->height) : UserCamera{};
  a.cam = s->cam_set ? Camera{} : make_camera(s, d->width, d->height);
  a.width = d->width, a.height = d->height, a.seed_seq = d->seed_seq;
  a.pix = s->path_pix.p, a.npix = npix;
  a.mat_albedo = s->feat_albedo.p;
  a.albedo_hits = reinterpret_cast<float4*>(d_albedo_hits), a.normal_depth = reinterpret_cast<float4*>(d_normal_depth), a.count = d_count;
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  // max_paths_in_flight bounds the samples of one launch as it bounds the paths of a render's chunk; a pixel's sums continue from
  // chunk to chunk in pass order, so the split is invisible in the result
  uint32_t chunk = d->num_sample;
  if (d->max_paths_in_flight) chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(d->num_sample, d->max_paths_in_flight / npix));
  for (uint32_t done = 0; done < d->num_sample; done += chunk) {
    a.first_pass = d->first_pass + done, a.npass = std::min(chunk, d->num_sample - done);
    launch_features(st, s->dscene, a, k);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(s->h_counts, s->counts.p, sizeof(uint32_t) * kCntNum, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (s->h_counts[kCntOverflow]) return fail(PBRHIP_EOVERFLOW, "BVH traversal stack overflow");
  return PBRHIP_OK;
}

extern "C" int pbrhip_render_features_device(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_albedo_hits, float* d_normal_depth,
                                             uint32_t* d_count) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_features: NULL argument");
    return features_impl(s, d, d_albedo_hits, d_normal_depth, d_count);
  });
}

extern "C" int pbrhip_render_features(pbrhip_scene* s, const pbrhip_render_desc* d, float* albedo_hits, float* normal_depth, uint32_t* count) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_features: NULL argument");
    if (int rc = check_render_desc(s, d)) return rc;
    HIPCHK(hipSetDevice(s->device));
    const size_t npx = (size_t)d->width * d->height;
    DevBuf<float> d_a, d_n;
    DevBuf<uint32_t> d_c;
    if (albedo_hits) HIPCHK(d_a.reserve(npx * 4));
    if (normal_depth) HIPCHK(d_n.reserve(npx * 4));
    if (count) HIPCHK(d_c.reserve(npx));
    if (d->flags & PBRHIP_RENDER_NO_CLEAR) {
      if (albedo_hits) HIPCHK(hipMemcpyAsync(d_a.p, albedo_hits, npx * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
      if (normal_depth) HIPCHK(hipMemcpyAsync(d_n.p, normal_depth, npx * 4 * sizeof(float), hipMemcpyHostToDevice, s->stream));
      if (count) HIPCHK(hipMemcpyAsync(d_c.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    }
    if (int rc = features_impl(s, d, d_a.p, d_n.p, d_c.p)) return rc;
    if (albedo_hits) HIPCHK(hipMemcpyAsync(albedo_hits, d_a.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (normal_depth) HIPCHK(hipMemcpyAsync(normal_depth, d_n.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    if (count) HIPCHK(hipMemcpyAsync(count, d_c.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}

// the checks both denoise entry points share; resolves the iteration default
static int check_denoise(int device, uint32_t width, uint32_t height, const void* rgba, const void* count, const void* albedo_hits,
                         const void* normal_depth, const void* feature_count, uint32_t* iterations, float sigma_color, float sigma_depth,
                         uint32_t normal_squarings, uint32_t flags, const void* out_rgba) {
  if (!rgba || !count || !out_rgba) return fail(PBRHIP_EINVAL, "denoise: NULL rgba, count or out_rgba");
  if (width == 0 || height == 0) return fail(PBRHIP_EINVAL, "denoise: empty image");
  if ((uint64_t)width * height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "denoise: image too large");
  const int nfeat = (albedo_hits ? 1 : 0) + (normal_depth ? 1 : 0) + (feature_count ? 1 : 0);
  if (nfeat != 0 && nfeat != 3) return fail(PBRHIP_EINVAL, "denoise: albedo_hits, normal_depth and feature_count come together or not at all");
  if (sigma_color != sigma_color || sigma_depth != sigma_depth) return fail(PBRHIP_EINVAL, "denoise: a sigma is NaN");
  if (*iterations > 8) return fail(PBRHIP_EINVAL, "denoise: %u iterations (at most 8)", *iterations);
  if (normal_squarings > 16) return fail(PBRHIP_EINVAL, "denoise: %u normal squarings (at most 16)", normal_squarings);
  if (flags & ~PBRHIP_DENOISE_NO_ALBEDO) return fail(PBRHIP_EINVAL, "denoise: unknown flags 0x%x", flags);
  if (*iterations == 0) *iterations = PBRHIP_DENOISE_ITERATIONS;
  int n = 0;
  if (int rc = pbrhip_device_count(&n)) return rc;
  if (n <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
  if (device < 0 || device >= n) return fail(PBRHIP_EINVAL, "denoise: device %d out of range (%d devices)", device, n);
  return PBRHIP_OK;
}

// prepare + one launch per iteration on the device's null stream; the three temporaries (two colour images, one guide image) live
// for the call
static int denoise_impl(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                        const float* normal_depth, const uint32_t* feature_count, uint32_t iterations, float sigma_color, float sigma_depth,
                        uint32_t normal_squarings, uint32_t flags, float* out_rgba) {
  HIPCHK(hipSetDevice(device));
  const size_t npx = (size_t)width * height;
  DevBuf<float4> e0, e1, guide;
  HIPCHK(e0.reserve(npx));
  HIPCHK(e1.reserve(npx));
  HIPCHK(guide.reserve(npx));
  DenoiseArgs a;
  a.width = width, a.height = height;
  a.rgba = reinterpret_cast<const float4*>(rgba), a.count = count;
  a.albedo_hits = reinterpret_cast<const float4*>(albedo_hits), a.normal_depth = reinterpret_cast<const float4*>(normal_depth), a.feature_count = feature_count;
  a.no_albedo = (flags & PBRHIP_DENOISE_NO_ALBEDO) ? 1u : 0u;
  a.sigma_color = sigma_color, a.sigma_depth = sigma_depth, a.normal_squarings = normal_squarings;
  launch_denoise_prepare(nullptr, a, e0.p, guide.p);
  HIPCHK(hipGetLastError());
  for (uint32_t i = 0; i < iterations; i++) {
    const bool last = i + 1 == iterations;
    float4* const src = (i & 1u) ? e1.p : e0.p;
    float4* const dst = last ? reinterpret_cast<float4*>(out_rgba) : ((i & 1u) ? e0.p : e1.p);
    launch_denoise_iteration(nullptr, a, i, last, src, guide.p, dst);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_denoise_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                     const float* d_albedo_hits, const float* d_normal_depth, const uint32_t* d_feature_count, uint32_t iterations,
                                     float sigma_color, float sigma_depth, uint32_t normal_squarings, uint32_t flags, float* d_out_rgba) {
  return guarded([&]() -> int {
    if (int rc = check_denoise(device, width, height, d_rgba, d_count, d_albedo_hits, d_normal_depth, d_feature_count, &iterations, sigma_color,
                               sigma_depth, normal_squarings, flags, d_out_rgba))
      return rc;
    return denoise_impl(device, width, height, d_rgba, d_count, d_albedo_hits, d_normal_depth, d_feature_count, iterations, sigma_color, sigma_depth,
                        normal_squarings, flags, d_out_rgba);
  });
}

extern "C" int pbrhip_denoise(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                              const float* normal_depth, const uint32_t* feature_count, uint32_t iterations, float sigma_color, float sigma_depth,
                              uint32_t normal_squarings, uint32_t flags, float* out_rgba) {
  return guarded([&]() -> int {
    if (int rc = check_denoise(device, width, height, rgba, count, albedo_hits, normal_depth, feature_count, &iterations, sigma_color, sigma_depth,
                               normal_squarings, flags, out_rgba))
      return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    DevBuf<float> d_rgba, d_a, d_n, d_out;
    DevBuf<uint32_t> d_count, d_fc;
    HIPCHK(d_rgba.reserve(npx * 4));
    HIPCHK(d_count.reserve(npx));
    HIPCHK(d_out.reserve(npx * 4));
    HIPCHK(hipMemcpy(d_rgba.p, rgba, npx * 4 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_count.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (albedo_hits) {
      HIPCHK(d_a.reserve(npx * 4));
      HIPCHK(d_n.reserve(npx * 4));
      HIPCHK(d_fc.reserve(npx));
      HIPCHK(hipMemcpy(d_a.p, albedo_hits, npx * 4 * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_n.p, normal_depth, npx * 4 * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_fc.p, feature_count, npx * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (int rc = denoise_impl(device, width, height, d_rgba.p, d_count.p, d_a.p, d_n.p, d_fc.p, iterations, sigma_color, sigma_depth,
                              normal_squarings, flags, d_out.p))
      return rc;
    HIPCHK(hipMemcpy(out_rgba, d_out.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return PBRHIP_OK;
  });
}

// ------------------------------------------------------------------ test hooks
extern "C" int pbrhip_texture_fetch(pbrhip_scene* s, uint32_t texture_id, const float* uv, size_t n, float* rgb) {
  return guarded([&]() -> int {
    if (!s || ((!uv || !rgb) && n)) return fail(PBRHIP_EINVAL, "texture_fetch: NULL argument");
    if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
    if (texture_id >= s->tex_descs.size()) return fail(PBRHIP_EINVAL, "texture_fetch: texture id %u out of range", texture_id);
    if (n > (1u << 24)) return fail(PBRHIP_EINVAL, "texture_fetch: too many coordinates");
    if (!n) return PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    DevBuf<float> d_uv, d_rgb;
    HIPCHK(d_uv.reserve(2 * n));
    HIPCHK(d_rgb.reserve(3 * n));
    HIPCHK(hipMemcpyAsync(d_uv.p, uv, 2 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    launch_texture_fetch(s->stream, s->dscene, texture_id, d_uv.p, (uint32_t)n, d_rgb.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgb, d_rgb.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}

// the GPU builder on bare boxes, whatever depth it reaches (the fallback at kStackDepth is pbrhip_scene_commit's)
extern "C" int pbrhip_lbvh_build(int device, const float* lo, const float* hi, const uint8_t* kinds, uint32_t n, void* nodes_out,
                                 uint32_t* order_out, uint32_t* depth_out) {
  return guarded([&]() -> int {
    if (n >= (1u << 27)) return fail(PBRHIP_EINVAL, "lbvh_build: too many boxes (%u)", n);
    if (n == 0) return PBRHIP_OK;
    if (!lo || !hi || !kinds || !nodes_out || !order_out || !depth_out) return fail(PBRHIP_EINVAL, "lbvh_build: NULL argument");
    int ndev = 0;
    if (int rc = pbrhip_device_count(&ndev)) return rc;
    if (ndev <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(PBRHIP_EINVAL, "lbvh_build: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    struct Stream {
      hipStream_t s = nullptr;
      ~Stream() {
        if (s) (void)hipStreamDestroy(s);
      }
    } st;
    HIPCHK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const size_t nn = n > 1 ? n - 1 : 1;
    DevBuf<BvhNode> d_nodes;
    HIPCHK(d_nodes.reserve(nn));
    const std::vector<float> vlo(lo, lo + 3 * (size_t)n), vhi(hi, hi + 3 * (size_t)n);
    const std::vector<uint8_t> vkinds(kinds, kinds + n);
    std::vector<uint32_t> order;
    uint32_t depth = 0;
    HIPCHK(build_bvh_gpu(st.s, vlo, vhi, vkinds, d_nodes.p, &order, &depth));
    HIPCHK(hipMemcpyAsync(nodes_out, d_nodes.p, nn * sizeof(BvhNode), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    memcpy(order_out, order.data(), sizeof(uint32_t) * n);
    *depth_out = depth;
    return PBRHIP_OK;
  });
}

// builder PBRHIP_BVH_GPU_LBVH_WIDE on bare boxes and slot records: the binary tree, then its collapse, whatever comes out (no fallback)
extern "C" int pbrhip_qtree_collapse(int device, const float* lo, const float* hi, const uint8_t* kinds, const void* slots, uint32_t n,
                                     void* nodes_out, uint32_t* order_out, void* qnodes_out, void* tri_out, void* pts_out,
                                     uint32_t* hit_out, uint32_t* sizes_out) {
  return guarded([&]() -> int {
    if (n >= (1u << 27)) return fail(PBRHIP_EINVAL, "qtree_collapse: too many boxes (%u)", n);
    if (!sizes_out) return fail(PBRHIP_EINVAL, "qtree_collapse: NULL argument");
    if (n == 0) {
      memset(sizes_out, 0, 6 * sizeof(uint32_t));
      return PBRHIP_OK;
    }
    if (!lo || !hi || !kinds || !slots) return fail(PBRHIP_EINVAL, "qtree_collapse: NULL argument");
    if (qnodes_out && (!nodes_out || !order_out || !tri_out || !pts_out || !hit_out)) return fail(PBRHIP_EINVAL, "qtree_collapse: NULL argument");
    int ndev = 0;
    if (int rc = pbrhip_device_count(&ndev)) return rc;
    if (ndev <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(PBRHIP_EINVAL, "qtree_collapse: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    struct Stream {
      hipStream_t s = nullptr;
      ~Stream() {
        if (s) (void)hipStreamDestroy(s);
      }
    } st;
    HIPCHK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const size_t nn = n > 1 ? n - 1 : 1;
    DevBuf<BvhNode> d_nodes;  // nodes, then the slots in leaf order: the layout of a committed scene
    HIPCHK(d_nodes.reserve(nn + n));
    const std::vector<float> vlo(lo, lo + 3 * (size_t)n), vhi(hi, hi + 3 * (size_t)n);
    const std::vector<uint8_t> vkinds(kinds, kinds + n);
    std::vector<uint32_t> order;
    uint32_t depth = 0;
    HIPCHK(build_bvh_gpu(st.s, vlo, vhi, vkinds, d_nodes.p, &order, &depth));
    std::vector<BvhNode> sl(n);  // (a slot is 64 bytes, like a node)
    for (uint32_t k = 0; k < n; k++) memcpy(&sl[k], static_cast<const char*>(slots) + 64 * (size_t)order[k], 64);
    HIPCHK(hipMemcpyAsync(d_nodes.p + nn, sl.data(), 64 * (size_t)n, hipMemcpyHostToDevice, st.s));
    DevBuf<float4> d_wide;
    DevBuf<uint32_t> d_hit;
    auto alloc = [&](size_t words, size_t hits, float4** w, uint32_t** h) -> hipError_t {
      hipError_t e = d_wide.reserve(words);
      if (e == hipSuccess) e = d_hit.reserve(hits);
      *w = d_wide.p, *h = d_hit.p;
      return e;
    };
    const bool tri_pairs = std::all_of(vkinds.begin(), vkinds.end(), [](uint8_t kd) { return kd == 0; });
    QCollapse qc;
    HIPCHK(collapse_qtree_gpu(st.s, d_nodes.p, n, reinterpret_cast<const float4*>(d_nodes.p + nn), tri_pairs, alloc, &qc));
    sizes_out[0] = qc.nodes, sizes_out[1] = (uint32_t)qc.tri_words, sizes_out[2] = (uint32_t)qc.pts, sizes_out[3] = 0;
    sizes_out[4] = (qc.fits ? 1u : 0u) | (qc.quantised ? 2u : 0u), sizes_out[5] = depth;
    if (!qc.fits || !qnodes_out) return PBRHIP_OK;  // (a call without output arrays reports the sizes)
    std::vector<QNode> qn(qc.nodes);
    HIPCHK(hipMemcpyAsync(nodes_out, d_nodes.p, nn * sizeof(BvhNode), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(qn.data(), d_wide.p, (size_t)qc.nodes * 64, hipMemcpyDeviceToHost, st.s));
    if (qc.tri_words) HIPCHK(hipMemcpyAsync(tri_out, d_wide.p + (size_t)qc.nodes * 4, qc.tri_words * 16, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(pts_out, d_wide.p + (size_t)qc.nodes * 4 + qc.tri_words, qc.pts * 16, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(hit_out, d_hit.p, qc.pts * 4, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    memcpy(qnodes_out, qn.data(), (size_t)qc.nodes * 64);
    memcpy(order_out, order.data(), sizeof(uint32_t) * n);
    sizes_out[3] = qtree_stack_need(qn);
    return PBRHIP_OK;
  });
}

// pbrhip_scene_refit's kernels on bare trees: plan, leaf records, both trees (no scene)
extern "C" int pbrhip_tree_refit(int device, uint32_t n, const void* slots, void* nodes_inout, void* qnodes_inout, uint32_t num_qnodes,
                                 void* tri_inout, uint32_t tri_words, int tri_pairs, void* pts_inout, const uint32_t* hit, uint32_t num_points) {
  return guarded([&]() -> int {
    if (n >= (1u << 27)) return fail(PBRHIP_EINVAL, "tree_refit: too many slots (%u)", n);
    if (n == 0) return PBRHIP_OK;
    if (!slots || !nodes_inout) return fail(PBRHIP_EINVAL, "tree_refit: NULL argument");
    if (qnodes_inout && (num_qnodes == 0 || (tri_words && !tri_inout) || !pts_inout || !hit)) return fail(PBRHIP_EINVAL, "tree_refit: NULL argument");
    if (qnodes_inout && (num_qnodes >= (1u << 27) || num_points >= (1u << 27) || tri_words >= 3u * (1u << 27))) return fail(PBRHIP_EINVAL, "tree_refit: a size is out of range");
    int ndev = 0;
    if (int rc = pbrhip_device_count(&ndev)) return rc;
    if (ndev <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(PBRHIP_EINVAL, "tree_refit: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    struct Stream {
      hipStream_t s = nullptr;
      ~Stream() {
        if (s) (void)hipStreamDestroy(s);
      }
    } st;
    HIPCHK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    const size_t nn = n > 1 ? n - 1 : 1;
    const size_t nq = qnodes_inout ? num_qnodes : 0;
    DevBuf<BvhNode> d_nodes;  // nodes, then the slots in leaf order: the layout of a committed scene
    DevBuf<float4> d_wide;
    DevBuf<uint32_t> d_hit;
    HIPCHK(d_nodes.reserve(nn + n));
    HIPCHK(hipMemcpyAsync(d_nodes.p, nodes_inout, nn * 64, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(d_nodes.p + nn, slots, (size_t)n * 64, hipMemcpyHostToDevice, st.s));
    RefitTree t;
    t.nodes = d_nodes.p, t.nb = (uint32_t)nn, t.ns = n;
    if (nq) {
      HIPCHK(d_wide.reserve(nq * 4 + tri_words + num_points));
      HIPCHK(d_hit.reserve(num_points));
      HIPCHK(hipMemcpyAsync(d_wide.p, qnodes_inout, nq * 64, hipMemcpyHostToDevice, st.s));
      if (tri_words) HIPCHK(hipMemcpyAsync(d_wide.p + nq * 4, tri_inout, (size_t)tri_words * 16, hipMemcpyHostToDevice, st.s));
      if (num_points) HIPCHK(hipMemcpyAsync(d_wide.p + nq * 4 + tri_words, pts_inout, (size_t)num_points * 16, hipMemcpyHostToDevice, st.s));
      if (num_points) HIPCHK(hipMemcpyAsync(d_hit.p, hit, (size_t)num_points * 4, hipMemcpyHostToDevice, st.s));
      t.q = reinterpret_cast<QNode*>(d_wide.p), t.nq = (uint32_t)nq;
      t.tri = d_wide.p + nq * 4, t.tri_words = tri_words, t.tri_pairs = tri_pairs != 0;
      t.pts = d_wide.p + nq * 4 + tri_words, t.hit = d_hit.p, t.npts = num_points;
    }
    RefitPlan plan;
    RefitTimes rt;
    HIPCHK(refit_tree_gpu(st.s, t, false, &plan, &rt));
    if (rt.failed) return fail(PBRHIP_EHIP, "tree_refit: %s", (rt.failed & 1u) ? "a node of the Q tree cannot be quantised" : "the tree holds an index out of range");
    HIPCHK(hipMemcpyAsync(nodes_inout, d_nodes.p, nn * 64, hipMemcpyDeviceToHost, st.s));
    if (nq) {
      HIPCHK(hipMemcpyAsync(qnodes_inout, d_wide.p, nq * 64, hipMemcpyDeviceToHost, st.s));
      if (tri_words) HIPCHK(hipMemcpyAsync(tri_inout, d_wide.p + nq * 4, (size_t)tri_words * 16, hipMemcpyDeviceToHost, st.s));
      if (num_points) HIPCHK(hipMemcpyAsync(pts_inout, d_wide.p + nq * 4 + tri_words, (size_t)num_points * 16, hipMemcpyDeviceToHost, st.s));
    }
    HIPCHK(hipStreamSynchronize(st.s));
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_leaf_eval(uint32_t op, const float* in, size_t n, uint32_t in_words, float* out, uint32_t out_words) {
  return guarded([&]() -> int {
    if ((!in || !out) && n) return fail(PBRHIP_EINVAL, "leaf_eval: NULL argument");
    if (op > 10u || in_words == 0 || out_words == 0 || n > (1u << 24)) return fail(PBRHIP_EINVAL, "leaf_eval: bad operation or sizes");
    static const uint32_t need_in[11] = {4, 3, 2, 2, 2, 2, 2, 9, 8, 29, 30}, need_out[11] = {1, 1, 1, 1, 5, 3, 2, 2, 5, 4, 7};
    if (in_words < need_in[op] || out_words < need_out[op]) return fail(PBRHIP_EINVAL, "leaf_eval: operation %u needs %u words in, %u out", op, need_in[op], need_out[op]);
    if (!n) return PBRHIP_OK;
    DevBuf<float> d_in, d_out;
    HIPCHK(d_in.reserve(n * in_words));
    HIPCHK(d_out.reserve(n * out_words));
    HIPCHK(hipMemcpy(d_in.p, in, n * in_words * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out.p, 0, n * out_words * sizeof(float)));
    launch_leaf_eval(nullptr, op, d_in.p, (uint32_t)n, in_words, d_out.p, out_words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out.p, n * out_words * sizeof(float), hipMemcpyDeviceToHost));
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_camera_rays(pbrhip_scene* s, uint32_t width, uint32_t height, uint64_t seed_seq, const uint32_t* x_y_pass, size_t n,
                                  pbrhip_ray* rays) {
  return guarded([&]() -> int {
  if (!s || (!x_y_pass && n) || (!rays && n)) return fail(PBRHIP_EINVAL, "camera_rays: NULL argument");
  if (width == 0 || height == 0) return fail(PBRHIP_EINVAL, "camera_rays: zero image size");
  if (!s->cam_set && !s->committed) return fail(PBRHIP_ESTATE, "camera_rays: the reference camera needs a committed scene");
  PB_NOT_STALE(s);
  if (n == 0) return PBRHIP_OK;
  if (n >= (1ull << 31)) return fail(PBRHIP_EINVAL, "too many rays");
  for (size_t i = 0; i < n; i++)
    if (x_y_pass[3 * i] >= width || x_y_pass[3 * i + 1] >= height) return fail(PBRHIP_EINVAL, "camera_rays: pixel %zu is outside the image", i);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(s->hook_rays.reserve(2 * n));
  HIPCHK(s->hook_xyp.reserve(3 * n));
  HIPCHK(hipMemcpyAsync(s->hook_xyp.p, x_y_pass, 3 * n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  const UserCamera uc = s->cam_set ? make_user_camera(s, width, height) : UserCamera{};
  const Camera dc = s->cam_set ? Camera{} : make_camera(s, width, height);
  launch_camera_rays(s->stream, uc, dc, s->cam_set, width, height, seed_seq, s->hook_xyp.p, (uint32_t)n, s->hook_rays.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rays, s->hook_rays.p, n * sizeof(pbrhip_ray), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return PBRHIP_OK;
  });
}
// the body of pbrhip_trace_closest (any = false: `out` receives n pbrhip_hit) and pbrhip_trace_any (any: n occlusion bytes)
static int trace_hook(pbrhip_scene* s, const pbrhip_ray* rays, size_t n, void* out, bool any) {
  const char* name = any ? "trace_any" : "trace_closest";
  if (!s || (!rays && n) || (!out && n)) return fail(PBRHIP_EINVAL, "%s: NULL argument", name);
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  if (n == 0) return PBRHIP_OK;
  if (n >= (1ull << 31)) return fail(PBRHIP_EINVAL, "too many rays");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(s->hook_rays.reserve(2 * n));
  if (any) HIPCHK(s->hook_occ.reserve(n));
  else HIPCHK(s->hook_hits.reserve(n));
  HIPCHK(s->counts.reserve(kCntNum * kMaxGroups));
  HIPCHK(hipMemsetAsync(s->counts.p, 0, sizeof(uint32_t) * kCntNum, s->stream));
  HIPCHK(hipMemcpyAsync(s->hook_rays.p, rays, n * sizeof(pbrhip_ray), hipMemcpyHostToDevice, s->stream));
  HIPCHK(s->spill.reserve(kSpillWords));
  launch_hook(s->stream, s->dscene, s->hook_rays.p, (uint32_t)n, any ? nullptr : s->hook_hits.p, any ? s->hook_occ.p : nullptr, s->counts.p, s->spill.p, k);
  HIPCHK(hipGetLastError());
  if (any) HIPCHK(hipMemcpyAsync(out, s->hook_occ.p, n, hipMemcpyDeviceToHost, s->stream));
  else HIPCHK(hipMemcpyAsync(out, s->hook_hits.p, n * sizeof(pbrhip_hit), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(s->h_counts, s->counts.p, sizeof(uint32_t) * kCntNum, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (s->h_counts[kCntOverflow]) return fail(PBRHIP_EOVERFLOW, "BVH traversal stack overflow");
  return PBRHIP_OK;
}
extern "C" int pbrhip_trace_closest(pbrhip_scene* s, const pbrhip_ray* rays, size_t n, pbrhip_hit* hits) {
  return guarded([&]() -> int { return trace_hook(s, rays, n, hits, false); });
}
extern "C" int pbrhip_trace_any(pbrhip_scene* s, const pbrhip_ray* rays, size_t n, uint8_t* occluded) {
  return guarded([&]() -> int { return trace_hook(s, rays, n, occluded, true); });
}
