// pbrlab_hip.hpp -- header-only C++ shim that keeps pbrlab's names AND value types (namespace pbrlab: float3, Attribute,
// TriangleMesh, CubicBezierCurveMesh, Texture, MaterialParameter, AreaLightParameter, MeshPtr, Scene, RenderLayer, Render)
// over the C ABI of libpbrhip (pbrhip.h).  What a pbrlab caller (pc/pbrlab-cli.cc:24-59, pc/pc-common.cc:100-270,
// pc/pbrlab-gui.cc:207-222, pc/glfw-window.cc:866-979) includes instead of scene.h / render.h: the call sequences of
// CreateSceneFromObj / CreateSceneFromCubicBezierCurve and of the GUI's material edit loop compile against it as they are
// (mpark::variant / mpark::get are std::variant / std::get here: the alias below; -DPBRLAB_HIP_NO_MPARK_ALIAS drops it).
//
// Differences a caller can observe: the library COPIES mesh, texture and material data when it is handed over (the
// reference's raytracer shares the mesh buffers, raytracer.h:34), and material edits made through
// Scene::FetchMeshMaterialParameters() reach the GPU at the next Render() call (the GUI applies them between calls too:
// EditQueue::EditAndPopAll, pc/pc-common.cc:57-84).
#ifndef PBRLAB_HIP_HPP_
#define PBRLAB_HIP_HPP_

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <variant>
#include <vector>

#include <dlfcn.h>

#include "pbrhip.h"

#ifndef PBRLAB_HIP_NO_MPARK_ALIAS
namespace mpark {  // pbrlab spells its variants mpark::variant / mpark::get<I> (src/material-param.h:14, src/mesh/mesh.h:9)
using std::get;
using std::get_if;
using std::holds_alternative;
using std::variant;
}  // namespace mpark
#endif

namespace pbrlab {

// src/type.h:8 (nanort::real3<float>): the part of it pbrlab's callers use
struct float3 {
  float3() : v{0.f, 0.f, 0.f} {}
  explicit float3(float s) : v{s, s, s} {}
  float3(float x, float y, float z) : v{x, y, z} {}
  explicit float3(const float* p) : v{p[0], p[1], p[2]} {}
  float x() const { return v[0]; }
  float y() const { return v[1]; }
  float z() const { return v[2]; }
  float operator[](int i) const { return v[i]; }
  float& operator[](int i) { return v[i]; }
  float v[3];
};

// src/mesh/attribute.h:7-18
struct Attribute {
  std::vector<float> vertices;   // 4(xyzw) * num vertices (w = 1.0f)
  std::vector<float> normals;    // 4(xyzw) * num normals or 0
  std::vector<float> texcoords;  // 2(uv) * num texcoords or 0
};
struct CurveAttribute {
  std::vector<float> vertices;  // 4(xyz + thickness) * num vertices
};

// src/mesh/triangle-mesh.h:15-62, triangle-mesh.cc:17-57 (the data side; the fetch functions run on the GPU)
class TriangleMesh {
public:
  TriangleMesh() : num_faces_(0) {}
  TriangleMesh(const std::string name, const std::shared_ptr<Attribute>& attribute, const std::vector<uint32_t> vertex_ids,
               const std::vector<uint32_t> normal_ids, const std::vector<uint32_t> texcoord_ids,
               const std::vector<uint32_t> material_ids)
      : num_faces_(uint32_t(vertex_ids.size() / 3)), vertex_ids_(vertex_ids), normal_ids_(normal_ids), texcoord_ids_(texcoord_ids),
        material_ids_(material_ids), pAttribute_(attribute), name_(name) {}
  const std::vector<uint32_t>& GetMaterials() const { return material_ids_; }
  uint32_t GetNumFaces() const { return num_faces_; }
  uint32_t GetNumVertices() const { return pAttribute_ ? uint32_t(pAttribute_->vertices.size() / 4) : 0u; }
  std::string GetName() const { return name_; }
  const std::vector<uint32_t>& GetVertexIds() const { return vertex_ids_; }
  const std::vector<float>& GetVertices() const { return pAttribute_->vertices; }
  void SetMaterialId(const uint32_t material_id, const uint32_t prim_id) { material_ids_.at(prim_id) = material_id; }
  // (not in the reference: what Scene::AddTriangleMesh hands to the library)
  const std::vector<uint32_t>& GetNormalIds() const { return normal_ids_; }
  const std::vector<uint32_t>& GetTexcoordIds() const { return texcoord_ids_; }
  const std::shared_ptr<Attribute>& GetAttribute() const { return pAttribute_; }

private:
  uint32_t num_faces_;
  std::vector<uint32_t> vertex_ids_, normal_ids_, texcoord_ids_;  // 3 * num_faces_ (normals / texcoords: or 0)
  std::vector<uint32_t> material_ids_;                            // num_faces_ or 0
  std::shared_ptr<Attribute> pAttribute_;
  std::string name_;
};

// src/mesh/cubic-bezier-curve-mesh.h:11-37
class CubicBezierCurveMesh {
public:
  CubicBezierCurveMesh() {}
  CubicBezierCurveMesh(const std::string& name, const std::shared_ptr<CurveAttribute> attribute,
                       const std::vector<uint32_t>& indices, const std::vector<uint32_t>& material_ids)
      : pAttribute_(attribute), indices_(indices), material_ids_(material_ids), name_(name) {}
  const std::vector<uint32_t>& GetIndices() const { return indices_; }
  uint32_t GetNumSegments() const { return uint32_t(indices_.size()); }
  uint32_t GetNumVertices() const { return pAttribute_ ? uint32_t(pAttribute_->vertices.size() / 4) : 0u; }
  const std::vector<uint32_t>& GetMaterials() const { return material_ids_; }
  std::string GetName() const { return name_; }
  const std::vector<float>& GetVertices() const { return pAttribute_->vertices; }
  void SetMaterialId(const uint32_t material_id, const uint32_t segment_id) {
    if (material_ids_.size() != indices_.size()) material_ids_.resize(indices_.size(), uint32_t(-1));
    material_ids_.at(segment_id) = material_id;
  }

private:
  std::shared_ptr<CurveAttribute> pAttribute_;
  std::vector<uint32_t> indices_, material_ids_;
  std::string name_;
};

// src/mesh/mesh.h:21-26
enum MeshType { kTriangleMesh = 0, kCubicBezierCurveMesh, kMeshNone };
using MeshPtr = std::variant<std::shared_ptr<TriangleMesh>, std::shared_ptr<CubicBezierCurveMesh>>;
inline std::string GetName(const MeshPtr& m) {
  return m.index() == kTriangleMesh ? std::get<kTriangleMesh>(m)->GetName() : std::get<kCubicBezierCurveMesh>(m)->GetName();
}
inline uint32_t GetNumPrimitive(const MeshPtr& m) {
  return m.index() == kTriangleMesh ? std::get<kTriangleMesh>(m)->GetNumFaces() : std::get<kCubicBezierCurveMesh>(m)->GetNumSegments();
}

// src/texture.h:11-44 (the data side; texture.cc:43-57 runs on the GPU)
class Texture {
public:
  Texture() : width_(0), height_(0), channels_(0) {}
  Texture(const std::vector<float>& pixels, const uint32_t width, const uint32_t height, const uint32_t channels,
          const std::string& name)
      : width_(width), height_(height), channels_(channels), pixels_(pixels), name_(name) {}
  bool Reset(const std::vector<float>& pixels, const uint32_t width, const uint32_t height, const uint32_t channels) {
    if (pixels.size() != size_t(width) * height * channels) return false;
    pixels_ = pixels, width_ = width, height_ = height, channels_ = channels;
    return true;
  }
  void SetName(const std::string& name) { name_ = name; }
  uint32_t GetWidth() const { return width_; }
  uint32_t GetHeight() const { return height_; }
  uint32_t GetChannels() const { return channels_; }
  std::string GetName() const { return name_; }
  const std::vector<float>& GetPixels() const { return pixels_; }  // (not in the reference)

private:
  uint32_t width_, height_, channels_;
  std::vector<float> pixels_;
  std::string name_;
};

// src/material-param.h:20-103: the same members, defaults and helper functions
enum MaterialParameterType { kCyclesPrincipledBsdfParameter = 0, kHairBsdfParameter };
struct CyclesPrincipledBsdfParameter {
  float3 base_color = {0.8f, 0.8f, 0.8f};
  float subsurface = 0.0f;
  float3 subsurface_radius = {1.0f, 1.0f, 1.0f};
  float3 subsurface_color = {0.7f, 0.1f, 0.1f};
  float metallic = 0.0f, specular = 0.5f, specular_tint = 0.0f, roughness = 0.5f, anisotropic = 0.0f, anisotropic_rotation = 0.0f;
  float sheen = 0.0f, sheen_tint = 0.5f, clearcoat = 0.0f, clearcoat_roughness = 0.03f, ior = 1.45f, transmission = 0.0f;
  float transmission_roughness = 0.0f;
  uint32_t base_color_tex_id = uint32_t(-1), subsurface_color_tex_id = uint32_t(-1);
  std::string name = "";
};
struct HairBsdfParameter {
  enum ColoringHair { kRGB = 0, kMelanin };
  ColoringHair coloring_hair = kMelanin;
  float3 base_color = {0.18f, 0.06f, 0.02f};
  float melanin = 0.5f, melanin_redness = 0.8f, melanin_randomize = 0.f;
  float roughness = 0.2f, azimuthal_roughness = 0.3f;
  float ior = 1.55f;
  float shift = 2.f;
  float3 specular_tint = {1.f, 1.f, 1.f}, second_specular_tint = {1.f, 1.f, 1.f}, transmission_tint = {1.f, 1.f, 1.f};
  std::string name = "";
};
using MaterialParameter = std::variant<CyclesPrincipledBsdfParameter, HairBsdfParameter>;
inline void SetMaterialName(const std::string& name, MaterialParameter* m) {
  if (m->index() == kCyclesPrincipledBsdfParameter) std::get<kCyclesPrincipledBsdfParameter>(*m).name = name;
  else std::get<kHairBsdfParameter>(*m).name = name;
}
inline std::string GetMaterialName(const MaterialParameter& m) {
  return m.index() == kCyclesPrincipledBsdfParameter ? std::get<kCyclesPrincipledBsdfParameter>(m).name : std::get<kHairBsdfParameter>(m).name;
}

// src/light-param.h:18-47
struct AreaLightParameter {
  float3 emission = float3(0.8f);
  std::string name;
};
enum LightType { kAreaLight = 0, kLightNone };
using LightParameter = std::variant<AreaLightParameter>;

// src/render-layer.h:11-26
struct RenderLayer {
  RenderLayer() = default;
  RenderLayer(size_t w, size_t h) { Resize(w, h), Clear(); }
  void Clear() {
    std::lock_guard<std::mutex> lock(mtx);
    std::fill(rgba.begin(), rgba.end(), 0.0f);
    std::fill(count.begin(), count.end(), 0u);
  }
  void Resize(size_t w, size_t h) {
    std::lock_guard<std::mutex> lock(mtx);
    width = w, height = h;
    rgba.resize(w * h * 4);
    count.resize(w * h);
  }
  size_t width = 0, height = 0;
  std::vector<float> rgba;
  std::vector<uint32_t> count;
  mutable std::mutex mtx;
};

namespace detail {
inline pbrhip_principled_param ToAbi(const CyclesPrincipledBsdfParameter& p) {
  pbrhip_principled_param q;
  std::memset(&q, 0, sizeof(q));
  for (int k = 0; k < 3; ++k)
    q.base_color[k] = p.base_color[k], q.subsurface_radius[k] = p.subsurface_radius[k], q.subsurface_color[k] = p.subsurface_color[k];
  q.subsurface = p.subsurface, q.metallic = p.metallic, q.specular = p.specular, q.specular_tint = p.specular_tint;
  q.roughness = p.roughness, q.anisotropic = p.anisotropic, q.anisotropic_rotation = p.anisotropic_rotation;
  q.sheen = p.sheen, q.sheen_tint = p.sheen_tint, q.clearcoat = p.clearcoat, q.clearcoat_roughness = p.clearcoat_roughness;
  q.ior = p.ior, q.transmission = p.transmission, q.transmission_roughness = p.transmission_roughness;
  q.base_color_tex_id = p.base_color_tex_id, q.subsurface_color_tex_id = p.subsurface_color_tex_id;
  return q;
}
inline pbrhip_hair_param ToAbi(const HairBsdfParameter& p) {
  pbrhip_hair_param q;
  std::memset(&q, 0, sizeof(q));
  q.coloring_hair = uint32_t(p.coloring_hair);
  for (int k = 0; k < 3; ++k) {
    q.base_color[k] = p.base_color[k], q.specular_tint[k] = p.specular_tint[k];
    q.second_specular_tint[k] = p.second_specular_tint[k], q.transmission_tint[k] = p.transmission_tint[k];
  }
  q.melanin = p.melanin, q.melanin_redness = p.melanin_redness, q.melanin_randomize = p.melanin_randomize;
  q.roughness = p.roughness, q.azimuthal_roughness = p.azimuthal_roughness, q.ior = p.ior, q.shift = p.shift;
  return q;
}
// what the library was last given for a material (compared byte for byte with the caller's current value before a render)
struct Pushed {
  uint32_t kind = 0;
  pbrhip_principled_param pr;
  pbrhip_hair_param hr;
};
inline Pushed Flatten(const MaterialParameter& m) {
  Pushed f;
  std::memset(&f.pr, 0, sizeof(f.pr)), std::memset(&f.hr, 0, sizeof(f.hr));
  f.kind = uint32_t(m.index());
  if (m.index() == kCyclesPrincipledBsdfParameter) f.pr = ToAbi(std::get<kCyclesPrincipledBsdfParameter>(m));
  else f.hr = ToAbi(std::get<kHairBsdfParameter>(m));
  return f;
}
}  // namespace detail

// src/scene.h:14-111
class Scene {
public:
  Scene() {
    if (pbrhip_abi_version() != PBRHIP_ABI_VERSION)  // (the library writes whole structs of ITS layout)
      throw std::runtime_error("libpbrhip.so was built from another version of pbrhip.h (struct layouts differ): rebuild");
    if (pbrhip_scene_create(&h_) != PBRHIP_OK) throw std::runtime_error(pbrhip_last_error());
  }
  ~Scene() { pbrhip_scene_destroy(h_); }
  Scene(const Scene&) = delete;
  Scene& operator=(const Scene&) = delete;

  // scene.h:19-24: AddTriangleMesh(triangle_mesh) as pc/pc-common.cc:159 calls it, or the constructor arguments of
  // TriangleMesh (name, attribute, vertex_ids, normal_ids, texcoord_ids, material_ids)
  template <class... Args>
  MeshPtr AddTriangleMesh(Args&&... args) {
    triangle_meshes_.emplace_back(std::make_shared<TriangleMesh>(args...));
    const TriangleMesh& m = *triangle_meshes_.back();
    const uint32_t nf = m.GetNumFaces();
    const Attribute empty;
    const Attribute& a = m.GetAttribute() ? *m.GetAttribute() : empty;
    uint32_t id;
    Check(pbrhip_scene_add_triangle_mesh(
        h_, a.vertices.data(), uint32_t(a.vertices.size() / 4), a.normals.data(), uint32_t(a.normals.size() / 4),
        a.texcoords.data(), uint32_t(a.texcoords.size() / 2), m.GetVertexIds().data(),
        m.GetNormalIds().size() == size_t(nf) * 3 ? m.GetNormalIds().data() : nullptr,
        m.GetTexcoordIds().size() == size_t(nf) * 3 ? m.GetTexcoordIds().data() : nullptr,
        m.GetMaterials().size() == size_t(nf) ? m.GetMaterials().data() : nullptr, nf, &id));
    mesh_ids_.emplace_back(triangle_meshes_.back().get(), id);
    return MeshPtr(triangle_meshes_.back());
  }
  // scene.h:26-32
  template <class... Args>
  MeshPtr AddCubicBezierCurveMesh(Args&&... args) {
    cubic_bezier_curve_meshes_.emplace_back(std::make_shared<CubicBezierCurveMesh>(args...));
    const CubicBezierCurveMesh& m = *cubic_bezier_curve_meshes_.back();
    const std::vector<float> none;
    const std::vector<float>& v = m.GetNumVertices() ? m.GetVertices() : none;
    uint32_t id;
    Check(pbrhip_scene_add_curve_mesh(h_, v.data(), uint32_t(v.size() / 4), m.GetIndices().data(),
                                      m.GetMaterials().size() == m.GetIndices().size() ? m.GetMaterials().data() : nullptr,
                                      m.GetNumSegments(), &id));
    mesh_ids_.emplace_back(cubic_bezier_curve_meshes_.back().get(), id);
    return MeshPtr(cubic_bezier_curve_meshes_.back());
  }
  // scene.h:34-37 (LightManager::AddLightParam)
  template <class... Args>
  uint32_t AddLightParam(Args&&... args) {
    const AreaLightParameter p(args...);
    uint32_t id;
    Check(pbrhip_scene_add_area_light(h_, p.emission.v, &id));
    return id;
  }
  // scene.h:39-44: a MaterialParameter, or either of its alternatives
  template <class... Args>
  uint32_t AddMaterialParam(Args&&... args) {
    // the library first: if it refuses the material nothing is appended and the two lists stay in step
    const uint32_t id = uint32_t(material_params_.size());
    MaterialParameter param(args...);
    const detail::Pushed f = detail::Flatten(param);
    uint32_t lib_id = uint32_t(-1);
    if (f.kind == kCyclesPrincipledBsdfParameter) Check(pbrhip_scene_add_principled_material(h_, &f.pr, &lib_id));
    else Check(pbrhip_scene_add_hair_material(h_, &f.hr, &lib_id));
    if (lib_id != id) throw std::runtime_error("pbrlab::Scene::AddMaterialParam: material ids of the library and of the shim differ");
    material_params_.emplace_back(std::move(param));
    pushed_.push_back(f);
    return id;
  }
  // scene.h:46-51: a Texture, or its constructor arguments (pixels, width, height, channels, name)
  template <class... Args>
  uint32_t AddTexture(Args&&... args) {
    const Texture t(args...);
    uint32_t id;
    Check(pbrhip_scene_add_texture(h_, t.GetPixels().data(), t.GetWidth(), t.GetHeight(), t.GetChannels(), &id));
    return id;
  }
  uint32_t AddMeshToLocalScene(const uint32_t local_scene_id, const MeshPtr& mesh_ptr) {
    const void* key = mesh_ptr.index() == kTriangleMesh ? static_cast<const void*>(std::get<kTriangleMesh>(mesh_ptr).get())
                                                        : static_cast<const void*>(std::get<kCubicBezierCurveMesh>(mesh_ptr).get());
    for (const auto& e : mesh_ids_)
      if (e.first == key) {
        uint32_t g;
        Check(pbrhip_scene_add_mesh_to_local_scene(h_, local_scene_id, e.second, &g));
        return g;
      }
    throw std::runtime_error("AddMeshToLocalScene: the mesh was not added to this scene");
  }
  // throws std::runtime_error on a size mismatch like scene.cc:64-94
  void AttachLightParamIdsToInstance(const uint32_t instance_id, const std::vector<std::vector<uint32_t>>& ids) {
    for (size_t g = 0; g < ids.size(); ++g)
      Check(pbrhip_scene_attach_light_ids(h_, instance_id, uint32_t(g), ids[g].data(), uint32_t(ids[g].size())));
  }
  void AttachMaterialParamIdsToInstance(const uint32_t instance_id, const std::vector<std::vector<uint32_t>>& ids) {
    for (size_t g = 0; g < ids.size(); ++g)
      Check(pbrhip_scene_attach_material_ids(h_, instance_id, uint32_t(g), ids[g].data(), uint32_t(ids[g].size())));
  }
  void CommitScene() { Check(pbrhip_scene_commit(h_)); }
  // Geometry edits between renders (pbrhip_scene_update_* / pbrhip_scene_refit; the reference has none): new VALUES for a mesh of this
  // scene, as many as it was added with (normals empty: kept), or a new transform of an instance.  On a committed scene RefitScene()
  // brings the trees up to date on the GPU before the next Render(); until then every call that reads the device scene throws.  The
  // mesh objects this shim keeps for FetchMeshMaterialParameters are not touched: they hold no positions a render reads.
  void UpdateTriangleMesh(const MeshPtr& mesh_ptr, const std::vector<float>& vertices_xyzw, const std::vector<float>& normals_xyzw = {}) {
    Check(pbrhip_scene_update_triangle_mesh(h_, LibraryMeshId(mesh_ptr), vertices_xyzw.data(), uint32_t(vertices_xyzw.size() / 4),
                                            normals_xyzw.empty() ? nullptr : normals_xyzw.data(), uint32_t(normals_xyzw.size() / 4)));
  }
  void UpdateCurveMesh(const MeshPtr& mesh_ptr, const std::vector<float>& vertices_xyzr) {
    Check(pbrhip_scene_update_curve_mesh(h_, LibraryMeshId(mesh_ptr), vertices_xyzr.data(), uint32_t(vertices_xyzr.size() / 4)));
  }
  void UpdateInstanceTransform(const uint32_t instance_id, const float transform[4][4]) {
    Check(pbrhip_scene_update_instance_transform(h_, instance_id, &transform[0][0]));
  }
  // The same edits from device memory of the scene's GPU (pbrhip_scene_update_*_mesh_device): `count` 16-byte elements at each pointer
  // (d_normals_xyzw null: kept), read after the work already enqueued on `stream` (a hipStream_t; null: the null stream).  The library has
  // its own copy when the call returns; from the first such call on a committed scene RefitScene() stages on the GPU as well.
  void UpdateTriangleMeshDevice(const MeshPtr& mesh_ptr, const void* d_vertices_xyzw, uint32_t num_vertices, const void* d_normals_xyzw = nullptr,
                                uint32_t num_normals = 0, void* stream = nullptr) {
    Check(pbrhip_scene_update_triangle_mesh_device(h_, LibraryMeshId(mesh_ptr), d_vertices_xyzw, num_vertices, d_normals_xyzw, num_normals, stream));
  }
  void UpdateCurveMeshDevice(const MeshPtr& mesh_ptr, const void* d_vertices_xyzr, uint32_t num_vertices, void* stream = nullptr) {
    Check(pbrhip_scene_update_curve_mesh_device(h_, LibraryMeshId(mesh_ptr), d_vertices_xyzr, num_vertices, stream));
  }
  void RefitScene() { Check(pbrhip_scene_refit(h_)); }
  // pbrhip_scene_snapshot_pose: keeps the committed scene's slots and camera state as the pose RenderMotion() measures from; before the
  // frame's edits.  A second call replaces the first, CommitScene() drops it.
  void SnapshotPose() { Check(pbrhip_scene_snapshot_pose(h_)); }
  // pbrhip_scene_object_ids: per pixel of RenderMotion()'s ident buffer the primitive, instance or geometry id (PBRHIP_ID_*) of the slot seen
  // there, PBRHIP_NONE for a miss: what SvgfAccumulate() tests the history's identity with, and an object matte
  std::vector<uint32_t> ObjectIds(const std::vector<uint32_t>& ident, const uint32_t what = PBRHIP_ID_INSTANCE) const {
    std::vector<uint32_t> ids(ident.size() / 4);
    Check(pbrhip_scene_object_ids(h_, ident.data(), ids.size(), what, ids.data()));
    return ids;
  }
  // Ray and nearest-point queries (include/pbrhip.h, "ray and nearest-point queries from device memory").  The *Device calls take
  // DEVICE pointers on the scene's GPU: n pbrhip_ray / pbrhip_point, read after the work already enqueued on `stream` (a hipStream_t;
  // null: the null stream); d_ident: 4 words per query (slot, bits of u, v, t or the distance; a miss: PBRHIP_NONE, 0, 0, 0), d_hits:
  // pbrhip_trace_closest's records, d_closest: the closest point | its squared distance; of the two outputs either may be null.  The
  // outputs are written when the call returns.  NearestPoint is the same query on host arrays: ident and closest are resized to 4 n.
  void TraceClosestDevice(const void* d_rays, size_t n, uint32_t* d_ident, pbrhip_hit* d_hits, void* stream = nullptr) const {
    Check(pbrhip_trace_closest_device(h_, d_rays, n, stream, d_ident, d_hits));
  }
  void TraceAnyDevice(const void* d_rays, size_t n, uint8_t* d_occluded, void* stream = nullptr) const {
    Check(pbrhip_trace_any_device(h_, d_rays, n, stream, d_occluded));
  }
  void NearestPoint(const std::vector<pbrhip_point>& points, std::vector<uint32_t>* ident, std::vector<float>* closest) const {
    if (ident) ident->assign(4 * points.size(), 0u);
    if (closest) closest->assign(4 * points.size(), 0.0f);
    Check(pbrhip_nearest_point(h_, points.data(), points.size(), ident ? ident->data() : nullptr, closest ? closest->data() : nullptr));
  }
  void NearestPointDevice(const void* d_points, size_t n, uint32_t* d_ident, float* d_closest, void* stream = nullptr) const {
    Check(pbrhip_nearest_point_device(h_, d_points, n, stream, d_ident, d_closest));
  }
  // All-hits ray queries (include/pbrhip.h, "all-hits ray queries"): per ray the number of accepted hits in (tmin, tmax] -- count, not
  // capped -- and the max_hits <= PBRHIP_ALL_HITS_MAX nearest of them, ordered by (t, canonical primitive id, u), in TraceClosestDevice's
  // identity format -- ident, max_hits entries of 4 words per ray, (PBRHIP_NONE, 0, 0, 0) past the count.  Either output may be null, not
  // both; max_hits == 0 asks for the count alone.  TraceAll takes host arrays (count resized to n, ident to 4 n max_hits), TraceAllDevice
  // DEVICE pointers on the scene's GPU, read after the work already enqueued on `stream`.
  void TraceAll(const std::vector<pbrhip_ray>& rays, uint32_t max_hits, std::vector<uint32_t>* count, std::vector<uint32_t>* ident) const {
    if (count) count->assign(rays.size(), 0u);
    if (ident) ident->assign(4 * rays.size() * max_hits, 0u);
    Check(pbrhip_trace_all(h_, rays.data(), rays.size(), max_hits, count ? count->data() : nullptr, ident ? ident->data() : nullptr));
  }
  void TraceAllDevice(const void* d_rays, size_t n, uint32_t max_hits, uint32_t* d_count, uint32_t* d_ident, void* stream = nullptr) const {
    Check(pbrhip_trace_all_device(h_, d_rays, n, max_hits, stream, d_count, d_ident));
  }
  // K-nearest queries (include/pbrhip.h, "k-nearest queries"): per query point the number of primitives within max_dist -- count, not
  // capped -- and the max_k <= PBRHIP_K_NEAREST_MAX nearest of them, ordered by (D2, canonical primitive id, piece index), in
  // NearestPoint's formats -- ident and closest, max_k entries of 4 words per query, (PBRHIP_NONE, 0, 0, 0) and zeros past the count.
  // Any output may be null, but closest needs ident and max_k == 0 needs count.  KNearest takes host arrays (count resized to n, ident
  // and closest to 4 n max_k), KNearestDevice DEVICE pointers on the scene's GPU, read after the work already enqueued on `stream`.
  void KNearest(const std::vector<pbrhip_point>& points, uint32_t max_k, std::vector<uint32_t>* count, std::vector<uint32_t>* ident,
                std::vector<float>* closest) const {
    if (count) count->assign(points.size(), 0u);
    if (ident) ident->assign(4 * points.size() * max_k, 0u);
    if (closest) closest->assign(4 * points.size() * max_k, 0.0f);
    Check(pbrhip_k_nearest(h_, points.data(), points.size(), max_k, count ? count->data() : nullptr, ident ? ident->data() : nullptr,
                           closest ? closest->data() : nullptr));
  }
  void KNearestDevice(const void* d_points, size_t n, uint32_t max_k, uint32_t* d_count, uint32_t* d_ident, float* d_closest, void* stream = nullptr) const {
    Check(pbrhip_k_nearest_device(h_, d_points, n, max_k, stream, d_count, d_ident, d_closest));
  }
  // Signed distance (include/pbrhip.h, "signed distance"): the nearest-point queries with a sign.  sd: 4 floats per query, the winning
  // feature's pseudonormal and the signed distance (outside positive); any of the three outputs may be null.  The grid variant asks at
  // origin + (i, j, k) * spacing and writes dims[2] x dims[1] x dims[0] floats, the signed distance alone.  SignedDistanceInfo builds
  // the pseudonormal table if it has to and reports the scene's topology.
  void SignedDistance(const std::vector<pbrhip_point>& points, std::vector<uint32_t>* ident, std::vector<float>* closest, std::vector<float>* sd) const {
    if (ident) ident->assign(4 * points.size(), 0u);
    if (closest) closest->assign(4 * points.size(), 0.0f);
    if (sd) sd->assign(4 * points.size(), 0.0f);
    Check(pbrhip_signed_distance(h_, points.data(), points.size(), ident ? ident->data() : nullptr, closest ? closest->data() : nullptr,
                                 sd ? sd->data() : nullptr));
  }
  void SignedDistanceDevice(const void* d_points, size_t n, uint32_t* d_ident, float* d_closest, float* d_sd, void* stream = nullptr) const {
    Check(pbrhip_signed_distance_device(h_, d_points, n, stream, d_ident, d_closest, d_sd));
  }
  void SignedDistanceGridDevice(const float origin[3], const float spacing[3], const uint32_t dims[3], float max_dist, float* d_sd,
                                void* stream = nullptr) const {
    Check(pbrhip_signed_distance_grid_device(h_, origin, spacing, dims, max_dist, stream, d_sd));
  }
  pbrhip_sd_info SignedDistanceInfo() const {
    pbrhip_sd_info info;
    Check(pbrhip_scene_signed_distance_info(h_, &info));
    return info;
  }
  // which builder CommitScene uses (pbrhip_scene_set_bvh_builder; the reference has Embree's only); before CommitScene
  enum BvhBuilder { kBvhHostSah = PBRHIP_BVH_HOST_SAH, kBvhGpuLbvh = PBRHIP_BVH_GPU_LBVH, kBvhGpuLbvhWide = PBRHIP_BVH_GPU_LBVH_WIDE };
  void SetBvhBuilder(BvhBuilder b) { Check(pbrhip_scene_set_bvh_builder(h_, static_cast<int>(b))); }
  uint32_t CreateInstance(const uint32_t local_scene_id, const float transform[4][4]) {
    uint32_t id;
    Check(pbrhip_scene_create_instance(h_, local_scene_id, &transform[0][0], &id));
    return id;
  }
  uint32_t CreateLocalScene() {
    uint32_t id;
    Check(pbrhip_scene_create_local_scene(h_, &id));
    return id;
  }
  // scene.cc:251-259 (the header there names the arguments (bmax, bmin); every caller passes (bmin, bmax))
  void FetchSceneAABB(float* bmin, float* bmax) const { Check(pbrhip_scene_aabb(h_, bmin, bmax)); }
  // A lat-long environment light (pbrhip_scene_set_environment): rgb = width x height x 3 floats, row 0 = the top; world_to_env a
  // row-major rotation or null.  rgb == nullptr removes it.  Takes effect at the next Render().
  void SetEnvironment(const float* rgb, uint32_t width, uint32_t height, float scale = 1.0f, const float* world_to_env = nullptr) {
    Check(pbrhip_scene_set_environment(h_, rgb, width, height, scale, world_to_env));
  }
  // A look-at camera (pbrhip_scene_set_camera): vfov in degrees; lens_radius > 0 = a thin lens focused at focus_distance along the view
  // direction (0: |lookat - eye|).  ResetCamera() restores the reference's camera.  Takes effect at the next Render().
  void SetCamera(const float eye[3], const float lookat[3], const float up[3], float vfov_degrees = 30.0f, float lens_radius = 0.0f,
                 float focus_distance = 0.0f) {
    Check(pbrhip_scene_set_camera(h_, eye, lookat, up, vfov_degrees, lens_radius, focus_distance));
  }
  void ResetCamera() { Check(pbrhip_scene_set_camera(h_, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0.0f)); }

  // scene.h:81, scene.cc:206-208: the scene's material table; the GUI edits its elements between renders
  // (pc/glfw-window.cc:866-979 through EditQueue, pc/pc-common.cc:57-84).  An edit reaches the GPU at the next Render():
  // PushMaterialEdits() compares every element with what the library was last given and calls
  // pbrhip_scene_update_*_material for those that differ (a material cannot change its kind).
  std::vector<MaterialParameter>* FetchMeshMaterialParameters() { return &material_params_; }
  void PushMaterialEdits() const {
    if (material_params_.size() != pushed_.size()) throw std::runtime_error("materials are added with AddMaterialParam");
    for (size_t i = 0; i < material_params_.size(); ++i) {
      const detail::Pushed f = detail::Flatten(material_params_[i]);
      if (f.kind == pushed_[i].kind && std::memcmp(&f.pr, &pushed_[i].pr, sizeof(f.pr)) == 0 && std::memcmp(&f.hr, &pushed_[i].hr, sizeof(f.hr)) == 0)
        continue;
      if (f.kind == kCyclesPrincipledBsdfParameter) Check(pbrhip_scene_update_principled_material(h_, uint32_t(i), &f.pr));
      else Check(pbrhip_scene_update_hair_material(h_, uint32_t(i), &f.hr));
      pushed_[i] = f;
    }
  }

  pbrhip_scene* handle() const { return h_; }

  // A copy of this committed scene on another GPU (device memory is copied device-to-device: no second ingestion or
  // BVH build); for the multi-GPU Render() overload below.  Material edits made afterwards go to the scene they are made on.
  std::unique_ptr<Scene> Replicate(int device) const {
    PushMaterialEdits();
    pbrhip_scene* h = nullptr;
    Check(pbrhip_scene_replicate(h_, device, &h));
    std::unique_ptr<Scene> r(new Scene(h));
    r->material_params_ = material_params_, r->pushed_ = pushed_;
    return r;
  }

private:
  explicit Scene(pbrhip_scene* h) : h_(h) {}
  static void Check(int rc) {
    if (rc != PBRHIP_OK) throw std::runtime_error(pbrhip_last_error());
  }
  uint32_t LibraryMeshId(const MeshPtr& mesh_ptr) const {
    const void* key = mesh_ptr.index() == kTriangleMesh ? static_cast<const void*>(std::get<kTriangleMesh>(mesh_ptr).get())
                                                        : static_cast<const void*>(std::get<kCubicBezierCurveMesh>(mesh_ptr).get());
    for (const auto& e : mesh_ids_)
      if (e.first == key) return e.second;
    throw std::runtime_error("the mesh was not added to this scene");
  }
  pbrhip_scene* h_ = nullptr;
  std::vector<std::shared_ptr<TriangleMesh>> triangle_meshes_;                 // scene.h:98
  std::vector<std::shared_ptr<CubicBezierCurveMesh>> cubic_bezier_curve_meshes_;  // scene.h:100
  std::vector<std::pair<const void*, uint32_t>> mesh_ids_;                      // mesh object -> the library's mesh id
  std::vector<MaterialParameter> material_params_;                              // scene.h:102
  mutable std::vector<detail::Pushed> pushed_;
};

namespace detail {
static_assert(sizeof(std::atomic_bool) == 1 && sizeof(std::atomic_size_t) == sizeof(size_t),
              "the library reads std::atomic_bool as a byte and stores std::atomic_size_t as a size_t");
// While the library renders, a watcher prints "finish pass N" as *finish_pass advances (render.cc:229 prints from the
// worker that completes a pass).
struct ProgressPrinter {
  explicit ProgressPrinter(const std::atomic_size_t* fin) : fin_(fin) {
    if (fin_) th_ = std::thread([this]() {
      size_t shown = 0;
      for (;;) {
        const bool last = stop_.load();
        for (const size_t now = fin_->load(); shown < now;) printf("finish pass %lu\n", (unsigned long)++shown);
        if (last) return;
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
      }
    });
  }
  ~ProgressPrinter() {
    stop_.store(true);
    if (th_.joinable()) th_.join();
  }
  const std::atomic_size_t* fin_;
  std::atomic_bool stop_{false};
  std::thread th_;
};
}  // namespace detail

// src/render.h:14-17.  Blocking; clears and resizes *layer.  cancel_render_flag is read live by the library (at every
// host round trip of its render loop; the reference polls it before every tile job, render.cc:217): setting it from
// another thread ends the call early with the completed passes in *layer.  *finish_pass advances while the call runs
// (render.cc:224-231).  Returns true like the reference (render.cc:240); a library error is reported on std::cerr and
// returns false.
inline bool Render(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t num_sample,
                   const std::atomic_bool& cancel_render_flag, RenderLayer* layer, std::atomic_size_t* finish_pass) {
  layer->Resize(width, height);  // PrepareRendering, render.cc:99-100 (the library clears)
  try {
    scene.PushMaterialEdits();  // edits made through FetchMeshMaterialParameters() since the last call
  } catch (const std::exception& e) {
    std::cerr << "pbrlab::Render: " << e.what() << std::endl;
    return false;
  }
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = num_sample;
  d.seed_seq = 1234567890;  // render.cc:215
  d.tile_world = 1;
  std::atomic_size_t local_fin(0);
  std::atomic_size_t* fin = finish_pass ? finish_pass : &local_fin;
  int rc;
  fin->store(0);  // render.cc:209: zero before any worker starts (a counter reused from the previous frame must not be reported)
  {
    detail::ProgressPrinter progress(fin);
    rc = pbrhip_render(scene.handle(), &d, reinterpret_cast<const volatile unsigned char*>(&cancel_render_flag),
                       layer->rgba.data(), layer->count.data(), reinterpret_cast<size_t*>(fin), nullptr);
  }
  if (rc != PBRHIP_OK) {
    std::cerr << "pbrlab::Render: " << pbrhip_last_error() << std::endl;
    return false;
  }
  return true;
}

// The same frame over several GPUs of this process: `scenes` = the committed scene and its replicas
// (Scene::Replicate), one per device.  Pixel blocks are dealt to the devices, the shards are gathered device-to-device
// over xGMI inside the library (pbrhip_render_multi); the image is bit-identical to the one-GPU frame.
inline bool Render(const std::vector<const Scene*>& scenes, const uint32_t width, const uint32_t height,
                   const uint32_t num_sample, const std::atomic_bool& cancel_render_flag, RenderLayer* layer,
                   std::atomic_size_t* finish_pass) {
  layer->Resize(width, height);
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = num_sample;
  d.seed_seq = 1234567890;
  d.tile_world = 1;
  std::vector<pbrhip_scene*> hs;
  try {
    for (const Scene* s : scenes) s->PushMaterialEdits(), hs.push_back(s->handle());
  } catch (const std::exception& e) {
    std::cerr << "pbrlab::Render: " << e.what() << std::endl;
    return false;
  }
  std::atomic_size_t local_fin(0);
  std::atomic_size_t* fin = finish_pass ? finish_pass : &local_fin;
  int rc;
  fin->store(0);  // render.cc:209: zero before any worker starts (a counter reused from the previous frame must not be reported)
  {
    detail::ProgressPrinter progress(fin);
    rc = pbrhip_render_multi(hs.data(), uint32_t(hs.size()), &d,
                             reinterpret_cast<const volatile unsigned char*>(&cancel_render_flag), layer->rgba.data(),
                             layer->count.data(), reinterpret_cast<size_t*>(fin), nullptr);
  }
  if (rc != PBRHIP_OK) {
    std::cerr << "pbrlab::Render: " << pbrhip_last_error() << std::endl;
    return false;
  }
  return true;
}

// ---- first-hit feature buffers and the denoiser (not in the reference) ----
// albedo: sum of albedo rgb | hits; normal_depth: sum of the viewer-facing shading normal | sum of the hit distance; count: samples
struct FeatureLayer {
  FeatureLayer() = default;
  FeatureLayer(size_t w, size_t h) { Resize(w, h), Clear(); }
  void Clear() {
    std::fill(albedo.begin(), albedo.end(), 0.0f);
    std::fill(normal_depth.begin(), normal_depth.end(), 0.0f);
    std::fill(count.begin(), count.end(), 0u);
  }
  void Resize(size_t w, size_t h) {
    width = w, height = h;
    albedo.resize(w * h * 4);
    normal_depth.resize(w * h * 4);
    count.resize(w * h);
  }
  size_t width = 0, height = 0;
  std::vector<float> albedo, normal_depth;
  std::vector<uint32_t> count;
};

// pbrhip_render_features: the features of passes [first_pass, first_pass + num_sample) of the frame Render() makes of this scene.
// Resizes *features unless no_clear, which accumulates on top of it.  Throws with pbrhip_last_error() on a library error.
inline void RenderFeatures(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t num_sample, FeatureLayer* features,
                           const uint32_t first_pass = 0, const bool no_clear = false) {
  if (!no_clear || features->width != width || features->height != height) features->Resize(width, height);
  scene.PushMaterialEdits();
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = num_sample, d.first_pass = first_pass;
  d.seed_seq = 1234567890;  // Render()'s
  d.tile_world = 1;
  d.flags = no_clear ? PBRHIP_RENDER_NO_CLEAR : 0u;
  if (pbrhip_render_features(scene.handle(), &d, features->albedo.data(), features->normal_depth.data(), features->count.data()) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderFeatures: ") + pbrhip_last_error());
}

struct DenoiseOptions {
  uint32_t iterations = 0;  // 0: PBRHIP_DENOISE_ITERATIONS
  float sigma_color = PBRHIP_DENOISE_SIGMA_COLOR, sigma_depth = PBRHIP_DENOISE_SIGMA_DEPTH;  // <= 0: that weight off
  uint32_t normal_squarings = PBRHIP_DENOISE_NORMAL_SQUARINGS;
  bool albedo = true;  // false: PBRHIP_DENOISE_NO_ALBEDO
  int device = 0;
};
// pbrhip_denoise: the edge-avoiding A-trous filter of `layer` guided by `features` (nullptr: by colour alone) -> width x height x 4
// floats, the denoised mean colour | 1.  Throws with pbrhip_last_error() on a library error.
inline std::vector<float> Denoise(const RenderLayer& layer, const FeatureLayer* features, const DenoiseOptions& o = DenoiseOptions()) {
  if (features && (features->width != layer.width || features->height != layer.height))
    throw std::runtime_error("pbrlab::Denoise: features and layer differ in size");
  std::vector<float> out(layer.width * layer.height * 4);
  const int rc = pbrhip_denoise(o.device, uint32_t(layer.width), uint32_t(layer.height), layer.rgba.data(), layer.count.data(),
                                features ? features->albedo.data() : nullptr, features ? features->normal_depth.data() : nullptr,
                                features ? features->count.data() : nullptr, o.iterations, o.sigma_color, o.sigma_depth, o.normal_squarings,
                                o.albedo ? 0u : PBRHIP_DENOISE_NO_ALBEDO, out.data());
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::Denoise: ") + pbrhip_last_error());
  return out;
}

// ---- motion vectors and temporal accumulation (not in the reference) ----
// motion: mx, my, z_prev, valid (0 none, 1 triangle, 2 curve); guide: viewer-facing shading normal | t; ident: slot (PBRHIP_NONE: a miss),
// the bits of u, v, t -- width x height x 4 each
struct MotionLayer {
  size_t width = 0, height = 0;
  std::vector<float> motion, guide;
  std::vector<uint32_t> ident;
};
// pbrhip_render_motion: where the point the current camera's centre ray sees in each pixel was at scene.SnapshotPose().  Throws with
// pbrhip_last_error() on a library error (no snapshot among them).
inline void RenderMotion(const Scene& scene, const uint32_t width, const uint32_t height, MotionLayer* out) {
  out->width = width, out->height = height;
  out->motion.assign(size_t(width) * height * 4, 0.0f), out->guide.assign(size_t(width) * height * 4, 0.0f), out->ident.assign(size_t(width) * height * 4, 0u);
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = 1, d.tile_world = 1;
  if (pbrhip_render_motion(scene.handle(), &d, out->motion.data(), out->guide.data(), out->ident.data()) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderMotion: ") + pbrhip_last_error());
}
// the accumulated mean | history length, and the guide of the frame it was made for: what TemporalAccumulate returns and takes back
struct TemporalHistory {
  size_t width = 0, height = 0;
  std::vector<float> rgba, guide;
  // the RenderLayer Denoise() takes for the accumulated frame: mean | 1, count 1 (0 where the history holds nothing)
  void Layer(RenderLayer* l) const {
    l->Resize(width, height);
    for (size_t i = 0; i < width * height; ++i) {
      const bool any = rgba[4 * i + 3] > 0.0f;
      l->count[i] = any ? 1u : 0u;
      for (int c = 0; c < 3; ++c) l->rgba[4 * i + c] = rgba[4 * i + c];
      l->rgba[4 * i + 3] = any ? 1.0f : 0.0f;
    }
  }
};
struct TemporalOptions {
  float alpha_min = PBRHIP_TEMPORAL_ALPHA_MIN, sigma_depth = PBRHIP_TEMPORAL_SIGMA_DEPTH, normal_cos_min = PBRHIP_TEMPORAL_NORMAL_COS_MIN;
  uint32_t max_history = PBRHIP_TEMPORAL_MAX_HISTORY;
  int device = 0;
};
// pbrhip_temporal_accumulate: the current frame's layer blended into `history` (nullptr: none) where `motion` says it shows the same
// surface -> the new history.  Throws with pbrhip_last_error() on a library error.
inline TemporalHistory TemporalAccumulate(const RenderLayer& layer, const MotionLayer& motion, const TemporalHistory* history,
                                          const TemporalOptions& o = TemporalOptions()) {
  if (motion.width != layer.width || motion.height != layer.height || (history && (history->width != layer.width || history->height != layer.height)))
    throw std::runtime_error("pbrlab::TemporalAccumulate: layer, motion and history differ in size");
  TemporalHistory out;
  out.width = layer.width, out.height = layer.height;
  out.rgba.resize(layer.width * layer.height * 4);
  out.guide = motion.guide;
  const int rc = pbrhip_temporal_accumulate(o.device, uint32_t(layer.width), uint32_t(layer.height), layer.rgba.data(), layer.count.data(),
                                            motion.motion.data(), motion.guide.data(), history ? history->rgba.data() : nullptr,
                                            history ? history->guide.data() : nullptr, o.alpha_min, o.sigma_depth, o.normal_cos_min,
                                            o.max_history, out.rgba.data());
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::TemporalAccumulate: ") + pbrhip_last_error());
  return out;
}

// ---- variance-guided filtering and identity-tested history (not in the reference) ----
// the accumulated albedo-free illumination | history length, the variance of its luminance, and the guide and object ids (empty: none) of
// the frame it was made for: what SvgfAccumulate returns and takes back, and what SvgfFilter filters
struct SvgfHistory {
  size_t width = 0, height = 0;
  std::vector<float> illum, var, guide;
  std::vector<uint32_t> ids;
};
struct SvgfAccumulateOptions {
  float alpha_min = PBRHIP_SVGF_ALPHA_MIN, sigma_depth = PBRHIP_TEMPORAL_SIGMA_DEPTH, normal_cos_min = PBRHIP_TEMPORAL_NORMAL_COS_MIN;
  uint32_t max_history = PBRHIP_TEMPORAL_MAX_HISTORY;
  int device = 0;
};
// pbrhip_svgf_accumulate: TemporalAccumulate on colour / albedo (`features`; nullptr: albedo 1) that also rejects history of another
// object (`ids`: scene.ObjectIds() of the frame; nullptr: no such test, as with a history made without ids) and carries the variance
// of the luminance -> the new history.  Throws with pbrhip_last_error() on a library error.
inline SvgfHistory SvgfAccumulate(const RenderLayer& layer, const MotionLayer& motion, const SvgfHistory* history, const FeatureLayer* features,
                                  const std::vector<uint32_t>* ids, const SvgfAccumulateOptions& o = SvgfAccumulateOptions()) {
  const size_t npx = layer.width * layer.height;
  if (motion.width != layer.width || motion.height != layer.height || (history && (history->width != layer.width || history->height != layer.height)) ||
      (features && (features->width != layer.width || features->height != layer.height)) || (ids && ids->size() != npx))
    throw std::runtime_error("pbrlab::SvgfAccumulate: layer, motion, history, features and ids differ in size");
  const bool with_ids = ids && (!history || !history->ids.empty());
  SvgfHistory out;
  out.width = layer.width, out.height = layer.height;
  out.illum.resize(npx * 4), out.var.resize(npx);
  out.guide = motion.guide;
  if (ids) out.ids = *ids;
  const int rc = pbrhip_svgf_accumulate(o.device, uint32_t(layer.width), uint32_t(layer.height), layer.rgba.data(), layer.count.data(),
                                        features ? features->albedo.data() : nullptr, features ? features->count.data() : nullptr,
                                        motion.motion.data(), motion.guide.data(), with_ids ? ids->data() : nullptr,
                                        history ? history->illum.data() : nullptr, history ? history->var.data() : nullptr,
                                        history ? history->guide.data() : nullptr, with_ids && history ? history->ids.data() : nullptr, o.alpha_min,
                                        o.sigma_depth, o.normal_cos_min, o.max_history, out.illum.data(), out.var.data());
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::SvgfAccumulate: ") + pbrhip_last_error());
  return out;
}
struct SvgfFilterOptions {
  uint32_t iterations = 0;  // 0: PBRHIP_SVGF_ITERATIONS
  float sigma_lum = PBRHIP_SVGF_SIGMA_LUM, sigma_depth = PBRHIP_DENOISE_SIGMA_DEPTH;  // <= 0: that weight off
  uint32_t normal_squarings = PBRHIP_DENOISE_NORMAL_SQUARINGS;
  int device = 0;
};
// pbrhip_svgf_filter: the variance-guided A-trous filter of `history`, the albedo of `features` multiplied back -> width x height x 4
// floats, colour | 1.  feedback (may be nullptr) receives the history whose illumination is the one after the first iteration: hand it
// to the next SvgfAccumulate() in the place of `history`.  Throws with pbrhip_last_error() on a library error.
inline std::vector<float> SvgfFilter(const SvgfHistory& history, const FeatureLayer* features, SvgfHistory* feedback = nullptr,
                                     const SvgfFilterOptions& o = SvgfFilterOptions()) {
  if (features && (features->width != history.width || features->height != history.height))
    throw std::runtime_error("pbrlab::SvgfFilter: features and history differ in size");
  std::vector<float> out(history.width * history.height * 4), fb(feedback ? out.size() : 0);
  const int rc = pbrhip_svgf_filter(o.device, uint32_t(history.width), uint32_t(history.height), history.illum.data(), history.var.data(),
                                    history.guide.data(), history.ids.empty() ? nullptr : history.ids.data(),
                                    features ? features->albedo.data() : nullptr, features ? features->count.data() : nullptr, o.iterations,
                                    o.sigma_lum, o.sigma_depth, o.normal_squarings, out.data(), feedback ? fb.data() : nullptr);
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::SvgfFilter: ") + pbrhip_last_error());
  if (feedback) {
    if (feedback != &history) *feedback = history;
    feedback->illum = fb;
  }
  return out;
}

// ---- the first-hit emission layer (not in the reference) ----
// emission: sum of what the renderer adds to a sample's radiance at depth 0 (an area light seen from its front, the environment behind a
// miss) | the number of samples that added one -- width x height x 4
struct EmissionLayer {
  EmissionLayer() = default;
  EmissionLayer(size_t w, size_t h) { Resize(w, h), Clear(); }
  void Clear() { std::fill(emission.begin(), emission.end(), 0.0f); }
  void Resize(size_t w, size_t h) {
    width = w, height = h;
    emission.resize(w * h * 4);
  }
  size_t width = 0, height = 0;
  std::vector<float> emission;
};
// pbrhip_render_features_emission: RenderFeatures() -- the same buffers, bit for bit -- and the emission layer of the same samples, in one
// trace.  Resizes both unless no_clear, which accumulates on top of them.  Throws with pbrhip_last_error() on a library error.
inline void RenderFeaturesEmission(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t num_sample,
                                   FeatureLayer* features, EmissionLayer* emission, const uint32_t first_pass = 0, const bool no_clear = false) {
  if (!no_clear || features->width != width || features->height != height) features->Resize(width, height);
  if (!no_clear || emission->width != width || emission->height != height) emission->Resize(width, height);
  scene.PushMaterialEdits();
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = num_sample, d.first_pass = first_pass;
  d.seed_seq = 1234567890;  // Render()'s
  d.tile_world = 1;
  d.flags = no_clear ? PBRHIP_RENDER_NO_CLEAR : 0u;
  if (pbrhip_render_features_emission(scene.handle(), &d, features->albedo.data(), features->normal_depth.data(), features->count.data(),
                                      emission->emission.data()) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderFeaturesEmission: ") + pbrhip_last_error());
}
// pbrhip_emission_split: *out_layer = `layer` without the directly seen emission, *out_features (with `features`; both or neither) =
// `features` with a miss counted as black albedo: what SvgfAccumulate(), SvgfFilter() and Denoise() take in the place of the originals.
// out_layer may be &layer, out_features may be features.  Throws with pbrhip_last_error() on a library error.
inline void SplitEmission(const RenderLayer& layer, const EmissionLayer& emission, const FeatureLayer* features, RenderLayer* out_layer,
                          FeatureLayer* out_features = nullptr, const int device = 0) {
  if (emission.width != layer.width || emission.height != layer.height || (features && (features->width != layer.width || features->height != layer.height)))
    throw std::runtime_error("pbrlab::SplitEmission: layer, emission and features differ in size");
  if ((features != nullptr) != (out_features != nullptr)) throw std::runtime_error("pbrlab::SplitEmission: features and out_features come together");
  if (out_layer != &layer) {
    out_layer->Resize(layer.width, layer.height);
    out_layer->count = layer.count;
  }
  if (features && out_features != features) {
    out_features->Resize(features->width, features->height);
    out_features->normal_depth = features->normal_depth;
    out_features->count = features->count;
  }
  const int rc = pbrhip_emission_split(device, uint32_t(layer.width), uint32_t(layer.height), layer.rgba.data(), layer.count.data(),
                                       emission.emission.data(), features ? features->albedo.data() : nullptr,
                                       features ? features->count.data() : nullptr, out_layer->rgba.data(),
                                       features ? out_features->albedo.data() : nullptr);
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::SplitEmission: ") + pbrhip_last_error());
}
// pbrhip_emission_merge: a filtered image of the split layer + the mean of the emission layer over `count` samples (the RenderLayer's)
// -> width x height x 4 floats.  Throws with pbrhip_last_error() on a library error.
inline std::vector<float> MergeEmission(const std::vector<float>& rgba, const EmissionLayer& emission, const std::vector<uint32_t>& count,
                                        const int device = 0) {
  if (rgba.size() != emission.emission.size() || count.size() * 4 != rgba.size())
    throw std::runtime_error("pbrlab::MergeEmission: rgba, emission and count differ in size");
  std::vector<float> out(rgba.size());
  const int rc = pbrhip_emission_merge(device, uint32_t(emission.width), uint32_t(emission.height), rgba.data(), emission.emission.data(),
                                       count.data(), out.data());
  if (rc != PBRHIP_OK) throw std::runtime_error(std::string("pbrlab::MergeEmission: ") + pbrhip_last_error());
  return out;
}

// ---- adaptive sampling (not in the reference) ----
struct AdaptiveOptions {
  float threshold = PBRHIP_ADAPTIVE_THRESHOLD;  // a tile stops when its error estimate E <= threshold
  uint32_t first_level = 0;                     // 0: PBRHIP_ADAPTIVE_FIRST_LEVEL
};
struct AdaptiveResult {
  std::vector<float> tile_error;  // ceil(width / 8) * ceil(height / 8): every tile's last E
  uint64_t samples = 0;           // the sum of layer->count
  uint32_t rounds = 0;
};
// pbrhip_render_adaptive: Render() with a sample count per 8x8 tile, at most max_sample.  Pixel p of *layer holds, bit for bit, what
// Render() with num_sample = layer->count[p] holds at p.  Clears and resizes *layer; cancel_render_flag and finish_pass as for Render()
// (*finish_pass: the level every pixel holds).  Throws with pbrhip_last_error() on a library error.
inline AdaptiveResult RenderAdaptive(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t max_sample,
                                     const std::atomic_bool& cancel_render_flag, RenderLayer* layer, std::atomic_size_t* finish_pass = nullptr,
                                     const AdaptiveOptions& o = AdaptiveOptions()) {
  layer->Resize(width, height);
  scene.PushMaterialEdits();
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = max_sample;
  d.seed_seq = 1234567890;  // Render()'s
  d.tile_world = 1;
  AdaptiveResult r;
  r.tile_error.resize(size_t((width + 7) / 8) * ((height + 7) / 8));
  std::atomic_size_t local_fin(0);
  std::atomic_size_t* fin = finish_pass ? finish_pass : &local_fin;
  fin->store(0);
  if (pbrhip_render_adaptive(scene.handle(), &d, o.threshold, o.first_level, reinterpret_cast<const volatile unsigned char*>(&cancel_render_flag),
                             layer->rgba.data(), layer->count.data(), r.tile_error.data(), reinterpret_cast<size_t*>(fin), &r.samples,
                             &r.rounds) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderAdaptive: ") + pbrhip_last_error());
  return r;
}

// ---- rendering along caller-supplied rays and the projections (not in the reference) ----
namespace detail {
// Device memory for the calls below that take device pointers: the HIP runtime libpbrhip.so is linked with is in the process with it,
// so its hipMalloc / hipFree / hipMemcpy are found by name and a caller of this header needs no HIP headers.
class DeviceMem {
public:
  explicit DeviceMem(size_t bytes) {
    if (!Fn().malloc_ || !Fn().free_ || !Fn().memcpy_) throw std::runtime_error("the HIP runtime of libpbrhip.so was not found in the process");
    if (Fn().malloc_(&p_, bytes ? bytes : 1) != 0) throw std::runtime_error("hipMalloc failed");
  }
  ~DeviceMem() {
    if (p_) Fn().free_(p_);
  }
  DeviceMem(const DeviceMem&) = delete;
  DeviceMem& operator=(const DeviceMem&) = delete;
  void* get() const { return p_; }
  void Upload(const void* src, size_t bytes, size_t offset = 0) { Copy(static_cast<char*>(p_) + offset, src, bytes, 1); }
  void Download(void* dst, size_t bytes, size_t offset = 0) const { Copy(dst, static_cast<const char*>(p_) + offset, bytes, 2); }

private:
  struct Fns {
    int (*malloc_)(void**, size_t) = reinterpret_cast<int (*)(void**, size_t)>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    int (*free_)(void*) = reinterpret_cast<int (*)(void*)>(dlsym(RTLD_DEFAULT, "hipFree"));
    int (*memcpy_)(void*, const void*, size_t, int) = reinterpret_cast<int (*)(void*, const void*, size_t, int)>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
  };
  static const Fns& Fn() {
    static const Fns f;
    return f;
  }
  static void Copy(void* dst, const void* src, size_t bytes, int kind) {  // (hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2)
    if (bytes && Fn().memcpy_(dst, src, bytes, kind) != 0) throw std::runtime_error("hipMemcpy failed");
  }
  void* p_ = nullptr;
};
inline pbrhip_render_desc RayDesc(uint32_t width, uint32_t height, uint32_t num_sample, uint32_t first_pass, bool no_clear) {
  pbrhip_render_desc d = {};
  d.width = width, d.height = height, d.num_sample = num_sample, d.first_pass = first_pass;
  d.seed_seq = 1234567890;  // Render()'s
  d.tile_world = 1;
  d.flags = no_clear ? PBRHIP_RENDER_NO_CLEAR : 0u;
  return d;
}
}  // namespace detail

struct RayOptions {
  uint32_t camera_draws = 2;  // draws of the sample's generator the rays' maker consumed (0 .. 16)
  uint32_t first_pass = 0;
  bool no_clear = false;      // accumulate on top of *layer
};
// pbrhip_render_rays: Render() with the first ray of every sample taken from `rays`: width x height of them (one per pixel, reused by
// every pass) or num_sample x width x height (pass-major).  A ray is traced as given, tmin and tmax included; an inactive one adds
// (0, 0, 0, 1).  Throws with pbrhip_last_error() on a library error.
inline void RenderRays(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t num_sample, const std::vector<pbrhip_ray>& rays,
                       const std::atomic_bool& cancel_render_flag, RenderLayer* layer, std::atomic_size_t* finish_pass = nullptr,
                       const RayOptions& o = RayOptions()) {
  const size_t npx = size_t(width) * height;
  if (rays.size() != npx && rays.size() != npx * num_sample) throw std::runtime_error("pbrlab::RenderRays: width x height rays, or num_sample times as many");
  if (!o.no_clear || layer->width != width || layer->height != height) layer->Resize(width, height);
  scene.PushMaterialEdits();
  const pbrhip_render_desc d = detail::RayDesc(width, height, num_sample, o.first_pass, o.no_clear);
  std::atomic_size_t local_fin(0);
  std::atomic_size_t* fin = finish_pass ? finish_pass : &local_fin;
  fin->store(0);
  if (pbrhip_render_rays(scene.handle(), &d, rays.data(), rays.size() == npx ? 1u : num_sample, o.camera_draws,
                         reinterpret_cast<const volatile unsigned char*>(&cancel_render_flag), layer->rgba.data(), layer->count.data(),
                         reinterpret_cast<size_t*>(fin), nullptr) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderRays: ") + pbrhip_last_error());
}

// pbrhip_render_features_rays_device: RenderFeatures() over the same rays (uploaded, and the buffers downloaded, by this call)
inline void RenderFeaturesRays(const Scene& scene, const uint32_t width, const uint32_t height, const uint32_t num_sample,
                               const std::vector<pbrhip_ray>& rays, FeatureLayer* features, const uint32_t first_pass = 0) {
  const size_t npx = size_t(width) * height;
  if (rays.size() != npx && rays.size() != npx * num_sample) throw std::runtime_error("pbrlab::RenderFeaturesRays: width x height rays, or num_sample times as many");
  features->Resize(width, height);
  scene.PushMaterialEdits();
  const pbrhip_render_desc d = detail::RayDesc(width, height, num_sample, first_pass, false);
  detail::DeviceMem d_rays(rays.size() * sizeof(pbrhip_ray)), d_out(npx * 36);  // albedo | normal_depth | count
  d_rays.Upload(rays.data(), rays.size() * sizeof(pbrhip_ray));
  char* const out = static_cast<char*>(d_out.get());
  if (pbrhip_render_features_rays_device(scene.handle(), &d, d_rays.get(), rays.size() == npx ? 1u : num_sample, nullptr,
                                         reinterpret_cast<float*>(out), reinterpret_cast<float*>(out + npx * 16),
                                         reinterpret_cast<uint32_t*>(out + npx * 32)) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::RenderFeaturesRays: ") + pbrhip_last_error());
  d_out.Download(features->albedo.data(), npx * 16), d_out.Download(features->normal_depth.data(), npx * 16, npx * 16);
  d_out.Download(features->count.data(), npx * 4, npx * 32);
}

enum Projection { kProjectionLatLong = PBRHIP_PROJECTION_LATLONG, kProjectionFisheye = PBRHIP_PROJECTION_FISHEYE, kProjectionOrtho = PBRHIP_PROJECTION_ORTHO };
// pbrhip_projection_rays_device: the rays of passes [first_pass, first_pass + num_pass) of a width x height frame through `projection`
// about the SetCamera() frame, as host rays.  param: fisheye -- the field of view in degrees (0: the camera's); ortho -- half the height.
inline std::vector<pbrhip_ray> ProjectionRays(const Scene& scene, const Projection projection, const float param, const uint32_t width,
                                              const uint32_t height, const uint32_t first_pass, const uint32_t num_pass) {
  std::vector<pbrhip_ray> rays(size_t(width) * height * num_pass);
  detail::DeviceMem d_rays(rays.size() * sizeof(pbrhip_ray));
  if (pbrhip_projection_rays_device(scene.handle(), uint32_t(projection), param, width, height, first_pass, num_pass, 1234567890, d_rays.get(), nullptr) != PBRHIP_OK)
    throw std::runtime_error(std::string("pbrlab::ProjectionRays: ") + pbrhip_last_error());
  d_rays.Download(rays.data(), rays.size() * sizeof(pbrhip_ray));  // (a copy on the null stream: behind the kernel)
  return rays;
}

constexpr size_t kRayBufferBytes = size_t(256) << 20;  // RenderProjection's cap on its ray buffer
// A frame through a projection: in chunks of passes whose rays fit kRayBufferBytes (at least one pass), pbrhip_projection_rays_device
// then pbrhip_render_rays_device with first_pass and PBRHIP_RENDER_NO_CLEAR per chunk, all in device memory of this call's own; the frame
// does not depend on the chunking.  Clears and resizes *layer; cancel_render_flag as for Render(), *finish_pass counts the frame's passes.
// Throws with pbrhip_last_error() on a library error.
inline void RenderProjection(const Scene& scene, const Projection projection, const float param, const uint32_t width, const uint32_t height,
                             const uint32_t num_sample, const std::atomic_bool& cancel_render_flag, RenderLayer* layer,
                             std::atomic_size_t* finish_pass = nullptr) {
  layer->Resize(width, height);
  layer->Clear();
  scene.PushMaterialEdits();
  const size_t npx = size_t(width) * height;
  if (npx == 0) throw std::runtime_error("pbrlab::RenderProjection: empty image");
  const uint32_t chunk = uint32_t(std::max<size_t>(1, std::min<size_t>(std::max<uint32_t>(num_sample, 1u), kRayBufferBytes / (npx * sizeof(pbrhip_ray)))));
  detail::DeviceMem d_rays(size_t(chunk) * npx * sizeof(pbrhip_ray)), d_layer(npx * 20);  // rgba | count
  float* const d_rgba = static_cast<float*>(d_layer.get());
  uint32_t* const d_count = reinterpret_cast<uint32_t*>(static_cast<char*>(d_layer.get()) + npx * 16);
  if (finish_pass) finish_pass->store(0);
  bool rendered = false;  // (the first chunk's call clears the device layer)
  for (uint32_t done = 0; done < num_sample && !cancel_render_flag.load();) {
    const uint32_t n = std::min(chunk, num_sample - done);
    if (pbrhip_projection_rays_device(scene.handle(), uint32_t(projection), param, width, height, done, n, 1234567890, d_rays.get(), nullptr) != PBRHIP_OK)
      throw std::runtime_error(std::string("pbrlab::RenderProjection: ") + pbrhip_last_error());
    const pbrhip_render_desc d = detail::RayDesc(width, height, n, done, done != 0);
    size_t fin = 0;
    if (pbrhip_render_rays_device(scene.handle(), &d, d_rays.get(), n, 2u, nullptr, reinterpret_cast<const volatile unsigned char*>(&cancel_render_flag),
                                  d_rgba, d_count, &fin, nullptr) != PBRHIP_OK)
      throw std::runtime_error(std::string("pbrlab::RenderProjection: ") + pbrhip_last_error());
    done += n, rendered = true;
    if (finish_pass) finish_pass->store(done - n + fin);
    if (fin < n) break;  // cancelled inside the chunk
  }
  if (rendered) d_layer.Download(layer->rgba.data(), npx * 16), d_layer.Download(layer->count.data(), npx * 4, npx * 16);
}

}  // namespace pbrlab
#endif  // PBRLAB_HIP_HPP_
