// scene_impl.h -- what libpbrhip's translation units share behind the C ABI: the error helpers, the device-buffer
// holder and the scene object (host model + device scene + render working set).  Not part of the interface.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pbrhip.h"
#include "geom_gpu.h"
#include "host_scene.h"
#include "kernels.h"
#include "rays_kernels.h"
#include "shaft_grid.h"

namespace pb {

// ------------------------------------------------------------------ errors
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int current_device();  // what pbrhip_set_device selected
#define HIPCHK(expr)                                                                                          \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess) return pb::fail(PBRHIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                                \
  } while (0)

// Every extern "C" body runs inside this guard: an allocation failure or any other C++ exception becomes an error
// code instead of unwinding through a C / ctypes caller.
template <typename F>
static inline int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(PBRHIP_ENOMEM, "out of host memory");
  } catch (const std::exception& e) {
    return fail(PBRHIP_EINVAL, "%s", e.what());
  } catch (...) {
    return fail(PBRHIP_EINVAL, "unknown C++ exception");
  }
}

// In front of the body of every entry point that reads the device scene: geometry edits are pending (pbrhip_scene_update_*)
#define PB_NOT_STALE(s)                                                                                                   \
  do {                                                                                                                    \
    if ((s)->stale) return pb::fail(PBRHIP_ESTATE, "the scene has pending geometry edits: call pbrhip_scene_refit first"); \
  } while (0)

// ------------------------------------------------------------------ device buffers
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, n = 0;
  }
  hipError_t reserve(size_t count) {
    if (count <= n) return hipSuccess;
    release();
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const std::vector<T>& h, hipStream_t s) {
    hipError_t e = reserve(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

// The binary tree with its slots and the Q tree on the device, and the one place that says how they are laid out: d_nodes holds
// num_nodes nodes, then num_slots slots (64-byte items both); d_wide holds wide_nodes Q nodes of four 16-byte words (0: no Q tree),
// then tri_words words of triangle leaves, then `points` curve points (DScene::q_tri0, q_pt0); d_qhit one hit code per point.
struct TreeBufs {
  uint32_t num_nodes = 0, num_slots = 0, wide_nodes = 0;
  size_t tri_words = 0, points = 0;
  static_assert(sizeof(BvhNode) == 64 && sizeof(QNode) == 64 && sizeof(float4) == 16, "node / slot footprint");
  DevBuf<BvhNode> d_nodes;
  DevBuf<float4> d_wide;  // filled from the host (upload), or on the device by qtree_gpu.hip (alloc_wide, then set_wide)
  DevBuf<uint32_t> d_qhit;

  static uint32_t lbvh_nodes(uint32_t n) { return n > 1 ? n - 1 : 1; }  // the nodes build_bvh_gpu makes over n primitives
  hipError_t reserve_nodes(uint32_t nodes, uint32_t slots) {
    num_nodes = nodes, num_slots = slots;
    return d_nodes.reserve((size_t)nodes + slots);
  }
  float4* slots() const { return reinterpret_cast<float4*>(d_nodes.p + num_nodes); }
  size_t tri0() const { return (size_t)wide_nodes * 4; }
  size_t pt0() const { return tri0() + tri_words; }
  float4* tri() const { return d_wide.p + tri0(); }
  float4* pts() const { return d_wide.p + pt0(); }
  void set_wide(uint32_t nodes, size_t tri_words_, size_t points_) { wide_nodes = nodes, tri_words = tri_words_, points = points_; }
  void counts_from(const TreeBufs& o) { num_nodes = o.num_nodes, num_slots = o.num_slots, set_wide(o.wide_nodes, o.tri_words, o.points); }  // (a replica)
  hipError_t alloc_wide(size_t words, size_t hits, float4** w, uint32_t** h) {  // what collapse_qtree_gpu asks for once it knows the sizes
    hipError_t e = d_wide.reserve(words);
    if (e == hipSuccess) e = d_qhit.reserve(hits);
    *w = d_wide.p, *h = d_qhit.p;
    return e;
  }
  // The Q tree from host arrays (a QLayout's, or a hook's).  No nodes: no Q tree, the buffers are released; tri_words and points
  // are recorded all the same, because commit's debug line and DScene::q_pt0 report what build_qlayout made before it gave up.
  hipError_t upload(const void* qn, uint32_t nodes, const void* tri_, size_t tw, const void* pts_, const uint32_t* hit, size_t np, hipStream_t st) {
    set_wide(nodes, tw, np);
    if (!nodes) {
      d_wide.release(), d_qhit.release();
      return hipSuccess;
    }
    hipError_t e = d_wide.reserve(pt0() + np);
    if (e == hipSuccess) e = d_qhit.reserve(np);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wide.p, qn, (size_t)nodes * 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && tw) e = hipMemcpyAsync(tri(), tri_, tw * 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && np) e = hipMemcpyAsync(pts(), pts_, np * 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && np) e = hipMemcpyAsync(d_qhit.p, hit, np * 4, hipMemcpyHostToDevice, st);
    return e;
  }
  RefitTree refit_tree(bool tri_pairs) const {  // (nq 0: no Q tree, and nothing else of it is read)
    RefitTree r;
    r.nodes = d_nodes.p, r.nb = num_nodes, r.ns = num_slots, r.tri_pairs = tri_pairs;
    r.q = reinterpret_cast<QNode*>(d_wide.p), r.nq = wide_nodes, r.hit = d_qhit.p, r.npts = points;
    r.tri = tri(), r.tri_words = tri_words, r.pts = pts();
    return r;
  }
};
// Device geometry mode (geom_gpu.h): on from the first successful pbrhip_scene_update_*_mesh_device call on a committed scene until the
// next commit.  A scene that never makes such a call holds empty buffers here and nothing else.
struct DevGeom {
  bool on = false;
  DevBuf<float4> verts, normals;           // every mesh's vertices / control points, and normals, concatenated (DgMeshRec says where)
  DevBuf<uint32_t> vidx, nidx;             // vid / cidx, and nid
  DevBuf<DgMeshRec> recs;
  DevBuf<uint32_t> geom_mesh, ig_off, slot_list;
  DevBuf<DgXf> xf;                         // per refit
  DevBuf<uint32_t> bounds, flag;
  DevBuf<float4> incoming;                 // a device update's array while it is checked: copied on only once it is accepted
  std::vector<DgMeshRec> h_recs;
  std::vector<uint32_t> inst_first;        // instance i's slots are slot_list[inst_first[i] .. inst_first[i + 1])
  std::vector<float> local_lo, local_hi;   // per instance: scene_bounds' local box, as of the last refit (the clean instances keep theirs)
  std::vector<DgXf> h_xf;                  // (staged here: outlives the copy)
  std::vector<uint32_t> h_bounds;
  uint32_t ngeoms = 0;
  double switch_ms = 0.0, download_ms = 0.0;  // since the last refit: the switch-on; the device updates' check + download to the model
  void drop() {
    on = false;
    verts.release(), normals.release(), vidx.release(), nidx.release(), recs.release(), geom_mesh.release(), ig_off.release();
    slot_list.release(), xf.release(), bounds.release(), incoming.release();
    h_recs.clear(), inst_first.clear(), local_lo.clear(), local_hi.clear(), h_xf.clear(), h_bounds.clear();
    ngeoms = 0, switch_ms = download_ms = 0.0;
  }
};
// What pbrhip_render_adaptive keeps between its rounds and calls (render_adaptive.cpp): lists of its own, so that path_pix,
// pix_index and the pk_* key stay what ensure_pixels made them.
struct AdaptiveBufs {
  DevBuf<uint32_t> tiles[2], pixels;       // the active tiles (in / out of a decision step) and the next round's pixel list
  DevBuf<uint32_t> keep, tile_off, pix_off, totals;
  DevBuf<float4> snapshot;                 // A: W x H
  DevBuf<float> tile_error;                // ceil(W / 8) x ceil(H / 8)
  std::vector<uint32_t> tiles0;            // the rank's tiles in the order of ensure_pixels' list: round 0's
  uint32_t key[7] = {0, 0, 0, 0, 0, 0, 0}; // the pk_* key tiles0 was derived under
};
// What defines the camera pbrhip_render derives for an image size: the caller's look-at camera (set), else the scene's bounds
struct PoseCamera {
  bool set = false;
  float eye[3] = {0, 0, 0}, lookat[3] = {0, 0, -1}, up[3] = {0, 1, 0};
  float vfov = 30.0f, lens = 0.0f, focus = 0.0f;
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
};
// What the signed-distance queries keep (sdf.cpp): sdf_topology.h's lists on the device -- built at the first signed
// call after a commit, because topology is fixed across refits -- and the pseudonormal table, built lazily from the slots as they are
// and invalidated by a refit.  A commit drops all of it.  A scene that never asks for signed distance holds empty buffers here.
struct SdfState {
  bool topology = false, table_valid = false;
  DevBuf<uint32_t> slot_feat, feat_off, feat_items;
  DevBuf<float4> faces, table;  // 2 and kSdfRows words per slot
  pbrhip_sd_info info = {};
  void drop() {
    topology = table_valid = false, info = pbrhip_sd_info{};
    slot_feat.release(), feat_off.release(), feat_items.release(), faces.release(), table.release();
  }
};
// The per-light shaft grid (shaft_grid.h): built on the device from the trees as they are -- at the end of a commit, and
// before the next render by whoever finds it invalid (after a refit, on a replica, after a change of its knobs).
struct ShaftState {
  bool valid = false;                 // `cells` describes the device scene as it is (or the scene gets no grid: n == 0)
  uint32_t n = 0, max_list = 0;       // what it was built with (n 0: no grid)
  uint32_t num_lights = 0;
  DevBuf<uint32_t> cells;
  double build_ms = 0.0;
  uint64_t culled = 0, clear_rays = 0, pair_tests = 0;  // of the last statistics render
  void drop() {
    valid = false, n = max_list = num_lights = 0, build_ms = 0.0;
    cells.release();
  }
};
inline bool all_triangles(const std::vector<uint8_t>& kinds) {  // (the Q tree's triangle leaves are TriPairs, dscene.h)
  return std::all_of(kinds.begin(), kinds.end(), [](uint8_t kd) { return kd == 0; });
}

}  // namespace pb

struct pbrhip_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  // host model
  std::vector<pb::HostMesh> meshes;
  std::vector<std::vector<uint32_t>> locals;
  std::vector<pb::HostInstance> instances;
  std::vector<pb::HostMaterial> materials;
  std::vector<pb::V3> light_params;
  std::vector<pb::TexDesc> tex_descs;  // Scene::AddTexture
  std::vector<float> tex_pixels;
  std::vector<pb::HostLight> lights;
  std::vector<float> light_cdf;
  bool committed = false, has_hair = false, has_sss = false, has_textured = false;  // has_sss: a material can enter a medium (or is textured)
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  uint32_t bvh_depth = 0;
  int bvh_builder = PBRHIP_BVH_HOST_SAH;
  bool bvh_built_on_gpu = false;
  uint32_t wide_stack_need = 0;    // of the Q tree (0: none): pbrhip_scene_wide_info
  bool wide_built_on_gpu = false;  // the Q tree was collapsed on the device (PBRHIP_BVH_GPU_LBVH_WIDE)
  // geometry edits on a committed scene (pbrhip_scene_update_triangle_mesh / _curve_mesh / _instance_transform) and what
  // pbrhip_scene_refit needs of the last commit ("The refit, exactly")
  bool stale = false;               // edits are pending: the device scene is not the model's until pbrhip_scene_refit or a commit
  bool replica = false;             // made by pbrhip_scene_replicate: no host geometry, nothing to edit or refit
  std::vector<uint8_t> dirty_inst;  // per instance: a mesh of its local scene or its transform changed since the device scene was made
  std::vector<uint32_t> slot_gid;   // slot -> canonical primitive id, as the builder ordered the leaves
  std::vector<pb::LightHead> light_heads;  // light -> its stretch of light records (fixed by the topology)
  std::vector<float> inst_lo, inst_hi;     // per instance: the bounds of its primitives' boxes (what the random walks' entries are cut around)
  // what bind_dscene needs beside the buffers (recorded by commit and refit, carried over by pbrhip_scene_replicate)
  uint32_t num_curves = 0, num_lrecs = 0, num_walk_entries = 0;  // curve pieces among the slots; light records; entries in d_sss_entries (0: none)
  bool lights_transformed = false;  // DScene::lights_transformed
  pb::RefitPlan rf_plan;            // built at the first refit of a committed tree, dropped by the next commit
  pb::DevBuf<float4> rf_packed;     // the dirty slots' upload: index | 64 B | 128 B (refit_gpu.hip::k_rf_scatter)
  pb::DevGeom dg;                   // device geometry mode (off, and empty, unless a *_mesh_device update switched it on)
  pb::ShaftState shaft;             // the per-light shaft grid (no cells unless the scene gets one)
  std::vector<float> light_box;     // per light: lo xyz, hi xyz of its primitives (stage_lights; carried over by pbrhip_scene_replicate)
  pb::SdfState sdf;                 // the signed-distance queries' lists and table (empty unless one was asked)
  // device scene
  pb::TreeBufs tree;
  pb::DevBuf<pb::ShadeRec> d_shade;
  pb::DevBuf<pb::Material> d_materials;
  pb::DevBuf<float> d_light_cdf, d_lprim_cdf, d_tex_pixels;
  pb::DevBuf<pb::TexDesc> d_tex_descs;
  pb::DevBuf<pb::LightHead> d_heads;
  pb::DevBuf<pb::LightRec> d_lrecs;
  pb::DevBuf<pb::BvhNode> d_light_boxes;
  pb::DevBuf<pb::SssEntry> d_sss_entries;  // DScene::sss_entries
  // the environment light as the caller set it (pbrhip_scene_set_environment; kept for pbrhip_scene_replicate) and its device tables
  std::vector<float> env_rgb;
  uint32_t env_w = 0, env_h = 0;
  float env_scale = 1.0f, env_m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  pb::DevBuf<float4> d_env_texels;  // DScene::env_texels
  pb::DevBuf<uint2> d_env_alias;    // DScene::env_alias
  // the look-at camera as the caller set it (pbrhip_scene_set_camera; kept for pbrhip_scene_replicate): none = the reference's
  bool cam_set = false;
  float cam_eye[3] = {0, 0, 0}, cam_lookat[3] = {0, 0, -1}, cam_up[3] = {0, 1, 0};
  float cam_vfov = 30.0f, cam_lens = 0.0f, cam_focus = 0.0f;
  pb::DevBuf<uint32_t> hook_xyp;  // pbrhip_camera_rays' (x, y, pass) triples
  pb::DevBuf<float4> own_rays;    // pbrhip_render_rays' device copy of the caller's host rays
  // pbrhip_scene_snapshot_pose: the slots and the camera state of the pose it was taken at; dropped by the next commit
  // (slot order changes), not carried by pbrhip_scene_replicate.  A scene that never takes one holds an empty buffer and nothing else.
  bool pose_set = false;
  pb::DevBuf<float4> pose_slots;  // tree.num_slots x 4 words, DScene::slots' layout
  pb::PoseCamera pose_cam;
  pb::DScene dscene;
  // render working set (grown on demand, reused across calls)
  pb::DevBuf<float4> rec, srec, ssrec, L, hit, sss_A, sh_e;  // path state (kernels.h::PathState): rec = 4 words of 16 B per path, srec = 2
  pb::DevBuf<uint32_t> q[7], counts, pix_index, path_pix, spill;  // pix_index: the rank's pixels in the shard's order (exchange); path_pix: in the order the paths are laid out in
  pb::DevBuf<unsigned long long> stats;
  pb::DevBuf<float> own_rgba;
  pb::DevBuf<uint32_t> own_count;
  pb::DevBuf<float4> hook_rays;
  pb::DevBuf<pb::HookHit> hook_hits;
  pb::DevBuf<uint8_t> hook_occ;
  uint32_t* h_counts = nullptr;            // pinned, kMaxGroups x kCntNum
  // Round 6: what the host learns about an iteration it enqueued -- written by the iteration's last kernel (k_advance) straight into
  // pinned host memory: kRingSlots slots of 4 words per group lane: live paths, pending shadow rays, overflow flag, stamp (a number
  // that is unique per scene and launch, written last).  The host polls the stamp: no copy, no stream query, and the NEXT iteration
  // is already enqueued behind this one (pbrhip.cpp::ChunkRun).
  uint32_t* h_ring = nullptr;              // pinned, kMaxGroups x kRingSlots x 4
  uint32_t* d_ring = nullptr;              // the same memory as the device addresses it
  uint32_t ring_stamp = 0;                 // last stamp handed out
  pb::DevBuf<uint32_t> heads;              // the heads of k_trace's ray queue: lanes x kTraceHeads x kHeadStride words
  pb::DevBuf<uint32_t> susp;               // suspend records of the resumable rays: lanes x 2 (written / read by alternate launches) x cap x kSuspWords
  std::vector<hipStream_t> group_streams;  // streams of path groups 1.. (group 0 uses `stream`)
  // pixel list cache key (ensure_pixels)
  uint32_t pk_w = 0, pk_h = 0, pk_rank = 0, pk_world = 0, pk_block = 0, pk_tile = 0, pk_npix = 0;
  std::vector<hipEvent_t> events;
  // layer exchange (multi.cpp): packed shard of this rank / staging for the shards of the others
  pb::DevBuf<float> xchg_send, xchg_recv;
  pb::DevBuf<uint32_t> xchg_pix;                  // pixel lists of the ranks whose shards arrive here, concatenated
  std::vector<size_t> xk_off, xk_cnt;             // per rank: first entry in xchg_pix / number of pixels
  uint32_t xk_key[7] = {0, 0, 0, 0, 0, 0, 0};     // w, h, world, block, first rank, end rank, skipped rank
  pb::DevBuf<float4> feat_albedo;                 // pbrhip_render_features: per material, albedo rgb | base-colour texture id (feature_kernels.h)
  pb::AdaptiveBufs as;                            // pbrhip_render_adaptive's lists and snapshot (empty unless it was called)

  // The buffers of the device scene, each named once.  `s.member...` expands over the scenes given: f(counted, buffer) for one scene,
  // f(counted, buffer, its counterpart) for two.  `counted`: in pbrhip_scene_info's device bytes.  (Not the environment's tables.)
  template <typename F, typename... S>
  static void each_scene_buf(F&& f, S&... s) {
    f(true, s.tree.d_nodes...), f(true, s.tree.d_wide...), f(true, s.tree.d_qhit...), f(true, s.d_shade...), f(true, s.d_materials...), f(true, s.d_lrecs...);
    f(false, s.d_light_cdf...), f(false, s.d_lprim_cdf...), f(false, s.d_tex_pixels...), f(false, s.d_tex_descs...), f(false, s.d_heads...);
    f(false, s.d_light_boxes...), f(false, s.d_sss_entries...);
    // (the shaft grid is not here: a replica builds its own; device_bytes counts it)
  }
  size_t device_bytes() const {
    size_t bytes = 0;
    each_scene_buf([&](bool counted, const auto& b) { bytes += counted ? b.n * sizeof(*b.p) : 0; }, *this);
    bytes += shaft.cells.n * sizeof(uint32_t);
    return bytes;
  }
};

namespace pb {
// pixel indices (y * w + x) of the blocks of rank `rank` in CreateTiles order (render-tile.cc:29-41 for block = 64)
void shard_pixels(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t block, std::vector<uint32_t>* out);
int ensure_pixels(pbrhip_scene* s, const Knobs& k, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t block);
// pbrhip_scene_set_environment's body (rgb null: no environment); also what pbrhip_scene_replicate calls to carry it over
int set_environment(pbrhip_scene* s, const float* rgb, uint32_t width, uint32_t height, float scale, const float* world_to_env);
// pbrhip_scene_set_camera's body (eye null: the reference's camera); also what pbrhip_scene_replicate calls to carry it over
int set_camera(pbrhip_scene* s, const float* eye, const float* lookat, const float* up, float vfov, float lens_radius, float focus_distance);
// the body of pbrhip_render_device (device pointers on the scene's device).  d_pixels: null, or a device list of num_pixels of the
// rank's pixels (y * width + x, distinct) to render in place of ensure_pixels' list (render_adaptive.cpp); the cached list stays as it is.
// rays: null, or the caller's first rays in place of the scene's camera (base_pass and height are filled in here)
int render_impl(pbrhip_scene* s, const pbrhip_render_desc* d, const volatile unsigned char* cancel, float* d_rgba,
                uint32_t* d_count, size_t* finish_pass, pbrhip_render_stats* stats, const uint32_t* d_pixels = nullptr,
                uint32_t num_pixels = 0, const RaySource* rays = nullptr);
// the shaft grid of the device scene as it is, under these knobs: kept if valid, else built (or dropped: a scene that gets none); binds DScene::shaft_*
int ensure_shadow_grid(pbrhip_scene* s, const Knobs& k);
void bind_dscene(pbrhip_scene* s);  // points every DScene member that comes from a scene buffer at it, with its count (commit.cpp)
inline const HostMesh* inst_mesh(const pbrhip_scene* s, uint32_t instance_id, uint32_t geom_id) {  // (per primitive in commit's loops: inline)
  const HostInstance& in = s->instances[instance_id];
  return &s->meshes[s->locals[in.local_scene][geom_id]];
}
int update_material(pbrhip_scene* s, uint32_t id, const HostMaterial& hm);  // pbrhip_scene_update_*_material's body (commit.cpp)
// pbrhip_scene_update_triangle_mesh_device / _curve_mesh_device after their argument checks (commit.cpp): the arrays checked on the
// device, downloaded into the model and, on a committed scene, taken into the device copy (switching device geometry mode on)
int update_mesh_device(pbrhip_scene* s, uint32_t mesh_id, const void* d_verts, const void* d_normals, void* stream, const char* who);
// device geometry mode on: the device copy of a mesh the host update calls just edited, refreshed from the model
int refresh_mesh_device(pbrhip_scene* s, uint32_t mesh_id);
// the scene's cameras for a width x height image (pbrhip.cpp; pbrhip_camera_rays launches them too)
UserCamera make_user_camera(const pbrhip_scene* s, uint32_t width, uint32_t height);
Camera make_camera(const pbrhip_scene* s, uint32_t width, uint32_t height);
// the same two from a recorded state (pose_camera: the scene's current one)
PoseCamera pose_camera(const pbrhip_scene* s);
UserCamera make_user_camera(const PoseCamera& c, uint32_t width, uint32_t height);
Camera make_camera(const PoseCamera& c, uint32_t width, uint32_t height);
// what every call on a render descriptor checks first: the scene's state, the image's size, the shard (pbrhip.cpp)
int check_render_desc(const pbrhip_scene* s, const pbrhip_render_desc* d);
// what the ray-list entry points check before anything touches a device: pointers, then the shape of the ray buffer, then the scene
int check_ray_args(const char* who, const pbrhip_scene* s, const pbrhip_render_desc* d, const void* rays, uint32_t ray_passes, uint32_t camera_draws);

// A caller's device array is read only after what its stream already holds (pbrhip_scene_update_triangle_mesh_device's rule): an event
// there, and the scene's stream -- behind which every path group starts -- waits for it
inline int wait_for_caller_stream(pbrhip_scene* s, void* stream) {
  hipEvent_t ev;
  HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, ev, 0);
  (void)hipEventDestroy(ev);
  HIPCHK(e);
  return PBRHIP_OK;
}
// In front of a one-ray-per-lane traversal outside the render loop (feature passes, motion, queries): zeroed counters (queue head,
// overflow flag) and the spill area, on the scene's stream
inline int prepare_traversal(pbrhip_scene* s) {
  HIPCHK(s->counts.reserve(kCntNum * kMaxGroups));
  HIPCHK(hipMemsetAsync(s->counts.p, 0, sizeof(uint32_t) * kCntNum, s->stream));
  HIPCHK(s->spill.reserve(kSpillWords));
  return PBRHIP_OK;
}
// ... and behind it: the counters come back, the stream drains, an overflow is reported
inline int finish_traversal(pbrhip_scene* s) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s->h_counts, s->counts.p, sizeof(uint32_t) * kCntNum, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (s->h_counts[kCntOverflow]) return fail(PBRHIP_EOVERFLOW, "BVH traversal stack overflow");
  return PBRHIP_OK;
}
}  // namespace pb
