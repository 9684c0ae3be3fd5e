// hooks.cpp -- the test hooks of the C ABI: single kernels and builders run on caller-provided arrays.  Host C++ only.
#include <string.h>

#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(pbrhip_hit) == sizeof(HookHit), "hit layout");
static_assert(sizeof(pbrhip_ray) == 32, "ray layout");

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

struct Stream {  // what a scene-less hook starts with (hook_stream): the device checked and selected, a stream of its own
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
static int hook_stream(const char* hook, int device, Stream* st) {
  int ndev = 0;
  if (int rc = pbrhip_device_count(&ndev)) return rc;
  if (ndev <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(PBRHIP_EINVAL, "%s: device %d out of range (%d devices)", hook, device, ndev);
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking));
  return PBRHIP_OK;
}

// the GPU builder on bare boxes, whatever depth it reaches (the fallback at kStackDepth is pbrhip_scene_commit's)
extern "C" int pbrhip_lbvh_build(int device, const float* lo, const float* hi, const uint8_t* kinds, uint32_t n, void* nodes_out,
                                 uint32_t* order_out, uint32_t* depth_out) {
  return guarded([&]() -> int {
    if (n >= (1u << 27)) return fail(PBRHIP_EINVAL, "lbvh_build: too many boxes (%u)", n);
    if (n == 0) return PBRHIP_OK;
    if (!lo || !hi || !kinds || !nodes_out || !order_out || !depth_out) return fail(PBRHIP_EINVAL, "lbvh_build: NULL argument");
    Stream st;
    if (int rc = hook_stream("lbvh_build", device, &st)) return rc;
    TreeBufs t;  // (the nodes alone)
    HIPCHK(t.reserve_nodes(TreeBufs::lbvh_nodes(n), 0));
    const std::vector<float> vlo(lo, lo + 3 * (size_t)n), vhi(hi, hi + 3 * (size_t)n);
    const std::vector<uint8_t> vkinds(kinds, kinds + n);
    std::vector<uint32_t> order;
    uint32_t depth = 0;
    HIPCHK(build_bvh_gpu(st.s, vlo, vhi, vkinds, t.d_nodes.p, &order, &depth));
    HIPCHK(hipMemcpyAsync(nodes_out, t.d_nodes.p, (size_t)t.num_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost, st.s));
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
    Stream st;
    if (int rc = hook_stream("qtree_collapse", device, &st)) return rc;
    TreeBufs t;  // the layout of a committed scene: the slots follow the nodes in leaf order
    HIPCHK(t.reserve_nodes(TreeBufs::lbvh_nodes(n), n));
    const std::vector<float> vlo(lo, lo + 3 * (size_t)n), vhi(hi, hi + 3 * (size_t)n);
    const std::vector<uint8_t> vkinds(kinds, kinds + n);
    std::vector<uint32_t> order;
    uint32_t depth = 0;
    HIPCHK(build_bvh_gpu(st.s, vlo, vhi, vkinds, t.d_nodes.p, &order, &depth));
    std::vector<BvhNode> sl(n);  // (a slot is 64 bytes, like a node)
    for (uint32_t k = 0; k < n; k++) memcpy(&sl[k], static_cast<const char*>(slots) + 64 * (size_t)order[k], 64);
    HIPCHK(hipMemcpyAsync(t.slots(), sl.data(), 64 * (size_t)n, hipMemcpyHostToDevice, st.s));
    QCollapse qc;
    HIPCHK(collapse_qtree_gpu(st.s, t.d_nodes.p, n, t.slots(), all_triangles(vkinds), [&](auto... a) { return t.alloc_wide(a...); }, &qc));
    sizes_out[0] = qc.nodes, sizes_out[1] = (uint32_t)qc.tri_words, sizes_out[2] = (uint32_t)qc.pts, sizes_out[3] = 0;
    sizes_out[4] = (qc.fits ? 1u : 0u) | (qc.quantised ? 2u : 0u), sizes_out[5] = depth;
    if (!qc.fits || !qnodes_out) return PBRHIP_OK;  // (a call without output arrays reports the sizes)
    t.set_wide(qc.nodes, qc.tri_words, qc.pts);
    std::vector<QNode> qn(qc.nodes);
    HIPCHK(hipMemcpyAsync(nodes_out, t.d_nodes.p, (size_t)t.num_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(qn.data(), t.d_wide.p, (size_t)qc.nodes * 64, hipMemcpyDeviceToHost, st.s));
    if (qc.tri_words) HIPCHK(hipMemcpyAsync(tri_out, t.tri(), qc.tri_words * 16, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(pts_out, t.pts(), qc.pts * 16, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(hit_out, t.d_qhit.p, qc.pts * 4, hipMemcpyDeviceToHost, st.s));
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
    Stream st;
    if (int rc = hook_stream("tree_refit", device, &st)) return rc;
    TreeBufs t;  // the layout of a committed scene
    HIPCHK(t.reserve_nodes(TreeBufs::lbvh_nodes(n), n));
    HIPCHK(hipMemcpyAsync(t.d_nodes.p, nodes_inout, (size_t)t.num_nodes * 64, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(t.slots(), slots, (size_t)n * 64, hipMemcpyHostToDevice, st.s));
    if (qnodes_inout) HIPCHK(t.upload(qnodes_inout, num_qnodes, tri_inout, tri_words, pts_inout, hit, num_points, st.s));
    RefitPlan plan;
    RefitTimes rt;
    HIPCHK(refit_tree_gpu(st.s, t.refit_tree(tri_pairs != 0), false, &plan, &rt));
    if (rt.failed) return fail(PBRHIP_EHIP, "tree_refit: %s", (rt.failed & 1u) ? "a node of the Q tree cannot be quantised" : "the tree holds an index out of range");
    HIPCHK(hipMemcpyAsync(nodes_inout, t.d_nodes.p, (size_t)t.num_nodes * 64, hipMemcpyDeviceToHost, st.s));
    if (t.wide_nodes) {
      HIPCHK(hipMemcpyAsync(qnodes_inout, t.d_wide.p, (size_t)t.wide_nodes * 64, hipMemcpyDeviceToHost, st.s));
      if (tri_words) HIPCHK(hipMemcpyAsync(tri_inout, t.tri(), (size_t)tri_words * 16, hipMemcpyDeviceToHost, st.s));
      if (num_points) HIPCHK(hipMemcpyAsync(pts_inout, t.pts(), (size_t)num_points * 16, hipMemcpyDeviceToHost, st.s));
    }
    HIPCHK(hipStreamSynchronize(st.s));
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_leaf_eval(uint32_t op, const float* in, size_t n, uint32_t in_words, float* out, uint32_t out_words) {
  return guarded([&]() -> int {
    if ((!in || !out) && n) return fail(PBRHIP_EINVAL, "leaf_eval: NULL argument");
    if (op > 13u || in_words == 0 || out_words == 0 || n > (1u << 24)) return fail(PBRHIP_EINVAL, "leaf_eval: bad operation or sizes");
    static const uint32_t need_in[14] = {4, 3, 2, 2, 2, 2, 2, 9, 8, 29, 30, 25, 11, 21}, need_out[14] = {1, 1, 1, 1, 5, 3, 2, 2, 5, 4, 7, 23, 8, 15};
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
