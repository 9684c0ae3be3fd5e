// host_scene.h -- host-side scene model kept by libpbrhip (the "scene upload / BVH flatten / tile
// dispatch stay in C++" part of the design).  Mirrors the read side of pbrlab's Scene
// (src/scene.h:93-110), LightManager (src/light-manager.h:172-193) and Raytracer facade.
#pragma once

#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "dshade.h"

namespace pb {

struct HostMesh {
  int kind = 0;  // 0 triangle mesh, 1 cubic Bezier curve mesh (mesh/mesh.h:23)
  // triangles (mesh/attribute.h, mesh/triangle-mesh.h)
  std::vector<float> vertices, normals, texcoords;  // xyzw, xyzw, uv
  std::vector<uint32_t> vid, nid, tid, mat;
  uint32_t nfaces = 0;
  // curves (mesh/cubic-bezier-curve-mesh.h)
  std::vector<float> cverts;  // xyz + radius
  std::vector<uint32_t> cidx, cmat;
  uint32_t num_prims() const { return kind == 0 ? nfaces : (uint32_t)cidx.size(); }
};

struct HostAreaLight {  // LightManager::AreaLight (light-manager.h:174-182)
  std::vector<uint32_t> light_param_ids;
  std::vector<float> choose_prob, cdf, area_pdf;
  float intensity_sum = 0.f;
  uint32_t global_id = kNone;
};

struct HostInstance {  // MeshInstance (mesh-instance.h:22-36)
  uint32_t local_scene = 0;
  float xf[16];
  bool identity = true;  // xf is bit-for-bit the identity: the raytracer sees the meshes as they are
  std::vector<std::vector<uint32_t>> material_ids, light_ids;
  std::vector<int> has_area_light;  // per geom
  std::vector<HostAreaLight> area_lights;
};

struct HostMaterial {
  uint32_t kind = kMatPrincipled;
  PrincipledParam pr;
  HairParam hr;
};

struct HostLight {  // LightManager::Light (light-manager.h:184-188)
  float choose_prob = 0.f;
  uint32_t instance_id = 0, geom_id = 0;
};

// canonical primitive reference; index in the flattened list = gid
// One traversal primitive.  A triangle is one; a cubic Bezier curve contributes FOUR, one per linear piece of its flat
// ribbon (sub = 0..3, curve parameter [sub/4, (sub+1)/4]): tight boxes instead of one box around the whole cubic, and a
// quarter of the intersection work per test.  The index of a PrimRef in canonical (instance, geom, prim, sub) order
// is the id that breaks ties between equal hit distances.
struct PrimRef {
  uint32_t instance_id, geom_id, prim_id, kind, sub;
};

struct FlatBvh {
  std::vector<BvhNode> nodes;
  std::vector<uint32_t> slot_gid;  // leaf order -> gid
  uint32_t depth = 0;
  // what the re-insertion passes did (BvhBuildOptions; all zero when they are off)
  uint32_t reinsert_passes = 0, reinsert_moves = 0;  // passes kept, subtrees moved by them
  double reinsert_cost0 = 0.0, reinsert_cost = 0.0;  // the deciding cost of the builder's tree and of the kept one
  double build_ms = 0.0, reinsert_ms = 0.0;          // the top-down build; the passes with their evaluations
};

// Subtree re-insertion on the build-time tree: up to `reinsert_passes` passes, each over the `reinsert_top`
// largest nodes by box area; a pass is kept only while it lowers the cost the Q collapse itself would pay (for_qtree; the binary
// surface-area sum otherwise, or when the builder's own tree already needs more Q stack than there is) and the tree still fits the
// traversal stack.  0 passes: the builder's tree, byte for byte.  Sets with curves get no pass whatever the options say: the passes
// gained 3 % on the hair scene, but a frame of a small hair scene with nearly every ray suspended did not end once on such a tree and
// the reason is not known; triangle-only trees are what the flagship scenes have.
//
// What the collapse and the passes minimise (`cost`; DESIGN.md section 8, "The cost").  kBvhCostTurns prices what a ray's traversal pays
// in loop turns: a Q node visit is one turn of weight kCostNode, a triangle leaf of a triangle-only tree is one TriPair and one turn of
// weight kCostLeaf whether it holds one triangle or two, and (`surface_term`) a leaf whose box on its Q node's 8-bit grid is thicker than
// the primitives behind it by more than the rays' tmin is also charged for the rays that START on those primitives -- every bounce and
// shadow ray starts on a surface and passes such a slab.  With this cost a pass decides every move on its own (`reinsert_try`): the
// best few positions by area growth are priced by the collapse's below[root] and the node goes where that is lowest, or back.
// kBvhCostPrims is the pricing of before: a leaf costs its primitives, a node 1, no surface term, a pass placed by area growth and kept
// or undone as a whole.  Trees with curve leaves are priced that way whatever `cost` says (a curve leaf's pieces ARE tested one after
// the other) and get no passes (above).
// Like the passes, the turn cost is something the caller asks for: a default-constructed BvhBuildOptions, and build_qtree / qtree_cost /
// build_qlayout called without options, build and collapse as they always did (tests/golden/qlayout_hashes.txt records exactly that);
// the scene commit fills the options from the knobs, where both are on by default.
constexpr uint32_t kReinsertPasses = 4, kReinsertTop = 20000, kReinsertTry = 4, kMaxReinsertTry = 8;
constexpr uint32_t kBvhCostPrims = 0, kBvhCostTurns = 1;
// The weights of a node turn and of a leaf turn.  Derivation (the re-insertion's A/B on C2, which runs about 6
// closest-hit rays per 4 shadow rays): per mixed ray 0.6 * 6.28 + 0.4 * 7.54 = 6.78 node visits and 2.84 triangle tests before,
// 0.6 * 5.40 + 0.4 * 6.03 = 5.65 and 0.6 * 3.01 + 0.4 * 4.78 = 3.72 after, k_trace 29.3 -> 27.7 ms.  With time ~ n + r * l:
// 29.3 / 27.7 = (6.78 + 2.84 r) / (5.65 + 3.72 r) gives r = 0.74.  Cross-check on the loop's two blocks: the leaf turn is 168
// instructions (136 VALU) against the node turn's 198 (157 VALU), 0.85-0.87 -- an upper bound, the node turn also pays the stack
// traffic and the sort.  On walked rays (tests/cpp/bvh_rays_check.cc --explore, the flagship's scene) 0.60, 0.75 and 0.85 build trees
// within 0.4 % of each other in turns per bounce and per shadow ray, and 1.00 costs camera rays 2 % more: 0.75 stays.
constexpr double kCostNode = 1.0, kCostLeaf = 0.75;
constexpr double kSurfaceEps = 1e-3;  // the tmin of bounce and shadow rays (dshade.h): a slab thinner than this lets a ray that starts on it out
struct BvhBuildOptions {
  uint32_t reinsert_passes = 0;
  uint32_t reinsert_top = kReinsertTop;
  bool for_qtree = true;
  uint32_t cost = kBvhCostPrims;        // kBvhCostTurns: what commit asks for unless PBRHIP_BVH_COST=0; kBvhCostPrims: the tree of before, byte for byte
  bool surface_term = true;             // (kBvhCostTurns only)
  uint32_t reinsert_try = kReinsertTry; // positions priced per candidate, at most kMaxReinsertTry; 0: passes placed by area growth and kept as a whole (kBvhCostTurns only)
  double cost_leaf = kCostLeaf;         // (kBvhCostTurns only; the harness varies it)
};

// Binned-SAH BVH2 over primitive boxes; leaves hold <= kMaxLeaf primitives of ONE kind.
// boxes: lo/hi per primitive (3 floats each); kinds: 0 triangle / 1 curve.
void build_bvh(const std::vector<float>& lo, const std::vector<float>& hi, const std::vector<uint8_t>& kinds,
               FlatBvh* out, const BvhBuildOptions& opt = BvhBuildOptions());

// What the collapse below pays for a binary tree -- below[root] of its dynamic programme -- without emitting a node, and the exact
// stack need of the Q tree it would emit.
double qtree_cost(const std::vector<BvhNode>& nodes, uint32_t* stack_need, const BvhBuildOptions& opt = BvhBuildOptions());

// The binary tree collapsed to four children per node with quantised boxes (dscene.h::QNode).  Which descendants of a
// binary node become the children of its Q node -- a frontier of at most four subtrees below it -- is chosen bottom-up by
// dynamic programming over the surface-area cost WITH THE BOX A CHILD REALLY PRESENTS: its box rounded outwards on the node's
// 8-bit grid (a thin primitive in a big node is a thick slab).
// map_leaf turns a leaf reference of the binary tree into the Q tree's; it is called in the collapse's visit order, which thus
// decides where the leaves sit in memory.  The Q child takes the box the binary tree stores (already widened); quantise_node only
// rounds outwards from there, as the traversal's exactness argument needs.
// Returns the EXACT stack need of a near-first traversal of the Q tree: the maximum over root-to-leaf paths of the sum of
// (children - 1) of the nodes on the path (a node pushes all hit children but the nearest).
// opt: the cost (`cost`, `surface_term`, `cost_leaf`) -- the one the tree was built for.
uint32_t build_qtree(const std::vector<BvhNode>& nodes, const std::function<uint32_t(uint32_t)>& map_leaf, std::vector<QNode>* out,
                     const BvhBuildOptions& opt = BvhBuildOptions());

// The Q tree as the traversal kernels read it (DScene::wide: nodes, then `tri` from q_tri0, then `pts` from q_pt0; dscene.h::QNode).
struct QLayout {
  std::vector<QNode> nodes;   // empty: no Q tree (it would need more than kStackDepth stack entries, or 2^27 points or more)
  std::vector<float4> tri, pts;  // triangle leaves padded to a multiple of 4 words; curve records, then four zero words
  std::vector<uint32_t> hit;  // DScene::q_hitcode: per point, the hit code of the piece that starts there (else kNone)
  uint32_t stack_need = 0;                 // what build_qtree reported
  size_t leaves_one = 0, leaves_pair = 0;  // curve leaves of one / two pieces (counted over the collapse's visits)
};
// slots: the binary tree's slots as dscene.h lays them out (routing bits in slots[4k + 2].w); kinds: per primitive, 0 triangle / 1 curve.
void build_qlayout(const FlatBvh& bvh, const std::vector<float4>& slots, const std::vector<uint8_t>& kinds, QLayout* out,
                   const BvhBuildOptions& opt = BvhBuildOptions());

// Where the random walks' rays start (dscene.h::SssEntry), per instance: the cut of the Q tree around the instance's primitive
// bounds ilo / ihi (3 floats per instance) with at most max_foreign foreign references.  entry 0: start at the root.
std::vector<SssEntry> build_sss_entries(const std::vector<QNode>& wide, const std::vector<float>& ilo, const std::vector<float>& ihi,
                                        uint32_t max_foreign);

// The same tree format built on the GPU (bvh_gpu.hip: Morton-order linear BVH).  nodes_out: DEVICE array of
// max(n - 1, 1) nodes; order_out: slot -> primitive index; depth_out: traversal stack depth needed.
hipError_t build_bvh_gpu(hipStream_t st, const std::vector<float>& lo, const std::vector<float>& hi,
                         const std::vector<uint8_t>& kinds, BvhNode* nodes_out, std::vector<uint32_t>* order_out,
                         uint32_t* depth_out);

// The collapse of that tree into the Q tree ON THE DEVICE (qtree_gpu.hip; DESIGN.md section 8, "The collapse, exactly").  d_nodes: the
// max(n - 1, 1) binary nodes build_bvh_gpu made, d_slots: the n 64-byte slots behind them (both device).  Once the sizes are known
// `alloc(words of 16 B, hit codes, &wide, &hit)` provides the device memory of DScene::wide / q_hitcode; the layout is QLayout's:
// nodes, then tri_words triangle words (q_tri0 = 4 * nodes), then pts points (q_pt0 = q_tri0 + tri_words).
struct QCollapse {
  uint32_t nodes = 0;      // Q nodes (heads)
  size_t tri_words = 0, pts = 0;
  uint32_t levels = 0;     // launches of the marking kernel
  double alloc_ms = 0.0;   // host time spent in hipMalloc / hipFree of the working arrays and in `alloc`
  bool fits = false;       // every record index fits its reference's bits (false: nothing was allocated or written)
  bool quantised = false;  // every node could be quantised
};
hipError_t collapse_qtree_gpu(hipStream_t st, const BvhNode* d_nodes, uint32_t n, const float4* d_slots, bool tri_pairs,
                              const std::function<hipError_t(size_t, size_t, float4**, uint32_t**)>& alloc, QCollapse* out);
// The refit of both trees ON THE DEVICE after vertex / transform edits (refit_gpu.hip; DESIGN.md section 8, "The refit, exactly"): the
// topology stays, every stored box and every geometry word of a leaf record is recomputed from the slots behind the binary nodes.
// The plan -- the nodes of either tree level by level -- is built at the first refit of a committed tree and kept until the next commit.
struct RefitPlan {
  uint32_t* d_list = nullptr;  // device: nb binary node indices by level, then nq Q node indices by level
  float4* d_qbox = nullptr;    // device: the working arrays of a refit: the unwidened union of the slots below every Q node ...
  float4* d_bbox = nullptr;    // ... and below every binary node (two 16-byte words each)
  uint32_t* d_cnt = nullptr;   // device: level counter, failure flags
  std::vector<uint32_t> bin_off, q_off;  // level l of a tree is list[off[l] .. off[l + 1])
  bool built = false;
  RefitPlan() = default;
  RefitPlan(const RefitPlan&) = delete;
  RefitPlan& operator=(const RefitPlan&) = delete;
  ~RefitPlan() { release(); }
  void release();
};
struct RefitTree {  // device pointers: nb binary nodes followed by ns slots; the Q tree as DScene::wide / q_hitcode lay it out (nq 0: none)
  BvhNode* nodes = nullptr;
  uint32_t nb = 0, ns = 0;
  QNode* q = nullptr;
  uint32_t nq = 0;
  float4* tri = nullptr;
  size_t tri_words = 0;
  bool tri_pairs = false;
  float4* pts = nullptr;
  const uint32_t* hit = nullptr;
  size_t npts = 0;
};
struct RefitTimes {
  double plan_ms = 0.0, trees_ms = 0.0;  // the plan (first refit only); leaf records + both trees
  uint32_t bin_levels = 0, q_levels = 0;
  uint32_t failed = 0;  // bit 0: a Q node cannot be quantised; bit 1: an index of the tree is out of range
};
// `timed`: synchronise in front of the plan so that plan_ms is its own.  Synchronises the stream once, at the end.
hipError_t refit_tree_gpu(hipStream_t st, const RefitTree& t, bool timed, RefitPlan* plan, RefitTimes* out);
// d_packed: m slot indices padded to whole 16-byte words | m x 64 B slots | m x 128 B ShadeRecs, scattered to their places
hipError_t scatter_slots_gpu(hipStream_t st, const float4* d_packed, uint32_t m, uint32_t ns, float4* d_slots, float4* d_shade);
// the exact stack need of a near-first traversal (build_qtree's definition) of a Q tree whose children need not follow their parents
uint32_t qtree_stack_need(const std::vector<QNode>& nodes);

}  // namespace pb
