// bvh_build.cpp -- host BVH2 builder + flatten (replaces Embree's rtcCommitScene,
// src/raytracer/raytracer_impl.cc:136-147,181-192).  Binned SAH (48 bins), leaves of <= kMaxLeaf
// primitives of a single kind, 64-byte nodes that carry both children's boxes so that one node fetch
// decides both descents.  Large subtrees are built on worker threads.  Optionally (BvhBuildOptions) the largest subtrees of a
// triangle-only tree are re-inserted before it is flattened: the best few positions by area growth are priced by the Q collapse's own
// cost -- loop turns of the traversal, host_scene.h::BvhBuildOptions -- and the subtree goes where that is lowest.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <functional>
#include <future>
#include <limits>
#include <thread>

#include "host_scene.h"
#include "qquant.h"

namespace pb {
namespace {

#ifndef PB_SAH_BINS
#define PB_SAH_BINS 48  // (round 4: 16 -> 48 bins: k_trace of C2 -2.4 %, of the hair scene -3.9 %, of C5 -0.6 %; 24 and 32 are better on two of the three)
#endif
constexpr int kBins = PB_SAH_BINS;
#ifndef PB_SAH_SWEEP
#define PB_SAH_SWEEP 256  // ranges of at most this many primitives are split by the exact SAH (all positions of all axes) instead of by bins
#endif
#ifndef PB_MAX_LEAF_CURVES
#define PB_MAX_LEAF_CURVES PB_MAX_LEAF  // curve pieces per leaf (1: every piece behind its own box)
#endif
constexpr float kTraversalCost = 1.0f;
constexpr float kPrimCost = 1.5f;

struct Box {
  float lo[3], hi[3];
  void reset() {
    for (int a = 0; a < 3; a++) lo[a] = std::numeric_limits<float>::infinity(), hi[a] = -lo[a];
  }
  void grow(const float* l, const float* h) {
    for (int a = 0; a < 3; a++) {
      lo[a] = std::min(lo[a], l[a]);
      hi[a] = std::max(hi[a], h[a]);
    }
  }
  void grow(const Box& b) { grow(b.lo, b.hi); }
  float area() const {
    float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    if (!(dx >= 0 && dy >= 0 && dz >= 0)) return 0.f;
    return 2.f * (dx * dy + dy * dz + dz * dx);
  }
};

struct TNode {  // build-time tree
  Box box;
  int32_t left = -1, right = -1;  // children (indices into the owning pool) or -1 for leaf
  uint32_t first = 0, count = 0;  // leaf range in the order array
  uint8_t kind = 0;
  uint32_t depth = 1;
};

struct Builder {
  const float* lo;
  const float* hi;
  const uint8_t* kinds;
  std::vector<float> cen;
  std::vector<uint32_t> order;

  struct Pool {
    std::vector<TNode> nodes;
  };

  bool uniform_kind(uint32_t first, uint32_t count) const {
    uint8_t k = kinds[order[first]];
    for (uint32_t i = first + 1; i < first + count; i++)
      if (kinds[order[i]] != k) return false;
    return true;
  }

  // returns node index inside pool
  int32_t build(Pool& pool, uint32_t first, uint32_t count, uint32_t depth) {
    int32_t id = (int32_t)pool.nodes.size();
    pool.nodes.emplace_back();
    Box box, cbox;
    box.reset(), cbox.reset();
    for (uint32_t i = first; i < first + count; i++) {
      uint32_t g = order[i];
      box.grow(lo + 3 * g, hi + 3 * g);
      cbox.grow(&cen[3 * g], &cen[3 * g]);
    }
    pool.nodes[id].box = box;
    pool.nodes[id].depth = depth;
    bool uni = uniform_kind(first, count);
    const uint32_t max_leaf = (uni && kinds[order[first]] != 0) ? (uint32_t)PB_MAX_LEAF_CURVES : (uint32_t)kMaxLeaf;
    if (count <= max_leaf && uni) {
      pool.nodes[id].first = first, pool.nodes[id].count = count, pool.nodes[id].kind = kinds[order[first]];
      return id;
    }
    uint32_t mid = first;
    // a range whose box has no area -- segments of one axis-parallel line, or points of it -- prices every split at 0: the SAH says
    // nothing there and its first candidate would peel one primitive (or bin) off per level; such a range is halved by the median
    const bool flat = !(box.area() > 0.f);
    if (!uni && count <= (uint32_t)kMaxLeaf) {
      // mixed small range: split by kind
      mid = (uint32_t)(std::partition(order.begin() + first, order.begin() + first + count,
                                      [&](uint32_t g) { return kinds[g] == 0; }) -
                       order.begin());
    } else if (!flat && count <= (uint32_t)PB_SAH_SWEEP) {
      // small ranges: the exact SAH -- every split position of every axis (the bins are too coarse down here), the two sides
      // priced by the LEAVES they will make (kMaxLeaf primitives each: an odd split of four triangles costs a third leaf)
      auto leaves = [max_leaf](uint32_t n) { return (float)((n + max_leaf - 1u) / max_leaf); };
      std::vector<uint32_t> idx(order.begin() + first, order.begin() + first + count), best_idx;
      std::vector<float> rarea(count);
      float best_cost = std::numeric_limits<float>::infinity();
      uint32_t best_k = 0;
      for (int a = 0; a < 3; a++) {
        if (!(cbox.hi[a] - cbox.lo[a] > 0.f)) continue;
        std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cen[3 * x + a] < cen[3 * y + a] || (cen[3 * x + a] == cen[3 * y + a] && x < y); });
        Box acc;
        acc.reset();
        for (uint32_t k = count - 1; k > 0; k--) acc.grow(lo + 3 * idx[k], hi + 3 * idx[k]), rarea[k] = acc.area();
        acc.reset();
        bool better = false;
        for (uint32_t k = 0; k + 1 < count; k++) {
          acc.grow(lo + 3 * idx[k], hi + 3 * idx[k]);
          const float cost = acc.area() * leaves(k + 1) + rarea[k + 1] * leaves(count - k - 1);
          if (cost < best_cost) best_cost = cost, best_k = k + 1, better = true;
        }
        if (better) best_idx = idx;
      }
      if (!best_idx.empty()) {
        std::copy(best_idx.begin(), best_idx.end(), order.begin() + first);
        mid = first + best_k;
      } else {
        mid = first + count / 2;  // all centroids coincide: halves in the order they are in
      }
    } else {
      int best_axis = -1, best_bin = 0;
      float best_cost = std::numeric_limits<float>::infinity();
      for (int a = 0; a < 3 && !flat; a++) {
        float ext = cbox.hi[a] - cbox.lo[a];
        if (!(ext > 0.f)) continue;
        Box bb[kBins];
        uint32_t bc[kBins];
        for (int k = 0; k < kBins; k++) bb[k].reset(), bc[k] = 0;
        float scale = (float)kBins / ext;
        for (uint32_t i = first; i < first + count; i++) {
          uint32_t g = order[i];
          int k = std::min(kBins - 1, std::max(0, (int)((cen[3 * g + a] - cbox.lo[a]) * scale)));
          bb[k].grow(lo + 3 * g, hi + 3 * g);
          bc[k]++;
        }
        float rarea[kBins];
        uint32_t rcnt[kBins];
        Box acc;
        acc.reset();
        uint32_t n = 0;
        for (int k = kBins - 1; k > 0; k--) {
          acc.grow(bb[k]);
          n += bc[k];
          rarea[k] = acc.area();
          rcnt[k] = n;
        }
        acc.reset();
        n = 0;
        for (int k = 0; k < kBins - 1; k++) {
          acc.grow(bb[k]);
          n += bc[k];
          if (n == 0 || rcnt[k + 1] == 0) continue;
          float cost = acc.area() * (float)n + rarea[k + 1] * (float)rcnt[k + 1];
          if (cost < best_cost) best_cost = cost, best_axis = a, best_bin = k;
        }
      }
      if (best_axis >= 0) {
        float scale = (float)kBins / (cbox.hi[best_axis] - cbox.lo[best_axis]);
        float base = cbox.lo[best_axis];
        mid = (uint32_t)(std::partition(order.begin() + first, order.begin() + first + count,
                                        [&](uint32_t g) {
                                          int k = std::min(kBins - 1, std::max(0, (int)((cen[3 * g + best_axis] - base) * scale)));
                                          return k <= best_bin;
                                        }) -
                         order.begin());
      }
      if (mid == first || mid == first + count) {
        // all centroids coincide, the range is flat or the SAH found no split: median split on the widest axis
        int a = 0;
        for (int c = 1; c < 3; c++)
          if (cbox.hi[c] - cbox.lo[c] > cbox.hi[a] - cbox.lo[a]) a = c;
        mid = first + count / 2;
        std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                         [&](uint32_t x, uint32_t y) { return cen[3 * x + a] < cen[3 * y + a] || (cen[3 * x + a] == cen[3 * y + a] && x < y); });
      }
    }
    int32_t l = build(pool, first, mid - first, depth + 1);
    int32_t r = build(pool, mid, first + count - mid, depth + 1);
    pool.nodes[id].left = l;
    pool.nodes[id].right = r;
    return id;
  }
};

uint32_t leaf_ref(const TNode& n) {
  return kLeafBit | (n.kind ? kCurveBit : 0u) | (n.first << 3) | (n.count - 1u);
}

// The binary tree as a tree of boxes whose leaves are the Q tree's leaf references: what the collapse's dynamic programme reads.
struct QV {
  float lo[3], hi[3];
  int32_t l = -1, r = -1;  // children, or -1: leaf
  uint32_t ref = 0;        // leaf: the Q tree's reference
  uint32_t prims = 0;      // leaf: primitives behind the reference
  uint8_t curve = 0;       // leaf: a curve leaf
};

// What a vertex of the collapse's programme is charged (host_scene.h::BvhBuildOptions): a node turn, a leaf turn (per primitive: the
// pricing of before and of trees with curve leaves), and per unit of a leaf's primitive area the rays that start on it (0: not priced).
struct QCost {
  double node = 1.0, leaf = 1.0;
  bool per_prim = true;
  double surface = 0.0;  // area of the root's box / primitive area of the scene: the share of surface-origin rays, in the units of qarea
};
// The area of the primitives behind a leaf, from its box alone (the builder never sees corners): a triangle is half a parallelogram
// whose projections fill its box's faces at most, so 1/2 |(dy dz, dz dx, dx dy)| bounds it from above and is exact for the axis-aligned
// right triangles that walls and floors are made of; a leaf of two is priced as the whole parallelogram.
double leaf_prim_area(const float* lo, const float* hi, uint32_t prims) {
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  const double a = sqrt(dx * dy * dx * dy + dy * dz * dy * dz + dz * dx * dz * dx);
  return std::isfinite(a) ? (prims >= 2 ? a : 0.5 * a) : 0.0;
}
double half_area(const float* lo, const float* hi) {
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  const double a = dx * dy + dy * dz + dz * dx;
  return a >= 0.0 && std::isfinite(a) ? a : 0.0;
}
QCost make_qcost(const BvhBuildOptions& opt, bool curves, double root_area, double prim_area) {
  QCost C;
  if (opt.cost == kBvhCostPrims || curves) return C;
  C.node = kCostNode, C.leaf = opt.cost_leaf, C.per_prim = false;
  if (opt.surface_term && prim_area > 0.0 && std::isfinite(root_area / prim_area)) C.surface = root_area / prim_area;
  return C;
}

// ... of a flattened tree.  Children follow their parent.
void qv_of_nodes(const std::vector<BvhNode>& N2, const std::function<uint32_t(uint32_t)>& map_leaf, std::vector<QV>* out) {
  std::vector<QV>& T = *out;
  T.clear();
  T.reserve(N2.size() * 2 + 1);
  struct Todo {
    uint32_t node2;
    int32_t v;
  };
  std::vector<Todo> todo;
  T.emplace_back();
  todo.push_back({0u, 0});
  while (!todo.empty()) {
    const Todo t = todo.back();
    todo.pop_back();
    const BvhNode& b = N2[t.node2];
    int32_t kids[2] = {-1, -1};
    int nk = 0;
    for (int k = 0; k < 2; k++) {
      const uint32_t ref = k ? b.c1 : b.c0;
      if (ref == kEmptyChild) continue;
      const int32_t v = (int32_t)T.size();
      T.emplace_back();
      for (int a = 0; a < 3; a++) T[v].lo[a] = b.lo[a][k], T[v].hi[a] = b.hi[a][k];
      kids[nk++] = v;
      if (ref & kLeafBit) T[v].ref = map_leaf(ref), T[v].prims = (ref & 7u) + 1u, T[v].curve = (ref & kCurveBit) ? 1 : 0;
      else todo.push_back({ref, v});
    }
    // vertex t.v takes the node's children; a node with one child (a scene of one leaf) passes it through
    if (nk == 2) T[t.v].l = kids[0], T[t.v].r = kids[1];
    else if (nk == 1) T[t.v].l = kids[0], T[t.v].r = -1;
  }
  // the root's own box: the union of its children
  for (int a = 0; a < 3; a++) {
    T[0].lo[a] = std::numeric_limits<float>::infinity(), T[0].hi[a] = -T[0].lo[a];
    for (int32_t k : {T[0].l, T[0].r})
      if (k >= 0) T[0].lo[a] = std::min(T[0].lo[a], T[k].lo[a]), T[0].hi[a] = std::max(T[0].hi[a], T[k].hi[a]);
  }
}

// The cost of a flattened tree's programme: curve leaves anywhere mean the pricing per primitive.
QCost qcost_of_tree(const std::vector<QV>& T, const BvhBuildOptions& opt) {
  bool curves = false;
  double prim_area = 0.0;
  for (const QV& v : T)
    if (v.l < 0 && v.prims) curves = curves || (v.curve != 0), prim_area += leaf_prim_area(v.lo, v.hi, v.prims);
  return make_qcost(opt, curves, T.empty() ? 0.0 : half_area(T[0].lo, T[0].hi), prim_area);
}

// Which descendants become the (up to four) children of the Q node of a vertex v is chosen bottom-up over the surface-area
// cost, with the box a child really presents to a ray: its box rounded outwards on the 8-bit grid of v (step = extent of v /
// 253 ).  That looseness is what matters for thin primitives in big nodes -- a wall triangle of
// the Cornell box as a child of a node two units wide is a slab 0.016 thick, and every ray that starts on the wall tests it:
// with plain areas the collapse put such leaves high up and a shadow ray tested 2.7 triangles instead of 0.9.
//   below[v] = min over the frontiers F below v, |F| <= 4, of  sum_{u in F} term(u | v) + below[u]
//   term(u | v) = qarea(u | v) * kCostNode                                                   u inner: one node turn
//               = (qarea(u | v) + [slab] * C.surface * prim_area(u)) * kCostLeaf             u a triangle leaf: one TriPair, one turn
//   [slab]: the box of u on v's grid is thicker than u's own along u's thinnest axis by more than kSurfaceEps -- the rays that start
//   on u's primitives (tmin = kSurfaceEps) then pass the slab test and take the leaf's turn, whatever their direction; C.surface puts
//   their share (area of u's primitives / the scene's) into the units of qarea (probability of crossing * area of the root's box).
//   (QCost::per_prim -- the pricing of before, and of trees with curve leaves -- : a leaf is qarea * prims, a node qarea, nothing else.)
// A vertex has at most a dozen frontiers (each inner member may be replaced by its two children while there is room).
// One vertex of that programme: below[vi] and the chosen frontier choice[4 vi ..], from the values of the vertices under it.
void qdp_vertex(const std::vector<QV>& T, size_t vi, const QCost& C, std::vector<double>& below, std::vector<int32_t>& choice) {
  using V = QV;
  auto area = [](const V& v) {
    const float dx = v.hi[0] - v.lo[0], dy = v.hi[1] - v.lo[1], dz = v.hi[2] - v.lo[2];
    const float a = dx * dy + dy * dz + dz * dx;
    return a >= 0.f && std::isfinite(a) ? (double)a : 0.0;
  };
  auto qarea = [&](const V& u, const V& v, bool* slab) {
    double e[3];
    for (int a = 0; a < 3; a++) {
      const double ext = (double)v.hi[a] - (double)v.lo[a];
      const double st = std::max(ext / 253.0, 1e-37);
      const double ql = floor(((double)u.lo[a] - (double)v.lo[a]) / st), qh = ceil(((double)u.hi[a] - (double)v.lo[a]) / st);
      e[a] = std::max(qh - ql, 0.0) * st;
    }
    if (slab) {
      int thin = 0;
      for (int a = 1; a < 3; a++)
        if (u.hi[a] - u.lo[a] < u.hi[thin] - u.lo[thin]) thin = a;
      *slab = e[thin] - ((double)u.hi[thin] - (double)u.lo[thin]) > kSurfaceEps;
    }
    const double a = e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
    return std::isfinite(a) ? a : 0.0;
  };
  auto leaf_term = [&](const V& u, double qa, bool slab) {
    if (C.per_prim) return qa * C.leaf * u.prims;
    return (qa + (slab ? C.surface * leaf_prim_area(u.lo, u.hi, u.prims) : 0.0)) * C.leaf;
  };
  const V& v = T[vi];
  for (int m = 0; m < 4; m++) choice[vi * 4 + m] = -1;
  below[vi] = 0.0;
  if (v.l < 0) return;  // leaf: nothing below
  if (v.r < 0) {        // pass-through (the root of a scene with one leaf or one subtree)
    choice[vi * 4] = v.l;
    below[vi] = T[v.l].l < 0 ? leaf_term(T[v.l], area(T[v.l]), false) : area(T[v.l]) * C.node + below[v.l];
    return;
  }
  // enumerate the frontiers: start from {l, r}; replace inner members by their children while the size stays <= 4
  int32_t fronts[16][4];
  int sizes[16], nf = 0;
  fronts[0][0] = v.l, fronts[0][1] = v.r, sizes[0] = 2, nf = 1;
  for (int i = 0; i < nf && nf < 16; i++) {
    if (sizes[i] >= 4) continue;
    for (int m = 0; m < sizes[i] && nf < 16; m++) {
      const V& u = T[fronts[i][m]];
      if (u.l < 0 || u.r < 0) continue;
      int32_t g[4];
      int n = 0;
      for (int j = 0; j < sizes[i]; j++) {
        if (j == m) g[n++] = u.l, g[n++] = u.r;
        else g[n++] = fronts[i][j];
      }
      std::sort(g, g + n);
      bool dup = false;
      for (int q = 0; q < nf && !dup; q++) dup = sizes[q] == n && std::equal(g, g + n, fronts[q]);
      if (dup) continue;
      std::copy(g, g + n, fronts[nf]), sizes[nf] = n, nf++;
    }
  }
  // (the frontiers draw their members from at most 2 + 4 + 8 vertices: each one's term is worked out once)
  int32_t term_of[16];
  double term[16];
  int nt = 0;
  auto member = [&](int32_t ui) {
    for (int k = 0; k < nt; k++)
      if (term_of[k] == ui) return term[k];
    const V& u = T[ui];
    if (u.l < 0) {
      bool slab = false;
      const double qa = qarea(u, v, C.surface > 0.0 ? &slab : nullptr);
      term[nt] = leaf_term(u, qa, slab);
    } else {
      term[nt] = qarea(u, v, nullptr) * C.node + below[ui];
    }
    term_of[nt] = ui;
    return term[nt++];
  };
  double best = 1e300;
  int bi = 0;
  for (int i = 0; i < nf; i++) {
    double c = 0.0;
    for (int m = 0; m < sizes[i]; m++) c += member(fronts[i][m]);
    if (c < best) best = c, bi = i;
  }
  below[vi] = best;
  for (int m = 0; m < sizes[bi]; m++) choice[vi * 4 + m] = fronts[bi][m];
}

// The stack need of the Q node of vertex vi, from its chosen frontier and the needs of the vertices under it (build_qtree's definition).
uint32_t qdp_need(const std::vector<QV>& T, size_t vi, const std::vector<int32_t>& choice, const std::vector<uint32_t>& need) {
  uint32_t nc = 0, deepest = 0;
  for (int m = 0; m < 4; m++) {
    const int32_t u = choice[vi * 4 + m];
    if (u < 0) continue;
    nc++;
    if (T[u].l >= 0) deepest = std::max(deepest, need[u]);
  }
  return (nc ? nc - 1u : 0u) + deepest;
}


// Subtree re-insertion on the build-time tree.  A top-down split decides near the root with the least knowledge:
// a dozen wall triangles among half a million small ones end up in nodes that span the room.  A pass takes the largest nodes, one
// after the other, out of the tree and puts each back where the tree grows least; leaves move as they are (ranges, kinds and the
// order array never change).  What decides is what the Q collapse would pay for the tree, not the binary surface-area sum: that one
// keeps falling while the collapsed tree gets worse.  With the turn cost (host_scene.h::BvhBuildOptions) every move is decided on its
// own: the area growth only ranks the positions, the best few are priced by below[root] and the subtree goes where that is lowest, or
// back (place_by_cost).  With the pricing of before, or where the rays walk the binary tree, a pass is placed by area growth alone and
// kept or undone as a whole.  The pass-level guards -- binary depth and Q stack need within kStackDepth -- hold either way.
struct Reinserter {
  std::vector<TNode>& T;
  int32_t root;
  const BvhBuildOptions& opt;
  std::vector<int32_t> parent;
  // the collapse's programme per pool node: a move dirties the two paths from its ends to the root and nothing else
  std::vector<QV> qv;
  std::vector<double> below;
  std::vector<int32_t> choice;
  std::vector<uint32_t> need;
  std::vector<uint8_t> dirty;
  struct Move {
    int32_t n, sibling;  // n was taken from beside `sibling`
  };
  std::vector<Move> log;  // the moves of the running pass, for undoing it
  QCost C;                // what the programme charges
  uint32_t ntry = 0;      // positions priced per candidate; 0: a pass is placed by area growth alone and kept or undone as a whole
  double cur = 0.0;       // below[root] of the tree as it stands (ntry > 0)

  static Box unite(const Box& a, const Box& b) {
    Box u = a;
    u.grow(b);
    return u;
  }
  void replace_child(int32_t g, int32_t from, int32_t to) { (T[g].left == from ? T[g].left : T[g].right) = to; }
  // boxes upwards from i, each the exact union of its two children; above the first one that stays as it is nothing changes
  void refit_up(int32_t i) {
    for (; i >= 0; i = parent[i]) {
      const Box b = unite(T[T[i].left].box, T[T[i].right].box);
      if (memcmp(&b, &T[i].box, sizeof(Box)) == 0) break;
      T[i].box = b;
    }
  }
  void mark_up(int32_t i) {
    if (dirty.empty()) return;
    for (; i >= 0; i = parent[i]) dirty[i] = 1;
  }
  // n leaves the tree together with its parent p, whose other child takes p's place; returns p
  int32_t unlink(int32_t n) {
    const int32_t p = parent[n], g = parent[p], s = T[p].left == n ? T[p].right : T[p].left;
    parent[s] = g;
    if (g < 0) root = s;
    else replace_child(g, p, s), refit_up(g);
    return p;
  }
  // p, which holds n on one side, takes x's place and x on its other side
  void link(int32_t p, int32_t n, int32_t x) {
    const int32_t g = parent[x];
    (T[p].left == n ? T[p].right : T[p].left) = x;
    parent[x] = p, parent[p] = g;
    T[p].box = unite(T[x].box, T[n].box);
    if (g < 0) root = p;
    else replace_child(g, x, p), refit_up(g);
  }

  using Entry = std::pair<double, int32_t>;  // (area growth of the ancestors, node): the least first, ties to the lower index

  // n, unlinked from beside s with its parent p, goes where the collapse pays least: the (up to) ntry positions whose area growth is
  // the smallest and below `here`, that of where it was, are linked one after the other and priced by below[root] -- an evaluation
  // walks the two paths a link dirties -- and n ends at the cheapest, or back beside s when none is cheaper than `cur` (ties: where
  // it was, then the smaller growth, then the lower index).  A position that takes the Q stack need beyond the stack is no position.
  // Returns 1 when n has moved.
  uint32_t place_by_cost(int32_t p, int32_t n, int32_t s, const Box& nb, double an, double here, std::vector<Entry>& heap) {
    Entry top[kMaxReinsertTry];  // (total growth, position), ascending
    uint32_t nt = 0;
    double bound = here;
    heap.clear();
    heap.push_back({0.0, root});
    while (!heap.empty()) {
      std::pop_heap(heap.begin(), heap.end(), std::greater<Entry>());
      const Entry e = heap.back();
      heap.pop_back();
      if (!(e.first + an < bound)) break;
      const int32_t x = e.second;
      const double total = e.first + (double)unite(T[x].box, nb).area();
      if (total < bound && x != s) {
        if (nt < ntry) nt++;
        uint32_t k = nt - 1;
        for (; k > 0 && Entry(total, x) < top[k - 1]; k--) top[k] = top[k - 1];
        top[k] = {total, x};
        if (nt == ntry) bound = top[nt - 1].first;
      }
      const double grown = total - (double)T[x].box.area();
      if (T[x].left >= 0 && grown + an < bound) {
        heap.push_back({grown, T[x].left}), std::push_heap(heap.begin(), heap.end(), std::greater<Entry>());
        heap.push_back({grown, T[x].right}), std::push_heap(heap.begin(), heap.end(), std::greater<Entry>());
      }
    }
    if (nt == 0) {
      link(p, n, s);  // (back where it was: the boxes are the same unions again, nothing is dirty)
      return 0;
    }
    mark_up(parent[s]);
    double best_c = cur;
    int32_t bx = s;
    for (uint32_t k = 0; k < nt; k++) {
      link(p, n, top[k].second);
      mark_up(p);
      const double c = evaluate();
      if (c < best_c && need[root] <= (uint32_t)kStackDepth) best_c = c, bx = top[k].second;
      unlink(n);
      mark_up(parent[top[k].second]);
    }
    link(p, n, bx);
    mark_up(p);
    cur = evaluate();
    if (bx == s) return 0;
    log.push_back({n, s});
    return 1;
  }

  // One pass over the opt.reinsert_top largest nodes, in descending order of area (ties: the lower index).  Returns the moves made.
  uint32_t pass() {
    std::vector<std::pair<float, int32_t>> cand;
    cand.reserve(T.size());
    for (int32_t i = 0; i < (int32_t)T.size(); i++)
      if (i != root && parent[i] != root) cand.push_back({T[i].box.area(), i});
    const size_t K = std::min<size_t>(opt.reinsert_top, cand.size());
    auto larger = [](const std::pair<float, int32_t>& a, const std::pair<float, int32_t>& b) {
      return a.first > b.first || (a.first == b.first && a.second < b.second);
    };
    if (K < cand.size()) std::nth_element(cand.begin(), cand.begin() + (ptrdiff_t)K, cand.end(), larger);
    std::sort(cand.begin(), cand.begin() + (ptrdiff_t)K, larger);
    std::vector<Entry> heap;
    uint32_t moves = 0;
    for (size_t c = 0; c < K; c++) {
      const int32_t n = cand[c].second;
      if (n == root || parent[n] == root) continue;  // (an earlier move of this pass put it there)
      const int32_t s = T[parent[n]].left == n ? T[parent[n]].right : T[parent[n]].left;
      const int32_t p = unlink(n);
      const Box nb = T[n].box;
      const double an = nb.area();
      // where it was: the position to beat
      double best = unite(T[s].box, nb).area();
      for (int32_t a = parent[s]; a >= 0; a = parent[a]) best += (double)unite(T[a].box, nb).area() - (double)T[a].box.area();
      if (ntry > 0) {
        moves += place_by_cost(p, n, s, nb, an, best, heap);
        continue;
      }
      int32_t bx = s;
      // best first from the root; a subtree whose ancestors alone grow by as much as the best position costs is left out
      heap.clear();
      heap.push_back({0.0, root});
      while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), std::greater<Entry>());
        const Entry e = heap.back();
        heap.pop_back();
        if (!(e.first + an < best)) break;
        const int32_t x = e.second;
        const double total = e.first + (double)unite(T[x].box, nb).area();
        if (total < best) best = total, bx = x;
        const double grown = total - (double)T[x].box.area();
        if (T[x].left >= 0 && grown + an < best) {
          heap.push_back({grown, T[x].left}), std::push_heap(heap.begin(), heap.end(), std::greater<Entry>());
          heap.push_back({grown, T[x].right}), std::push_heap(heap.begin(), heap.end(), std::greater<Entry>());
        }
      }
      const int32_t g = parent[s];
      link(p, n, bx);
      if (bx == s) continue;  // (back where it was: the boxes are the same unions again)
      mark_up(g), mark_up(p);
      log.push_back({n, s});
      moves++;
    }
    return moves;
  }
  void undo_pass() {
    for (size_t i = log.size(); i-- > 0;) link(unlink(log[i].n), log[i].n, log[i].sibling);
    log.clear();
  }

  // below[root] of the collapse's programme: the vertices a move has dirtied, children first
  double evaluate() {
    std::vector<int32_t> todo{root}, pre;
    while (!todo.empty()) {
      const int32_t i = todo.back();
      todo.pop_back();
      if (!dirty[i]) continue;
      pre.push_back(i);
      if (T[i].left >= 0) todo.push_back(T[i].left), todo.push_back(T[i].right);
    }
    for (size_t k = pre.size(); k-- > 0;) {
      const int32_t i = pre[k];
      const TNode& t = T[i];
      QV& q = qv[i];
      for (int a = 0; a < 3; a++) q.lo[a] = BvhNode::widen_lo(t.box.lo[a]), q.hi[a] = BvhNode::widen_hi(t.box.hi[a]);  // (the boxes the flattened tree stores)
      q.l = t.left, q.r = t.right, q.prims = t.left < 0 ? t.count : 0u;
      qdp_vertex(qv, (size_t)i, C, below, choice);
      need[i] = qdp_need(qv, (size_t)i, choice, need);
      dirty[i] = 0;
    }
    return below[root];
  }
  double inner_area() const {  // the binary tree's surface-area sum (every pool node is in the tree)
    double sum = 0.0;
    for (const TNode& t : T)
      if (t.left >= 0) sum += (double)t.box.area();
    return sum;
  }
  // TNode::depth of every node; returns the deepest inner node's (what the flattened tree reports: FlatBvh::depth)
  uint32_t set_depths() {
    uint32_t deepest = 0;
    std::vector<int32_t> todo{root};
    T[root].depth = 1;
    while (!todo.empty()) {
      const int32_t i = todo.back();
      todo.pop_back();
      if (T[i].left < 0) continue;
      deepest = std::max(deepest, T[i].depth);
      T[T[i].left].depth = T[T[i].right].depth = T[i].depth + 1;
      todo.push_back(T[i].left), todo.push_back(T[i].right);
    }
    return deepest;
  }

  void run(FlatBvh* out) {
    if (T[root].left < 0) return;
    parent.assign(T.size(), -1);
    for (int32_t i = 0; i < (int32_t)T.size(); i++)
      if (T[i].left >= 0) parent[T[i].left] = parent[T[i].right] = i;
    bool by_q = opt.for_qtree;
    double cost = 0.0;
    if (by_q) {
      // (the root's box and the leaves never change: the surface term's scale is the one qtree_cost and build_qtree work out)
      float rlo[3], rhi[3];
      for (int a = 0; a < 3; a++) rlo[a] = BvhNode::widen_lo(T[root].box.lo[a]), rhi[a] = BvhNode::widen_hi(T[root].box.hi[a]);
      double prim_area = 0.0;
      for (const TNode& t : T)
        if (t.left < 0) {
          float lo[3], hi[3];
          for (int a = 0; a < 3; a++) lo[a] = BvhNode::widen_lo(t.box.lo[a]), hi[a] = BvhNode::widen_hi(t.box.hi[a]);
          prim_area += leaf_prim_area(lo, hi, t.count);
        }
      C = make_qcost(opt, false, half_area(rlo, rhi), prim_area);
      qv.resize(T.size()), below.assign(T.size(), 0.0), choice.assign(T.size() * 4, -1), need.assign(T.size(), 0u), dirty.assign(T.size(), 1);
      cost = evaluate();
      by_q = need[root] <= (uint32_t)kStackDepth;  // (a Q tree that is dropped anyway: the binary tree is what gets walked)
      if (!by_q) dirty.clear();
      else if (opt.cost != kBvhCostPrims) ntry = std::min(opt.reinsert_try, kMaxReinsertTry);
      cur = cost;
    }
    if (!by_q) cost = inner_area();
    out->reinsert_cost0 = out->reinsert_cost = cost;
    for (uint32_t k = 0; k < opt.reinsert_passes; k++) {
      const uint32_t moves = pass();
      if (moves == 0) break;
      const double c = by_q ? evaluate() : inner_area();  // (moves priced one by one: nothing is dirty, this is `cur`)
      const bool fits = set_depths() <= (uint32_t)kStackDepth && (!by_q || need[root] <= (uint32_t)kStackDepth);
      if (!(c < cost) || !fits) {  // the first pass that does not pay, or that the traversal stack cannot hold, is taken back
        undo_pass();
        break;
      }
      log.clear();
      cost = c;
      out->reinsert_cost = c, out->reinsert_passes++, out->reinsert_moves += moves;
    }
    set_depths();
  }
};

}  // namespace

void build_bvh(const std::vector<float>& lo, const std::vector<float>& hi, const std::vector<uint8_t>& kinds,
               FlatBvh* out, const BvhBuildOptions& opt) {
  *out = FlatBvh();
  uint32_t n = (uint32_t)kinds.size();
  if (n == 0) return;
  Builder b;
  b.lo = lo.data(), b.hi = hi.data(), b.kinds = kinds.data();
  b.cen.resize(3 * (size_t)n);
  b.order.resize(n);
  for (uint32_t g = 0; g < n; g++) {
    for (int a = 0; a < 3; a++) b.cen[3 * g + a] = 0.5f * (lo[3 * g + a] + hi[3 * g + a]);
    b.order[g] = g;
  }
  Builder::Pool pool;
  pool.nodes.reserve(2 * (size_t)n / 2 + 16);
  const auto t_build = std::chrono::steady_clock::now();
  int32_t root = b.build(pool, 0, n, 1);
  const auto t_reinsert = std::chrono::steady_clock::now();
  out->build_ms = std::chrono::duration<double, std::milli>(t_reinsert - t_build).count();
  // (triangle-only scenes: a tree with curve leaves stays as the builder left it -- host_scene.h::BvhBuildOptions)
  if (opt.reinsert_passes > 0 && opt.reinsert_top > 0 && std::all_of(kinds.begin(), kinds.end(), [](uint8_t kd) { return kd == 0; })) {
    Reinserter re{pool.nodes, root, opt};
    re.run(out);
    root = re.root;
    out->reinsert_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_reinsert).count();
  }

  // flatten: internal nodes get consecutive indices; node 0 is always internal
  const std::vector<TNode>& T = pool.nodes;
  const float kNaN3[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::quiet_NaN(),
                          std::numeric_limits<float>::quiet_NaN()};
  std::vector<BvhNode>& N = out->nodes;
  uint32_t depth = 0;
  if (T[root].left < 0) {
    BvhNode nd;
    memset(&nd, 0, sizeof(nd));
    nd.set_box(0, T[root].box.lo, T[root].box.hi);
    nd.set_box(1, kNaN3, kNaN3);
    nd.c0 = leaf_ref(T[root]);
    nd.c1 = kEmptyChild;
    N.push_back(nd);
    depth = 1;
  } else {
    struct Item {
      int32_t t;
      uint32_t out;
    };
    // Numbering: breadth first for the first kTopNodes nodes (the top of the tree is one contiguous block that the
    // traversal kernel copies into LDS: dscene.h), depth first below
    std::deque<Item> work;
    N.emplace_back();
    work.push_back({root, 0});
    while (!work.empty()) {
      Item it;
      if (N.size() < (size_t)kTopNodes) it = work.front(), work.pop_front();
      else it = work.back(), work.pop_back();
      const TNode& t = T[it.t];
      depth = std::max(depth, t.depth);
      BvhNode nd;
      memset(&nd, 0, sizeof(nd));
      const TNode &l = T[t.left], &r = T[t.right];
      nd.set_box(0, l.box.lo, l.box.hi);
      nd.set_box(1, r.box.lo, r.box.hi);
      if (l.left < 0) {
        nd.c0 = leaf_ref(l);
      } else {
        nd.c0 = (uint32_t)N.size();
        N.emplace_back();
        work.push_back({t.left, nd.c0});
      }
      if (r.left < 0) {
        nd.c1 = leaf_ref(r);
      } else {
        nd.c1 = (uint32_t)N.size();
        N.emplace_back();
        work.push_back({t.right, nd.c1});
      }
      N[it.out] = nd;
    }
  }
  out->slot_gid = b.order;
  out->depth = depth;
}

// (the quantiser of a node -- quantise_node -- is qquant.h's: the collapse on the device, qtree_gpu.hip, shares it)

// The exact stack need of a near-first traversal of a Q tree: the maximum over root-to-leaf paths of the sum of (children - 1).
// need(node) = (children - 1) + max over inner children need(child); children need not follow their parent, so: depth first
uint32_t qtree_stack_need(const std::vector<QNode>& N) {
  if (N.empty()) return 0;
  std::vector<uint32_t> need(N.size(), 0);
  std::vector<uint8_t> state(N.size(), 0);  // 0 new, 1 open, 2 done
  std::vector<uint32_t> todo{0u};
  while (!todo.empty()) {
    const uint32_t i = todo.back();
    const QNode& nd = N[i];
    if (state[i] == 0) {
      state[i] = 1;
      for (int k = 0; k < 4; k++)
        if (!(nd.c[k] & kLeafBit) && nd.c[k] < N.size() && state[nd.c[k]] == 0) todo.push_back(nd.c[k]);
      continue;
    }
    todo.pop_back();
    if (state[i] == 2) continue;
    state[i] = 2;
    uint32_t nc = 0, deepest = 0;
    for (int k = 0; k < 4; k++) {
      if (nd.c[k] == kEmptyChild) continue;
      nc++;
      if (!(nd.c[k] & kLeafBit) && nd.c[k] < N.size()) deepest = std::max(deepest, need[nd.c[k]]);
    }
    need[i] = (nc ? nc - 1u : 0u) + deepest;
  }
  return need[0];
}

double qtree_cost(const std::vector<BvhNode>& N2, uint32_t* stack_need, const BvhBuildOptions& opt) {
  if (stack_need) *stack_need = 0;
  if (N2.empty()) return 0.0;
  std::vector<QV> T;
  qv_of_nodes(N2, [](uint32_t ref) { return ref; }, &T);
  const QCost C = qcost_of_tree(T, opt);
  const size_t nv = T.size();
  std::vector<double> below(nv, 0.0);
  std::vector<int32_t> choice(nv * 4, -1);
  std::vector<uint32_t> need(nv, 0u);
  for (size_t vi = nv; vi-- > 0;) {  // (children follow their parent)
    qdp_vertex(T, vi, C, below, choice);
    need[vi] = qdp_need(T, vi, choice, need);
  }
  // (a pass-through root whose only child is inner gets a node of its own under the root's: one child, nothing left behind)
  if (stack_need) *stack_need = need[0];
  return below[0];
}

uint32_t build_qtree(const std::vector<BvhNode>& N2, const std::function<uint32_t(uint32_t)>& map_leaf, std::vector<QNode>* out,
                     const BvhBuildOptions& opt) {
  out->clear();
  if (N2.empty()) return 0;
  using V = QV;
  std::vector<V> T;
  qv_of_nodes(N2, map_leaf, &T);
  const QCost C = qcost_of_tree(T, opt);
  const size_t nv = T.size();
  std::vector<double> below(nv, 0.0);
  std::vector<int32_t> choice(nv * 4, -1);  // the chosen frontier of v
  for (size_t vi = nv; vi-- > 0;) qdp_vertex(T, vi, C, below, choice);
  // emit: the Q node of vertex v has its chosen frontier as children
  struct Item {
    int32_t v;
    uint32_t out;
  };
  // numbering: breadth first for the first kTopNodes nodes (the top of the tree is one contiguous block that the traversal
  // kernel of triangle-only scenes copies into LDS: dscene.h), depth first below; a node's inner children get consecutive numbers
  std::deque<Item> work;
  out->emplace_back();
  work.push_back({0, 0u});
  while (!work.empty()) {
    Item it;
    if (out->size() < (size_t)kTopNodes) it = work.front(), work.pop_front();
    else it = work.back(), work.pop_back();
    int32_t fr[4];
    int n = 0;
    if (T[it.v].l < 0) {
      fr[n++] = it.v;  // (a scene of one leaf: the root node holds it)
    } else {
      for (int m = 0; m < 4; m++)
        if (choice[(size_t)it.v * 4 + m] >= 0) fr[n++] = choice[(size_t)it.v * 4 + m];
      // (a pass-through vertex hands on its only child; if that child is inner it gets a node of its own below)
    }
    QBox c[4];
    for (int i = 0; i < n; i++)
      for (int a = 0; a < 3; a++) c[i].lo[a] = T[fr[i]].lo[a], c[i].hi[a] = T[fr[i]].hi[a];
    QNode nd;
    if (n == 0 || !quantise_node(c, n, &nd)) {
      out->clear();
      return 0;
    }
    for (int i = 0; i < 4; i++) nd.c[i] = kEmptyChild;
    for (int i = 0; i < n; i++) {
      const V& u = T[fr[i]];
      if (u.l < 0) {
        nd.c[i] = u.ref;
      } else {
        const uint32_t id = (uint32_t)out->size();
        out->emplace_back();
        nd.c[i] = id;
        work.push_back({fr[i], id});
      }
    }
    (*out)[it.out] = nd;
  }
  // the stack a near-first traversal can need: on the way down every node leaves at most (children - 1) entries behind
  return qtree_stack_need(*out);
}

void build_qlayout(const FlatBvh& bvh, const std::vector<float4>& slots, const std::vector<uint8_t>& kinds, QLayout* out,
                   const BvhBuildOptions& opt) {
  static_assert(kMaxLeaf <= 2, "a leaf of the binary tree becomes one TriPair / one curve record");
  *out = QLayout();
  std::vector<float4>&qtri = out->tri, &qpts = out->pts;
  std::vector<uint32_t>& qhit = out->hit;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  // the complete hit code of slot k: k | routing bits
  auto code = [&](uint32_t k) { return k | __builtin_bit_cast(uint32_t, slots[4 * (size_t)k + 2].w); };
  // Triangle leaves.  Triangle-only scenes: one TriPair per leaf (dscene.h): its one or two triangles interleaved coordinate by
  // coordinate, 80 bytes, both tested at once on packed fp32.  Scenes with curves (their kernels have no registers to spare
  // and meet triangles rarely): 48 bytes per triangle -- three corners, the hit code in the third word's .w -- one after the other.
  const bool tri_pairs = std::all_of(kinds.begin(), kinds.end(), [](uint8_t kd) { return kd == 0; });
  auto tri_leaf = [&](uint32_t first, uint32_t count) -> uint32_t {
    if (!tri_pairs) {
      const uint32_t rec = (uint32_t)(qtri.size() / 3);
      for (uint32_t i = 0; i < count; i++) {
        for (int c = 0; c < 3; c++) qtri.push_back(slots[4 * (size_t)(first + i) + c]);
        qtri.back().w = __builtin_bit_cast(float, code(first + i));
      }
      return rec;
    }
    const uint32_t rec = (uint32_t)(qtri.size() / kTriPairWords);
    const float4* a = &slots[4 * (size_t)first];
    const float4* b = count == 2 ? &slots[4 * (size_t)(first + 1)] : a;  // (one triangle: stored twice, the copy is no candidate)
    const float ca = __builtin_bit_cast(float, code(first)), cb = __builtin_bit_cast(float, count == 2 ? code(first + 1) : kNone);
    qtri.insert(qtri.end(), {make_float4(a[0].x, b[0].x, a[0].y, b[0].y), make_float4(a[0].z, b[0].z, a[1].x, b[1].x),
                             make_float4(a[1].y, b[1].y, a[1].z, b[1].z), make_float4(a[2].x, b[2].x, a[2].y, b[2].y),
                             make_float4(a[2].z, b[2].z, ca, cb)});
    return rec;
  };
  // Curve leaves: a record (dscene.h) of the end points of the leaf's one or two pieces, at a point index P that is a multiple
  // of 4.  Points 0..3 stay zero: the first record is at point 4.
  qpts.assign(4, zero);
  qhit.assign(4, kNone);
  auto curve_leaf = [&](uint32_t first, uint32_t count) -> uint32_t {
    while (qpts.size() % 4) qpts.push_back(zero);
    const uint32_t P = (uint32_t)qpts.size();
    uint32_t sub[2] = {0u, 0u};
    for (uint32_t i = 0; i < count; i++) {
      const float4* sl = &slots[4 * (size_t)(first + i)];  // (a piece's slot of the binary tree: its two end points, then its index in the cubic)
      qpts.push_back(sl[0]), qpts.push_back(sl[1]);
      sub[i] = __builtin_bit_cast(uint32_t, sl[2].x) & 3u;
    }
    qhit.resize(qpts.size(), kNone);
    qhit[P] = code(first);
    if (count == 2) qhit[P + 2] = code(first + 1);
    (count == 2 ? out->leaves_pair : out->leaves_one)++;
    return kLeafBit | kCurveBit | ((P | sub[0]) << 3) | (count == 2 ? (kCurvePairBit | sub[1]) : 0u);
  };
  auto map_leaf = [&](uint32_t ref) -> uint32_t {
    const uint32_t first = (ref & 0x3FFFFFFFu) >> 3, count = (ref & 7u) + 1u;
    if (ref & kCurveBit) return curve_leaf(first, count);
    return kLeafBit | (tri_leaf(first, count) << 3) | (count - 1u);
  };
  // (a tree the traversal stack cannot hold, or with point indices beyond the reference's 27 bits, is dropped: no Q tree)
  out->stack_need = build_qtree(bvh.nodes, map_leaf, &out->nodes, opt);
  if (out->stack_need > (uint32_t)kStackDepth || qpts.size() >= (1u << 27)) out->nodes.clear();
  while (qtri.size() % 4) qtri.push_back(zero);    // (q_pt0 a multiple of 4: the low bits of a curve record's address are free)
  for (int k = 0; k < 4; k++) qpts.push_back(zero);  // (the load site reads four words of a leaf)
  qhit.resize(qpts.size(), kNone);
}

std::vector<SssEntry> build_sss_entries(const std::vector<QNode>& wide, const std::vector<float>& ilo, const std::vector<float>& ihi,
                                        uint32_t max_foreign) {
  const size_t ninst = ilo.size() / 3;
  std::vector<SssEntry> entries(ninst, SssEntry{});
  struct CutRef { uint32_t ref; float lo[3], hi[3]; };
  for (size_t i = 0; i < ninst; i++) {
    SssEntry& E = entries[i];
    if (!(ilo[3 * i] <= ihi[3 * i])) continue;  // (no primitive)
    float ext = 0.f;
    for (int a = 0; a < 3; a++) ext = std::max(ext, ihi[3 * i + a] - ilo[3 * i + a]);
    if (!(ext > 0.f) || !std::isfinite(ext)) continue;
    const float m1 = 1e-4f * ext, m2 = 2e-3f * ext;  // the region rays may stay in / how far beyond it a primitive's box can matter
    float rlo[3], rhi[3], wlo[3], whi[3];
    for (int a = 0; a < 3; a++) rlo[a] = ilo[3 * i + a] - m1, rhi[a] = ihi[3 * i + a] + m1, wlo[a] = rlo[a] - m2, whi[a] = rhi[a] + m2;
    std::vector<CutRef> cut{{0u, {-INFINITY, -INFINITY, -INFINITY}, {INFINITY, INFINITY, INFINITY}}};
    for (bool changed = true; changed;) {
      changed = false;
      for (size_t c = 0; c < cut.size() && !changed; c++) {
        if (cut[c].ref & kLeafBit) continue;
        const QNode& nd = wide[cut[c].ref];
        const float org[3] = {nd.org[0], nd.org[1], nd.org[2]}, st3[3] = {nd.sx, nd.sy, nd.sz};
        const uint32_t ql[3] = {nd.qlo_x, nd.qlo_y, nd.qlo_z}, qh[3] = {nd.qhi_x, nd.qhi_y, nd.qhi_z};
        std::vector<CutRef> kids;
        int nchild = 0;
        for (int k = 0; k < 4; k++) {
          if (nd.c[k] == kEmptyChild) continue;
          nchild++;
          CutRef r;
          r.ref = nd.c[k];
          bool meets = true;
          for (int a = 0; a < 3; a++) {  // the box the traversal rebuilds for this child (dtrace.h::box_test4q): fma(q, s, org)
            r.lo[a] = fmaf((float)((ql[a] >> (8 * k)) & 255u), st3[a], org[a]);
            r.hi[a] = fmaf((float)((qh[a] >> (8 * k)) & 255u), st3[a], org[a]);
            meets = meets && r.lo[a] <= whi[a] && r.hi[a] >= wlo[a];
          }
          if (meets) kids.push_back(r);
        }
        // descend where that drops a child (or leads to an only child), while the cut stays small
        if (((int)kids.size() < nchild || kids.size() == 1) && cut.size() - 1 + kids.size() <= 1u + max_foreign) {
          cut.erase(cut.begin() + (ptrdiff_t)c);
          cut.insert(cut.end(), kids.begin(), kids.end());
          changed = true;
        }
      }
    }
    // the entry: the inner node of the cut that shares the most volume with the instance's bounds
    int best = -1;
    double best_v = -1.0;
    for (size_t c = 0; c < cut.size(); c++) {
      if (cut[c].ref & kLeafBit) continue;
      double v = 1.0;
      for (int a = 0; a < 3; a++) v *= std::max(0.0, (double)std::min(cut[c].hi[a], ihi[3 * i + a]) - (double)std::max(cut[c].lo[a], ilo[3 * i + a]));
      if (v > best_v) best_v = v, best = (int)c;
    }
    if (best < 0 || cut[(size_t)best].ref == 0u) continue;  // (the root, or leaves only: start at the root)
    E.entry = cut[(size_t)best].ref;
    for (int a = 0; a < 3; a++) E.lo[a] = rlo[a], E.hi[a] = rhi[a];
    for (size_t c = 0; c < cut.size(); c++) {
      if ((int)c == best) continue;
      auto& f = E.foreign[E.nforeign++];
      f.ref = cut[c].ref;
      for (int a = 0; a < 3; a++) f.lo[a] = cut[c].lo[a], f.hi[a] = cut[c].hi[a];
    }
  }
  return entries;
}

}  // namespace pb
