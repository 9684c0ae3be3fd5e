// The host builder's subtree re-insertion (pbrlab_amd/csrc/bvh_build.cpp: build_bvh with BvhBuildOptions::reinsert_passes) on small and
// degenerate primitive sets and, given a file of boxes (uint32 n, 3n floats lo, 3n floats hi, n bytes kinds) and optionally the number of
// candidates per pass, on a scene.  For every
// set the tree is built with the passes off and on and checked: every primitive in exactly one leaf, the same leaves as the
// builder's own tree, every stored box the widened exact union of what is below it, the reported depth, two builds byte-identical,
// no passes == the plain call, a set with curves == the builder's tree, and the collapse's cost not above the builder's tree's.  For the file the Q tree is collapsed from
// either tree and a fixed set of rays is walked near first through it: node and leaf visits per ray are printed.
// tests/test_bvh_reinsert_cpu.py builds and runs this (once more under ASan/UBSan) and asserts on the printed lines.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "host_scene.h"
using namespace pb;

static uint64_t rng_state;
static float rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((rng_state >> 40) & 0xFFFFFF) / 16777216.0f;
}

struct Set {
  std::vector<float> lo, hi;
  std::vector<uint8_t> kinds;
  void add(const float* c, const float* h, uint8_t kind) {
    for (int a = 0; a < 3; a++) lo.push_back(c[a] - h[a]), hi.push_back(c[a] + h[a]);
    kinds.push_back(kind);
  }
};

using Leaf = std::pair<int, std::vector<uint32_t>>;  // kind, sorted primitives

// Walks the flattened tree.  Returns false (with a message) when an invariant does not hold.
static bool check_tree(const char* name, const Set& s, const FlatBvh& b, std::vector<Leaf>* leaves) {
  const uint32_t n = (uint32_t)s.kinds.size();
  if (b.slot_gid.size() != n) return printf("FAIL %s: slot count\n", name), false;
  std::vector<int> seen(n, 0);
  for (uint32_t g : b.slot_gid)
    if (g >= n || seen[g]++) return printf("FAIL %s: slot permutation\n", name), false;
  std::vector<int> in_leaf(n, 0);
  // the tight box below a child, children first: post-order with an explicit stack
  struct Fr {
    uint32_t node, depth;
    int state;
    float lo[2][3], hi[2][3];
  };
  std::vector<Fr> st;
  std::vector<int> visited(b.nodes.size(), 0);
  uint32_t deepest = 0;
  float rlo[3], rhi[3];  // what the last finished frame hands to its parent
  auto open = [&](uint32_t node, uint32_t depth) {
    Fr f;
    memset(&f, 0, sizeof(f));
    f.node = node, f.depth = depth, f.state = 0;
    st.push_back(f);
  };
  open(0, 1);
  while (!st.empty()) {
    Fr& f = st.back();
    if (f.node >= b.nodes.size()) return printf("FAIL %s: node index\n", name), false;
    const BvhNode& nd = b.nodes[f.node];
    if (f.state == 0) {
      if (visited[f.node]++) return printf("FAIL %s: node visited twice\n", name), false;
      deepest = std::max(deepest, f.depth);
    }
    if (f.state >= 1 && f.state <= 2 && !(((f.state == 1 ? nd.c0 : nd.c1) & kLeafBit))) {  // an inner child has just finished
      memcpy(f.lo[f.state - 1], rlo, 12), memcpy(f.hi[f.state - 1], rhi, 12);
    }
    if (f.state < 2) {
      const int c = f.state++;
      const uint32_t ref = c ? nd.c1 : nd.c0;
      if (ref == kEmptyChild) {
        if (!(c == 1 && n <= (uint32_t)kMaxLeaf)) return printf("FAIL %s: empty child\n", name), false;
        for (int a = 0; a < 3; a++) f.lo[c][a] = INFINITY, f.hi[c][a] = -INFINITY;
        continue;
      }
      if (ref & kLeafBit) {
        const uint32_t first = (ref & 0x3FFFFFFFu) >> 3, cnt = (ref & 7u) + 1u;
        if (first + cnt > n || cnt > (uint32_t)kMaxLeaf) return printf("FAIL %s: leaf range\n", name), false;
        Leaf lf;
        lf.first = (ref & kCurveBit) ? 1 : 0;
        for (int a = 0; a < 3; a++) f.lo[c][a] = INFINITY, f.hi[c][a] = -INFINITY;
        for (uint32_t k = first; k < first + cnt; k++) {
          const uint32_t g = b.slot_gid[k];
          if ((s.kinds[g] != 0) != (lf.first != 0)) return printf("FAIL %s: leaf kind\n", name), false;
          if (in_leaf[g]++) return printf("FAIL %s: primitive %u in two leaves\n", name, g), false;
          lf.second.push_back(g);
          for (int a = 0; a < 3; a++) f.lo[c][a] = std::min(f.lo[c][a], s.lo[3 * g + a]), f.hi[c][a] = std::max(f.hi[c][a], s.hi[3 * g + a]);
        }
        std::sort(lf.second.begin(), lf.second.end());
        leaves->push_back(lf);
      } else {
        const uint32_t d = f.depth + 1;
        open(ref, d);  // (invalidates f)
      }
      continue;
    }
    // both children known: the stored boxes are their exact unions, widened
    for (int c = 0; c < 2; c++) {
      if ((c ? nd.c1 : nd.c0) == kEmptyChild) continue;
      for (int a = 0; a < 3; a++) {
        const float wl = BvhNode::widen_lo(f.lo[c][a]), wh = BvhNode::widen_hi(f.hi[c][a]);
        if (memcmp(&wl, &nd.lo[a][c], 4) || memcmp(&wh, &nd.hi[a][c], 4)) return printf("FAIL %s: node %u child %d axis %d: stored box is not the widened union\n", name, f.node, c, a), false;
      }
    }
    for (int a = 0; a < 3; a++) rlo[a] = std::min(f.lo[0][a], f.lo[1][a]), rhi[a] = std::max(f.hi[0][a], f.hi[1][a]);
    st.pop_back();
  }
  for (uint32_t g = 0; g < n; g++)
    if (in_leaf[g] != 1) return printf("FAIL %s: primitive %u in %d leaves\n", name, g, in_leaf[g]), false;
  for (int v : visited)
    if (v != 1) return printf("FAIL %s: unreachable node\n", name), false;
  if (b.depth != deepest) return printf("FAIL %s: depth %u reported, %u found\n", name, b.depth, deepest), false;
  if (b.depth > (uint32_t)kStackDepth) return printf("FAIL %s: depth %u beyond the stack\n", name, b.depth), false;
  std::sort(leaves->begin(), leaves->end());
  return true;
}

static bool same_bytes(const FlatBvh& a, const FlatBvh& b) {
  return a.depth == b.depth && a.nodes.size() == b.nodes.size() && a.slot_gid == b.slot_gid &&
         (a.nodes.empty() || memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(BvhNode)) == 0);
}

struct Built {
  FlatBvh off, on;
  double cost_off = 0.0, cost_on = 0.0;
  uint32_t need_off = 0, need_on = 0;
};

static bool run_set(const char* name, const Set& s, uint32_t top, Built* out) {
  BvhBuildOptions on;
  on.reinsert_passes = kReinsertPasses, on.reinsert_top = top;
  FlatBvh plain, again;
  build_bvh(s.lo, s.hi, s.kinds, &plain);
  build_bvh(s.lo, s.hi, s.kinds, &out->off, BvhBuildOptions());
  build_bvh(s.lo, s.hi, s.kinds, &out->on, on);
  build_bvh(s.lo, s.hi, s.kinds, &again, on);
  if (!same_bytes(plain, out->off)) return printf("FAIL %s: no passes is not the plain call's tree\n", name), false;
  if (!same_bytes(out->on, again)) return printf("FAIL %s: two builds differ\n", name), false;
  if (out->off.reinsert_passes || out->off.reinsert_moves) return printf("FAIL %s: passes reported with the option off\n", name), false;
  const bool curves = std::any_of(s.kinds.begin(), s.kinds.end(), [](uint8_t kd) { return kd != 0; });
  if (curves && (out->on.reinsert_passes || !same_bytes(out->on, out->off))) return printf("FAIL %s: a set with curves does not keep the builder's tree\n", name), false;
  std::vector<Leaf> l_off, l_on;
  if (!check_tree(name, s, out->off, &l_off) || !check_tree(name, s, out->on, &l_on)) return false;
  if (l_off != l_on) return printf("FAIL %s: the leaves changed\n", name), false;
  out->cost_off = qtree_cost(out->off.nodes, &out->need_off), out->cost_on = qtree_cost(out->on.nodes, &out->need_on);
  if (!(out->cost_on <= out->cost_off)) return printf("FAIL %s: collapse cost %.9g with the passes, %.9g without\n", name, out->cost_on, out->cost_off), false;
  if (out->need_off <= (uint32_t)kStackDepth && out->need_on > (uint32_t)kStackDepth) return printf("FAIL %s: Q stack need %u beyond the stack\n", name, out->need_on), false;
  printf("set %s n %zu passes %u moves %u cost_off %.9g cost_on %.9g depth_off %u depth_on %u need_off %u need_on %u\n", name, s.kinds.size(),
         out->on.reinsert_passes, out->on.reinsert_moves, out->cost_off, out->cost_on, out->off.depth, out->on.depth, out->need_off, out->need_on);
  return true;
}

// ---- the near-first walk of the Q tree, primitives taken as their boxes
struct Ray {
  float org[3], dir[3], tmax;
  uint32_t skip;  // the primitive the ray starts on
};
static bool slab(const float* lo, const float* hi, const Ray& r, float tmax, float* tnear) {
  float t0 = 0.f, t1 = tmax;
  for (int a = 0; a < 3; a++) {
    const float inv = 1.f / r.dir[a];
    float ta = (lo[a] - r.org[a]) * inv, tb = (hi[a] - r.org[a]) * inv;
    if (ta > tb) std::swap(ta, tb);
    if (ta > t0) t0 = ta;  // (a NaN -- origin on a face of a flat slab -- constrains nothing)
    if (tb < t1) t1 = tb;
  }
  *tnear = t0;
  return t0 <= t1;
}
struct Visits {
  double nodes = 0, leaves = 0;
};
static void walk(const std::vector<QNode>& Q, const FlatBvh& b, const Set& s, const Ray& r, bool any, Visits* v) {
  struct E {
    uint32_t ref;
    float t;
  };
  std::vector<E> st{{0u, 0.f}};
  float tmax = r.tmax;
  while (!st.empty()) {
    const E e = st.back();
    st.pop_back();
    if (e.t > tmax) continue;
    if (e.ref & kLeafBit) {
      v->leaves++;
      const uint32_t first = (e.ref & 0x3FFFFFFFu) >> 3, cnt = (e.ref & 7u) + 1u;
      for (uint32_t k = first; k < first + cnt; k++) {
        const uint32_t g = b.slot_gid[k];
        float t;
        if (g == r.skip || !slab(&s.lo[3 * g], &s.hi[3 * g], r, tmax, &t)) continue;
        if (any) return;
        tmax = t;
      }
      continue;
    }
    v->nodes++;
    const QNode& nd = Q[e.ref];
    const float sc[3] = {nd.sx, nd.sy, nd.sz};
    const uint32_t ql[3] = {nd.qlo_x, nd.qlo_y, nd.qlo_z}, qh[3] = {nd.qhi_x, nd.qhi_y, nd.qhi_z};
    E hit[4];
    int nh = 0;
    for (int c = 0; c < 4; c++) {
      if (nd.c[c] == kEmptyChild) continue;
      float lo[3], hi[3], t;
      for (int a = 0; a < 3; a++) lo[a] = fmaf((float)((ql[a] >> (8 * c)) & 255u), sc[a], nd.org[a]), hi[a] = fmaf((float)((qh[a] >> (8 * c)) & 255u), sc[a], nd.org[a]);
      if (slab(lo, hi, r, tmax, &t)) hit[nh++] = {nd.c[c], t};
    }
    std::stable_sort(hit, hit + nh, [](const E& x, const E& y) { return x.t > y.t; });  // the nearest on top
    for (int i = 0; i < nh; i++) st.push_back(hit[i]);
  }
}

static bool run_scene(const char* path, uint32_t top) {
  FILE* f = fopen(path, "rb");
  if (!f) return printf("FAIL: cannot open %s\n", path), false;
  uint32_t n = 0;
  Set s;
  bool ok = fread(&n, 4, 1, f) == 1 && n > 0 && n < (1u << 27);
  if (ok) s.lo.resize(3 * (size_t)n), s.hi.resize(3 * (size_t)n), s.kinds.resize(n);
  ok = ok && fread(s.lo.data(), 12, n, f) == n && fread(s.hi.data(), 12, n, f) == n && fread(s.kinds.data(), 1, n, f) == n;
  fclose(f);
  if (!ok) return printf("FAIL: %s is not a file of boxes\n", path), false;
  Built t;
  if (!run_set("scene", s, top, &t)) return false;
  printf("scene build_ms %.1f reinsert_ms %.1f\n", t.on.build_ms, t.on.reinsert_ms);
  float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t g = 0; g < n; g++)
    for (int a = 0; a < 3; a++) blo[a] = std::min(blo[a], s.lo[3 * g + a]), bhi[a] = std::max(bhi[a], s.hi[3 * g + a]);
  // 20 000 closest-hit rays from points of random primitives into random directions, 20 000 any-hit rays from such points to a point
  // under the ceiling
  const uint32_t nr = 20000;
  std::vector<Ray> rays(2 * nr);
  rng_state = 20260;
  const float light[3] = {0.5f * (blo[0] + bhi[0]), bhi[1] - 0.02f * (bhi[1] - blo[1]), 0.5f * (blo[2] + bhi[2])};
  for (uint32_t i = 0; i < 2 * nr; i++) {
    Ray& r = rays[i];
    r.skip = std::min(n - 1u, (uint32_t)(rnd() * (float)n));
    for (int a = 0; a < 3; a++) r.org[a] = s.lo[3 * r.skip + a] + rnd() * (s.hi[3 * r.skip + a] - s.lo[3 * r.skip + a]);
    if (i < nr) {
      float d[3], l2;
      do {
        for (int a = 0; a < 3; a++) d[a] = 2.f * rnd() - 1.f;
        l2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      } while (l2 > 1.f || l2 < 1e-4f);
      for (int a = 0; a < 3; a++) r.dir[a] = d[a] / sqrtf(l2);
      r.tmax = 1e30f;
    } else {
      for (int a = 0; a < 3; a++) r.dir[a] = light[a] - r.org[a];
      r.tmax = 1.f;
    }
  }
  Visits v[2][2];  // [tree][ray kind]
  for (int k = 0; k < 2; k++) {
    const FlatBvh& b = k ? t.on : t.off;
    std::vector<QNode> Q;
    const uint32_t need = build_qtree(b.nodes, [](uint32_t ref) { return ref; }, &Q);
    if (Q.empty() || need != (k ? t.need_on : t.need_off)) return printf("FAIL scene: build_qtree reports stack need %u, qtree_cost %u\n", need, k ? t.need_on : t.need_off), false;
    for (uint32_t i = 0; i < 2 * nr; i++) walk(Q, b, s, rays[i], i >= nr, &v[k][i >= nr]);
  }
  for (int kind = 0; kind < 2; kind++)
    printf("visits %s nodes_off %.4f nodes_on %.4f node_ratio %.4f leaves_off %.4f leaves_on %.4f leaf_ratio %.4f\n", kind ? "any" : "closest", v[0][kind].nodes / nr,
           v[1][kind].nodes / nr, v[1][kind].nodes / v[0][kind].nodes, v[0][kind].leaves / nr, v[1][kind].leaves / nr, v[1][kind].leaves / v[0][kind].leaves);
  return true;
}

// combs: box centres at 2^b + 0.5 along every axis, one box at the origin and one far out (the set whose Morton tree is a chain), and
// a longer one with boxes that grow with the distance.  Re-insertion deepens the first one's tree from 10 to 13 levels: built with
// -DPB_STACK_DEPTH=12 (a traversal stack of 12 entries) this program must see that pass taken back.
static bool run_combs(bool both) {
  Built t;
  for (int longer = 0; longer < (both ? 2 : 1); longer++) {
    Set s;
    const float h[3] = {0.25f, 0.25f, 0.25f};
    const float o[3] = {0.f, 0.f, 0.f}, far_out[3] = {2097151.f, 2097151.f, 2097151.f};
    s.add(o, h, 0), s.add(far_out, h, 0);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < (longer ? 60 : 21); b++) {
        float c[3] = {0.f, 0.f, 0.f};
        c[a] = ldexpf(1.f, longer ? b - 20 : b) + 0.5f;
        const float e = longer ? ldexpf(0.25f, b - 20) : 0.25f;
        const float hh[3] = {e, e, e};
        s.add(c, hh, 0);
      }
    if (!run_set(longer ? "comb_182" : "comb_65", s, 1000, &t)) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--comb") == 0) return run_combs(false) ? (printf("comb ok, stack %d\n", kStackDepth), 0) : 1;
  if (argc > 1) return run_scene(argv[1], argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : kReinsertTop) ? (printf("scene ok\n"), 0) : 1;
  int sets = 0;
  Built t;
  auto soup = [&](const char* name, uint32_t n, float curve_share, int shape, uint64_t seed) {
    rng_state = seed;
    Set s;
    for (uint32_t g = 0; g < n; g++) {
      const uint8_t kind = rnd() < curve_share ? 1 : 0;
      float c[3], h[3];
      for (int a = 0; a < 3; a++) c[a] = rnd(), h[a] = rnd() * 0.02f;
      if (shape == 1) c[0] = c[1] = c[2] = 0.25f, h[0] = h[1] = h[2] = 0.01f;  // all identical
      if (shape == 2) c[0] = c[1] = c[2] = 0.25f;                               // coincident centroids, different extents
      if (shape == 3 && g < 12) h[g % 3] = 0.f, h[(g + 1) % 3] = h[(g + 2) % 3] = 0.5f, c[(g + 1) % 3] = c[(g + 2) % 3] = 0.5f, c[g % 3] = (g / 3) % 2 ? 1.f : 0.f;  // walls
      s.add(c, h, kind);
    }
    sets++;
    return run_set(name, s, 64 + n / 8, &t);
  };
  bool ok = soup("random_1", 1, 0.f, 0, 1) && soup("random_2", 2, 0.f, 0, 2) && soup("random_3", 3, 0.f, 0, 3) && soup("random_64", 64, 0.f, 0, 4) &&
            soup("random_5000", 5000, 0.f, 0, 5) && soup("identical_300", 300, 0.f, 1, 6) && soup("one_centre_300", 300, 0.f, 2, 7) &&
            soup("mixed_2000", 2000, 0.4f, 0, 8) && soup("walls_3000", 3000, 0.f, 3, 9) && soup("mixed_walls_1500", 1500, 0.3f, 3, 10);
  if (!ok) return 1;
  if (!run_combs(true)) return 1;
  sets += 2;
  printf("bvh reinsert: %d sets ok\n", sets);
  return 0;
}
