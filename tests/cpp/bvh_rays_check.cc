// What the host builder's cost (pbrlab_amd/csrc/bvh_build.cpp, host_scene.h::BvhBuildOptions) buys on rays like the renderer's.  Given
// a file of triangles (uint32 n, uint32 nl, 9 n floats of corners, nl uint32 indices of the emissive triangles) the tree is built
// through build_bvh + build_qtree under several option sets and three seeded ray sets of 20 000 rays are walked near first through the
// Q tree with the quantised slab test of the traversal (fma(q, step, org) bounds, the ray's own interval):
//   camera  from the default camera of the scene's box (16:9), closest-hit, [0, inf)
//   bounce  origin uniform by area on the triangles, direction cosine-distributed about the winding normal, closest-hit, [1e-3, inf)
//   shadow  from the same origins to uniform points on the emissive triangles, any-hit, [1e-3, dist - 1e-3]; pairs of which one side
//           faces away are dropped, as the renderer's light sampling drops them
// Triangles are tested in double precision (closest-hit rays shorten their interval, any-hit rays stop): the counts are the result, not
// the bits.  Printed per option set: a hash of FlatBvh::nodes, what the passes did, and per ray set Q node visits and leaf turns per
// ray (a leaf is one turn whether it holds one triangle or two).  Two builds per set must be byte-identical.  --sets: small and
// degenerate box sets under the turn cost (run_box_set).
// tests/test_bvh_rays_cpu.py builds and runs this (once more under ASan/UBSan) and asserts on the printed lines.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "host_scene.h"
using namespace pb;

static uint64_t rng_state;
static double rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((rng_state >> 11) & ((1ull << 53) - 1)) / 9007199254740992.0;
}
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

struct Ray {
  double org[3], dir[3], tmin, tmax;
};
struct Scene {
  uint32_t n = 0;
  std::vector<float> tri;  // 9 per triangle
  std::vector<uint32_t> lights;
  std::vector<float> lo, hi;
  std::vector<uint8_t> kinds;
};

static void sub3(const double* a, const double* b, double* o) { o[0] = a[0] - b[0], o[1] = a[1] - b[1], o[2] = a[2] - b[2]; }
static void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

static void corners(const Scene& s, uint32_t g, double p[3][3]) {
  for (int c = 0; c < 3; c++)
    for (int a = 0; a < 3; a++) p[c][a] = (double)s.tri[9 * (size_t)g + 3 * c + a];
}
// Moeller-Trumbore, both sides
static bool hit_triangle(const Scene& s, uint32_t g, const Ray& r, double tmax, double* t) {
  double p[3][3], e1[3], e2[3], pv[3], tv[3], qv[3];
  corners(s, g, p);
  sub3(p[1], p[0], e1), sub3(p[2], p[0], e2);
  cross3(r.dir, e2, pv);
  const double det = dot3(e1, pv);
  if (det == 0.0) return false;
  const double inv = 1.0 / det;
  sub3(r.org, p[0], tv);
  const double u = dot3(tv, pv) * inv;
  if (!(u >= 0.0 && u <= 1.0)) return false;
  cross3(tv, e1, qv);
  const double v = dot3(r.dir, qv) * inv;
  if (!(v >= 0.0 && u + v <= 1.0)) return false;
  *t = dot3(e2, qv) * inv;
  return *t >= r.tmin && *t <= tmax;
}
static bool slab(const float* lo, const float* hi, const Ray& r, double tmax, double* tnear) {
  double t0 = r.tmin, t1 = tmax;
  for (int a = 0; a < 3; a++) {
    const double inv = 1.0 / r.dir[a];
    double ta = ((double)lo[a] - r.org[a]) * inv, tb = ((double)hi[a] - r.org[a]) * inv;
    if (ta > tb) std::swap(ta, tb);
    if (ta > t0) t0 = ta;  // (a NaN -- origin on a face of a flat slab -- constrains nothing)
    if (tb < t1) t1 = tb;
  }
  *tnear = t0;
  return t0 <= t1;
}
struct Visits {
  double nodes = 0, leaves = 0, rays = 0;
};
static void walk(const std::vector<QNode>& Q, const FlatBvh& b, const Scene& s, const Ray& r, bool any, Visits* v) {
  struct E {
    uint32_t ref;
    double t;
  };
  std::vector<E> st{{0u, 0.0}};
  double tmax = r.tmax;
  v->rays++;
  while (!st.empty()) {
    const E e = st.back();
    st.pop_back();
    if (e.t > tmax) continue;
    if (e.ref & kLeafBit) {
      v->leaves++;
      const uint32_t first = (e.ref & 0x3FFFFFFFu) >> 3, cnt = (e.ref & 7u) + 1u;
      for (uint32_t k = first; k < first + cnt; k++) {
        double t;
        if (!hit_triangle(s, b.slot_gid[k], r, tmax, &t)) continue;
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
      float lo[3], hi[3];
      double t;
      for (int a = 0; a < 3; a++) lo[a] = fmaf((float)((ql[a] >> (8 * c)) & 255u), sc[a], nd.org[a]), hi[a] = fmaf((float)((qh[a] >> (8 * c)) & 255u), sc[a], nd.org[a]);
      if (slab(lo, hi, r, tmax, &t)) hit[nh++] = {nd.c[c], t};
    }
    std::stable_sort(hit, hit + nh, [](const E& x, const E& y) { return x.t > y.t; });  // the nearest on top
    for (int i = 0; i < nh; i++) st.push_back(hit[i]);
  }
}

static bool read_scene(const char* path, Scene* s) {
  FILE* f = fopen(path, "rb");
  if (!f) return printf("FAIL: cannot open %s\n", path), false;
  uint32_t n = 0, nl = 0;
  bool ok = fread(&n, 4, 1, f) == 1 && fread(&nl, 4, 1, f) == 1 && n > 0 && n < (1u << 27) && nl > 0 && nl <= n;
  if (ok) s->tri.resize(9 * (size_t)n), s->lights.resize(nl);
  ok = ok && fread(s->tri.data(), 36, n, f) == n && fread(s->lights.data(), 4, nl, f) == nl;
  fclose(f);
  for (uint32_t l : s->lights) ok = ok && l < n;
  if (!ok) return printf("FAIL: %s is not a file of triangles\n", path), false;
  s->n = n;
  s->lo.resize(3 * (size_t)n), s->hi.resize(3 * (size_t)n), s->kinds.assign(n, 0);
  for (uint32_t g = 0; g < n; g++)
    for (int a = 0; a < 3; a++) {
      const float* t = &s->tri[9 * (size_t)g];
      s->lo[3 * g + a] = std::min(t[a], std::min(t[3 + a], t[6 + a])), s->hi[3 * g + a] = std::max(t[a], std::max(t[3 + a], t[6 + a]));
    }
  return true;
}

static double tri_area(const Scene& s, uint32_t g, double* normal) {
  double p[3][3], e1[3], e2[3], n[3];
  corners(s, g, p);
  sub3(p[1], p[0], e1), sub3(p[2], p[0], e2);
  cross3(e1, e2, n);
  const double l = sqrt(dot3(n, n));
  if (normal)
    for (int a = 0; a < 3; a++) normal[a] = l > 0.0 ? n[a] / l : 0.0;
  return 0.5 * l;
}
static void point_on(const Scene& s, uint32_t g, double* o) {
  double p[3][3], u = rnd(), v = rnd();
  if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
  corners(s, g, p);
  for (int a = 0; a < 3; a++) o[a] = p[0][a] + u * (p[1][a] - p[0][a]) + v * (p[2][a] - p[0][a]);
}
static uint32_t pick(const std::vector<double>& cdf) {
  const double x = rnd() * cdf.back();
  return (uint32_t)std::min<size_t>(cdf.size() - 1, (size_t)(std::upper_bound(cdf.begin(), cdf.end(), x) - cdf.begin()));
}

static void make_rays(const Scene& s, uint32_t nr, std::vector<Ray>* camera, std::vector<Ray>* bounce, std::vector<Ray>* shadow) {
  double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t g = 0; g < s.n; g++)
    for (int a = 0; a < 3; a++) blo[a] = std::min(blo[a], (double)s.lo[3 * g + a]), bhi[a] = std::max(bhi[a], (double)s.hi[3 * g + a]);
  rng_state = 20261;
  // the default camera (pbrhip.cpp::make_camera) at 16:9: the eye behind the open side, targets uniform on the box's front plane
  {
    const double W = 16.0, H = 9.0;
    double hs, vs;
    if (bhi[0] - blo[0] > bhi[1] - blo[1]) hs = bhi[0] - blo[0], vs = hs * H / W;
    else vs = bhi[1] - blo[1], hs = vs * W / H;
    const double eye[3] = {0.5 * (bhi[0] + blo[0]), 0.5 * (bhi[1] + blo[1]), bhi[2] + hs * 0.5 * sqrt(3.0)};
    for (uint32_t i = 0; i < nr; i++) {
      Ray r;
      const double target[3] = {eye[0] + hs * (rnd() - 0.5), eye[1] + vs * (rnd() - 0.5), bhi[2]};
      sub3(target, eye, r.dir);
      const double l = sqrt(dot3(r.dir, r.dir));
      for (int a = 0; a < 3; a++) r.org[a] = eye[a], r.dir[a] /= l;
      r.tmin = 0.0, r.tmax = INFINITY;
      camera->push_back(r);
    }
  }
  std::vector<double> cdf(s.n), lcdf(s.lights.size());
  double acc = 0.0;
  for (uint32_t g = 0; g < s.n; g++) cdf[g] = acc += tri_area(s, g, nullptr);
  acc = 0.0;
  for (size_t k = 0; k < s.lights.size(); k++) lcdf[k] = acc += tri_area(s, s.lights[k], nullptr);
  for (uint32_t i = 0; i < nr; i++) {
    const uint32_t g = pick(cdf);
    double n[3], t1[3], t2[3];
    Ray r;
    tri_area(s, g, n);
    point_on(s, g, r.org);
    // cosine-distributed about n
    const double up[3] = {fabs(n[0]) < 0.9 ? 1.0 : 0.0, fabs(n[0]) < 0.9 ? 0.0 : 1.0, 0.0};
    cross3(n, up, t1);
    const double l1 = sqrt(dot3(t1, t1));
    for (int a = 0; a < 3; a++) t1[a] /= l1;
    cross3(n, t1, t2);
    const double u = rnd(), phi = 6.283185307179586 * rnd(), rr = sqrt(u), z = sqrt(std::max(0.0, 1.0 - u));
    for (int a = 0; a < 3; a++) r.dir[a] = rr * cos(phi) * t1[a] + rr * sin(phi) * t2[a] + z * n[a];
    r.tmin = 1e-3, r.tmax = INFINITY;
    bounce->push_back(r);
    // the shadow ray of the same origin
    const uint32_t lg = s.lights[pick(lcdf)];
    double ln[3], lp[3], d[3];
    tri_area(s, lg, ln);
    point_on(s, lg, lp);
    sub3(lp, r.org, d);
    const double dist = sqrt(dot3(d, d));
    if (!(dist > 2e-3) || !(dot3(d, n) > 0.0) || !(dot3(d, ln) < 0.0)) continue;
    Ray sr = r;
    for (int a = 0; a < 3; a++) sr.dir[a] = d[a] / dist;
    sr.tmax = dist - 1e-3;
    shadow->push_back(sr);
  }
}

struct OptionSet {
  const char* name;
  BvhBuildOptions opt;
};

// --sets: small and degenerate box sets (bvh_reinsert_check.cc's shapes, which that program builds without options, that is under the
// pricing of before) built under the turn cost with the passes off and on: every primitive in exactly one leaf, depth and Q stack need
// within the stack wherever the builder's own tree is, two builds byte-identical, the cost not above the builder's tree's under the
// same cost.
static bool run_box_set(const char* name, const std::vector<float>& lo, const std::vector<float>& hi, uint32_t top) {
  const std::vector<uint8_t> kinds(lo.size() / 3, 0);
  BvhBuildOptions off, on;
  off.cost = on.cost = kBvhCostTurns;
  on.reinsert_passes = kReinsertPasses, on.reinsert_top = top;
  FlatBvh a, b, again;
  build_bvh(lo, hi, kinds, &a, off), build_bvh(lo, hi, kinds, &b, on), build_bvh(lo, hi, kinds, &again, on);
  if (b.nodes.size() != again.nodes.size() || b.slot_gid != again.slot_gid || memcmp(b.nodes.data(), again.nodes.data(), b.nodes.size() * sizeof(BvhNode)) != 0)
    return printf("FAIL %s: two builds differ\n", name), false;
  std::vector<int> seen(kinds.size(), 0);
  std::vector<uint32_t> todo{0u};
  size_t visited = 0;
  while (!todo.empty()) {
    const uint32_t i = todo.back();
    todo.pop_back();
    if (i >= b.nodes.size() || ++visited > b.nodes.size()) return printf("FAIL %s: node index\n", name), false;
    for (uint32_t ref : {b.nodes[i].c0, b.nodes[i].c1}) {
      if (ref == kEmptyChild) continue;
      if (!(ref & kLeafBit)) {
        todo.push_back(ref);
        continue;
      }
      const uint32_t first = (ref & 0x3FFFFFFFu) >> 3, cnt = (ref & 7u) + 1u;
      if (first + cnt > b.slot_gid.size()) return printf("FAIL %s: leaf range\n", name), false;
      for (uint32_t k = first; k < first + cnt; k++) seen[b.slot_gid[k]]++;
    }
  }
  for (int c : seen)
    if (c != 1) return printf("FAIL %s: a primitive in %d leaves\n", name, c), false;
  uint32_t need_a = 0, need_b = 0;
  const double cost_a = qtree_cost(a.nodes, &need_a, on), cost_b = qtree_cost(b.nodes, &need_b, on);
  if (!(cost_b <= cost_a)) return printf("FAIL %s: cost %.9g with the passes, %.9g without\n", name, cost_b, cost_a), false;
  if (b.depth > (uint32_t)kStackDepth || (need_a <= (uint32_t)kStackDepth && need_b > (uint32_t)kStackDepth)) return printf("FAIL %s: depth %u, stack need %u\n", name, b.depth, need_b), false;
  printf("set %s n %zu passes %u moves %u cost_off %.9g cost_on %.9g depth_off %u depth_on %u need_off %u need_on %u\n", name, kinds.size(), b.reinsert_passes, b.reinsert_moves,
         cost_a, cost_b, a.depth, b.depth, need_a, need_b);
  return true;
}
static bool run_box_sets() {
  auto soup = [](const char* name, uint32_t n, int shape, uint64_t seed) {
    rng_state = seed;
    std::vector<float> lo, hi;
    for (uint32_t g = 0; g < n; g++) {
      float c[3], h[3];
      for (int a = 0; a < 3; a++) c[a] = (float)rnd(), h[a] = (float)rnd() * 0.02f;
      if (shape == 1) c[0] = c[1] = c[2] = 0.25f, h[0] = h[1] = h[2] = 0.01f;  // all identical
      if (shape == 2) c[0] = c[1] = c[2] = 0.25f;                               // coincident centroids, different extents
      if (shape == 3 && g < 12) h[g % 3] = 0.f, h[(g + 1) % 3] = h[(g + 2) % 3] = 0.5f, c[(g + 1) % 3] = c[(g + 2) % 3] = 0.5f, c[g % 3] = (g / 3) % 2 ? 1.f : 0.f;  // walls
      for (int a = 0; a < 3; a++) lo.push_back(c[a] - h[a]), hi.push_back(c[a] + h[a]);
    }
    return run_box_set(name, lo, hi, 64 + n / 8);
  };
  if (!(soup("random_1", 1, 0, 1) && soup("random_2", 2, 0, 2) && soup("random_3", 3, 0, 3) && soup("random_64", 64, 0, 4) && soup("random_5000", 5000, 0, 5) &&
        soup("identical_300", 300, 1, 6) && soup("one_centre_300", 300, 2, 7) && soup("walls_3000", 3000, 3, 9)))
    return false;
  for (int longer = 0; longer < 2; longer++) {  // the combs: chains along every axis, sixty binades in the longer one
    std::vector<float> lo, hi;
    auto add = [&](const float* c, float h) {
      for (int a = 0; a < 3; a++) lo.push_back(c[a] - h), hi.push_back(c[a] + h);
    };
    const float o[3] = {0.f, 0.f, 0.f}, far_out[3] = {2097151.f, 2097151.f, 2097151.f};
    add(o, 0.25f), add(far_out, 0.25f);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < (longer ? 60 : 21); b++) {
        float c[3] = {0.f, 0.f, 0.f};
        c[a] = ldexpf(1.f, longer ? b - 20 : b) + 0.5f;
        add(c, longer ? ldexpf(0.25f, b - 20) : 0.25f);
      }
    if (!run_box_set(longer ? "comb_182" : "comb_65", lo, hi, 1000)) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return printf("usage: bvh_rays_check triangles.bin [--explore] | --sets\n"), 2;
  if (strcmp(argv[1], "--sets") == 0) return run_box_sets() ? (printf("sets ok\n"), 0) : 1;
  const bool explore = argc > 2 && strcmp(argv[2], "--explore") == 0;
  Scene s;
  if (!read_scene(argv[1], &s)) return 1;
  std::vector<Ray> rays[3];
  make_rays(s, 20000, &rays[0], &rays[1], &rays[2]);
  const char* set_names[3] = {"camera", "bounce", "shadow"};
  std::vector<OptionSet> sets;
  auto add = [&](const char* name, uint32_t passes, uint32_t cost, bool surface, uint32_t ntry, double leaf) {
    OptionSet o;
    o.name = name;
    o.opt.reinsert_passes = passes, o.opt.cost = cost, o.opt.surface_term = surface, o.opt.reinsert_try = ntry, o.opt.cost_leaf = leaf;
    sets.push_back(o);
  };
  {  // the three sets the test reads, named after what a scene commit does: its default (the turn cost, the passes), that with the
     // passes off (PBRHIP_BVH_REINSERT=0), and the pricing of before with the passes (PBRHIP_BVH_COST=0)
    OptionSet off, parent, dflt;
    off.name = "off", parent.name = "parent", dflt.name = "default";
    parent.opt.reinsert_passes = dflt.opt.reinsert_passes = kReinsertPasses;
    parent.opt.cost = kBvhCostPrims, off.opt.cost = dflt.opt.cost = kBvhCostTurns;
    sets.push_back(off), sets.push_back(parent), sets.push_back(dflt);
  }
  if (explore) {
    add("parent_off", 0, kBvhCostPrims, false, 0, 1.0);
    add("turns_area_passes", kReinsertPasses, kBvhCostTurns, true, 0, kCostLeaf);
    add("no_surface", kReinsertPasses, kBvhCostTurns, false, kReinsertTry, kCostLeaf);
    add("no_surface_off", 0, kBvhCostTurns, false, kReinsertTry, kCostLeaf);
    add("try_1", kReinsertPasses, kBvhCostTurns, true, 1, kCostLeaf);
    add("try_2", kReinsertPasses, kBvhCostTurns, true, 2, kCostLeaf);
    add("try_8", kReinsertPasses, kBvhCostTurns, true, 8, kCostLeaf);
    add("leaf_0.60", kReinsertPasses, kBvhCostTurns, true, kReinsertTry, 0.60);
    add("leaf_0.85", kReinsertPasses, kBvhCostTurns, true, kReinsertTry, 0.85);
    add("leaf_1.00", kReinsertPasses, kBvhCostTurns, true, kReinsertTry, 1.00);
  }
  printf("scene triangles %u emissive %zu camera_rays %zu bounce_rays %zu shadow_rays %zu cost_node %.4f cost_leaf %.4f\n", s.n, s.lights.size(), rays[0].size(), rays[1].size(),
         rays[2].size(), kCostNode, kCostLeaf);
  for (const OptionSet& o : sets) {
    FlatBvh b, again;
    build_bvh(s.lo, s.hi, s.kinds, &b, o.opt);
    build_bvh(s.lo, s.hi, s.kinds, &again, o.opt);
    if (b.nodes.size() != again.nodes.size() || b.slot_gid != again.slot_gid || memcmp(b.nodes.data(), again.nodes.data(), b.nodes.size() * sizeof(BvhNode)) != 0)
      return printf("FAIL %s: two builds differ\n", o.name), 1;
    if (b.depth > (uint32_t)kStackDepth) return printf("FAIL %s: depth %u beyond the stack\n", o.name, b.depth), 1;
    std::vector<QNode> Q, Q2;
    const uint32_t need = build_qtree(b.nodes, [](uint32_t ref) { return ref; }, &Q, o.opt);
    build_qtree(again.nodes, [](uint32_t ref) { return ref; }, &Q2, o.opt);
    if (Q.empty() || need > (uint32_t)kStackDepth) return printf("FAIL %s: no Q tree (stack need %u)\n", o.name, need), 1;
    if (Q.size() != Q2.size() || memcmp(Q.data(), Q2.data(), Q.size() * sizeof(QNode)) != 0) return printf("FAIL %s: two collapses differ\n", o.name), 1;
    uint32_t need2 = 0;
    const double cost = qtree_cost(b.nodes, &need2, o.opt);
    if (need2 != need) return printf("FAIL %s: build_qtree reports stack need %u, qtree_cost %u\n", o.name, need, need2), 1;
    uint64_t h = fnv(14695981039346656037ull, b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
    h = fnv(h, b.slot_gid.data(), b.slot_gid.size() * 4);
    const uint64_t hq = fnv(14695981039346656037ull, Q.data(), Q.size() * sizeof(QNode));
    printf("tree %s nodes_hash %016llx qtree_hash %016llx nodes %zu qnodes %zu depth %u need %u passes %u moves %u cost %.9g reinsert_ms %.1f\n", o.name, (unsigned long long)h,
           (unsigned long long)hq, b.nodes.size(), Q.size(), b.depth, need, b.reinsert_passes, b.reinsert_moves, cost, b.reinsert_ms);
    for (int k = 0; k < 3; k++) {
      Visits v;
      for (const Ray& r : rays[k]) walk(Q, b, s, r, k == 2, &v);
      printf("rays %s %s nodes %.4f leaves %.4f turns %.4f\n", o.name, set_names[k], v.nodes / v.rays, v.leaves / v.rays, (kCostNode * v.nodes + kCostLeaf * v.leaves) / v.rays);
    }
  }
  printf("rays ok\n");
  return 0;
}
