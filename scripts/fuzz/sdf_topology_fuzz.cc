// Stand-alone check of pbrlab_amd/csrc/sdf_topology.cpp (the incidence lists and the topology report of the signed-distance queries,
// DESIGN.md §20) under AddressSanitizer + UBSan on the CPU: random and degenerate index sets -- repeated indices inside a face, isolated
// vertices, duplicated faces, a 1000-face fan around one vertex, curve slots mixed in, several objects, permuted slot orders, refused
// inputs -- with the invariants of the lists checked after every build.  Build and run (scripts/README.md):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ipbrlab_amd/csrc scripts/fuzz/sdf_topology_fuzz.cc \
//       pbrlab_amd/csrc/sdf_topology.cpp -o /tmp/sdf_topology_fuzz && /tmp/sdf_topology_fuzz
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "sdf_topology.h"

using namespace pb;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                          \
      return;                                                              \
    }                                                                      \
  } while (0)

// the invariants of a build over `n` slots
static void check(uint32_t n, const std::vector<uint32_t>& slot_gid, const std::vector<uint32_t>& object, const std::vector<uint32_t>& vid) {
  SdfTopology t;
  CHECK(build_sdf_topology(n, slot_gid.data(), object.data(), vid.data(), &t));
  CHECK(t.slot_feat.size() == 6 * (size_t)n && !t.feat_off.empty() && t.feat_off.front() == 0 && t.feat_off.back() == t.feat_items.size());
  const uint32_t nf = (uint32_t)t.feat_off.size() - 1;
  uint32_t tris = 0;
  std::vector<uint32_t> used(nf, 0);
  for (uint32_t s = 0; s < n; s++) {
    const bool curve = object[slot_gid[s]] == kSdfNone;
    tris += !curve;
    for (int k = 0; k < 6; k++) {
      const uint32_t f = t.slot_feat[6 * (size_t)s + k];
      CHECK(curve ? f == kSdfNone : f < nf);
      if (curve) continue;
      used[f]++;
      // the feature's list holds this slot, with this corner if it is a vertex
      bool found = false;
      for (uint32_t j = t.feat_off[f]; j < t.feat_off[f + 1]; j++) found = found || (t.feat_items[j] >> 2 == s && (t.feat_items[j] & 3u) == (k < 3 ? 3u : (uint32_t)k - 3u));
      CHECK(found);
    }
  }
  CHECK(t.report.triangles == tris && t.feat_items.size() == 6 * (size_t)tris);
  for (uint32_t f = 0; f < nf; f++) {
    CHECK(t.feat_off[f] < t.feat_off[f + 1] && used[f] == t.feat_off[f + 1] - t.feat_off[f]);
    for (uint32_t j = t.feat_off[f]; j < t.feat_off[f + 1]; j++) {
      CHECK((t.feat_items[j] >> 2) < n && object[slot_gid[t.feat_items[j] >> 2]] != kSdfNone);
      if (j > t.feat_off[f]) CHECK(slot_gid[t.feat_items[j - 1] >> 2] <= slot_gid[t.feat_items[j] >> 2]);  // ascending canonical id
    }
  }
  // the report against a map-based count
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> edges;  // -> (faces, forward)
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> verts;
  for (uint32_t g = 0; g < n; g++) {
    if (object[g] == kSdfNone) continue;
    for (int k = 0; k < 3; k++) {
      const uint32_t a = vid[3 * (size_t)g + k], b = vid[3 * (size_t)g + (k + 1) % 3];
      auto& e = edges[{object[g], std::min(a, b), std::max(a, b)}];
      e.first++, e.second += a < b;
      verts[{object[g], a}]++;
    }
  }
  SdfReport want;
  for (const auto& kv : edges) {
    const uint32_t faces = kv.second.first, fwd = kv.second.second;
    if (faces == 1) want.edges_boundary++;
    else if (faces >= 3) want.edges_nonmanifold++;
    else if (fwd == 1) want.edges_manifold++;
    else want.edges_inconsistent++;
  }
  CHECK(t.report.vertices == verts.size() && nf == edges.size() + verts.size());
  CHECK(t.report.edges_boundary == want.edges_boundary && t.report.edges_nonmanifold == want.edges_nonmanifold);
  CHECK(t.report.edges_manifold == want.edges_manifold && t.report.edges_inconsistent == want.edges_inconsistent);
}

int main() {
  std::mt19937 rng(20);
  auto identity = [](uint32_t n) {
    std::vector<uint32_t> p(n);
    for (uint32_t i = 0; i < n; i++) p[i] = i;
    return p;
  };
  // nothing at all; one triangle; one curve piece
  check(0, {}, {}, {});
  check(1, {0}, {0}, {0, 1, 2});
  check(1, {0}, {kSdfNone}, {0, 0, 0});
  // a closed cube, an open quad, a flipped face, three faces on an edge: the reports the tests expect
  {
    const std::vector<uint32_t> cube = {0, 1, 2, 0, 2, 3, 5, 6, 7, 5, 7, 4, 1, 5, 4, 1, 4, 0, 3, 2, 6, 3, 6, 7, 2, 6, 5, 2, 5, 1, 0, 3, 7, 0, 7, 4};
    check(12, identity(12), std::vector<uint32_t>(12, 0), cube);
    SdfTopology t;
    build_sdf_topology(12, identity(12).data(), std::vector<uint32_t>(12, 0).data(), cube.data(), &t);
    if (t.report.edges_boundary + t.report.edges_nonmanifold != 0 || t.report.edges_manifold + t.report.edges_inconsistent != 18 || t.report.vertices != 8) g_failed++;
    check(3, identity(3), {0, 0, 0}, {0, 1, 2, 0, 1, 3, 1, 0, 4});
    check(2, {1, 0}, {0, 0}, {0, 1, 2, 0, 2, 3});
  }
  // a 1000-face fan around vertex 0, in a shuffled slot order
  {
    const uint32_t n = 1000;
    std::vector<uint32_t> vid, order = identity(n);
    for (uint32_t i = 0; i < n; i++) vid.insert(vid.end(), {0u, 1 + i, 1 + (i + 1) % n});
    std::shuffle(order.begin(), order.end(), rng);
    check(n, order, std::vector<uint32_t>(n, 0), vid);
  }
  // random sets: few vertices (many shared and repeated indices, duplicated faces), isolated vertices (indices far apart), the largest
  // index, curve slots mixed in, several objects
  for (int round = 0; round < 400; round++) {
    const uint32_t n = 1 + rng() % 200, nv = 1 + rng() % (round % 3 == 0 ? 4 : 300), nobj = 1 + rng() % 4;
    std::vector<uint32_t> object(n), vid(3 * (size_t)n), order = identity(n);
    for (uint32_t g = 0; g < n; g++) {
      object[g] = rng() % 7 == 0 ? kSdfNone : rng() % nobj;
      for (int k = 0; k < 3; k++) vid[3 * (size_t)g + k] = rng() % 50 == 0 ? 0xFFFFFFFFu - rng() % 2 : (rng() % nv) * (round % 5 == 0 ? 1000003u : 1u);
      if (rng() % 10 == 0) vid[3 * (size_t)g + 1] = vid[3 * (size_t)g];  // a repeated index
      if (g && rng() % 10 == 0) object[g] = object[g - 1], std::copy(&vid[3 * (size_t)(g - 1)], &vid[3 * (size_t)g], &vid[3 * (size_t)g]);  // a duplicate
    }
    std::shuffle(order.begin(), order.end(), rng);
    check(n, order, object, vid);
  }
  // refused: a slot order that is no permutation
  {
    SdfTopology t;
    const uint32_t dup[3] = {0, 0, 1}, big[2] = {0, 2}, obj[3] = {0, 0, 0}, vid[9] = {0, 1, 2, 0, 1, 2, 0, 1, 2};
    if (build_sdf_topology(3, dup, obj, vid, &t) || !t.slot_feat.empty()) g_failed++;
    if (build_sdf_topology(2, big, obj, vid, &t) || !t.feat_off.empty()) g_failed++;
  }
  if (g_failed) {
    fprintf(stderr, "sdf_topology_fuzz: %d checks failed\n", g_failed);
    return 1;
  }
  printf("sdf_topology_fuzz ok\n");
  return 0;
}
