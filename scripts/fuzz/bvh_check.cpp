// host BVH builders under ASan/UBSan: random / degenerate inputs, structural validation of the binary tree, of the Q tree's
// device layout (build_qlayout) and of the random walks' entries (build_sss_entries)
#include <math.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "host_scene.h"
using namespace pb;
static bool inside(const float* lo, const float* hi, const float* l, const float* h) {
  for (int a = 0; a < 3; a++) if (!(lo[a] <= l[a] && h[a] <= hi[a])) return false;
  return true;
}
int main() {
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  size_t cases = 0;
  for (int it = 0; it < 400; ++it) {
    uint32_t n = it < 8 ? (uint32_t)it : (uint32_t)(rng() % 3000);
    std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
    std::vector<uint8_t> kinds(n);
    const int mode = it % 5;
    for (uint32_t i = 0; i < n; i++) {
      float c[3] = {U(rng), U(rng), U(rng)};
      if (mode == 1) c[0] = c[1] = c[2] = 0.25f;                 // all centroids equal
      if (mode == 2) c[1] = 0.f, c[2] = 0.f;                     // on a line
      if (mode == 3 && i % 2) { c[0] = lo[3 * (i - 1)], c[1] = lo[3 * (i - 1) + 1], c[2] = lo[3 * (i - 1) + 2]; }   // duplicates
      float e = mode == 4 ? 0.f : 0.05f * (U(rng) + 1.f);
      for (int a = 0; a < 3; a++) lo[3 * i + a] = c[a] - (mode == 3 ? 0.f : e), hi[3 * i + a] = c[a] + e;
      if (it >= 392) {  // the last cases: segments of one axis-parallel line (a scene collapsed to a line: no box has an area, every split costs 0)
        const int ax = it % 3;
        for (int a = 0; a < 3; a++)
          if (a != ax) lo[3 * i + a] = hi[3 * i + a] = 0.5f;
      }
      kinds[i] = (uint8_t)(it % 3 != 0 && rng() % 4 == 0);  // (every third case: triangles only)
    }
    FlatBvh b;
    BvhBuildOptions opt;  // (every other case: with subtree re-insertion -- it runs on the triangle-only cases -- over few to all of the nodes, decided by the Q collapse's cost or by the binary tree's)
    opt.reinsert_passes = it % 2 ? kReinsertPasses : 0u, opt.reinsert_top = 8u + 13u * (uint32_t)it, opt.for_qtree = it % 4 == 1;
    build_bvh(lo, hi, kinds, &b, opt);
    if (b.depth > (uint32_t)kStackDepth) return printf("FAIL: depth %u\n", b.depth), 1;
    if (n == 0) { if (!b.nodes.empty()) return printf("FAIL: nodes for empty input\n"), 1; continue; }
    std::vector<int> seen(n, 0);
    if (b.slot_gid.size() != n) return printf("FAIL: slot count\n"), 1;
    for (uint32_t g : b.slot_gid) { if (g >= n || seen[g]++) return printf("FAIL: slot permutation\n"), 1; }
    // walk: every leaf range valid, one kind, <= kMaxLeaf; child boxes (stored widened) contain their primitives
    std::vector<uint32_t> stack{0}, leaf_first(n, 0), leaf_cnt(n, 0);  // (the binary leaf of every slot: its first slot and count)
    size_t leaves_prims = 0;
    while (!stack.empty()) {
      uint32_t id = stack.back(); stack.pop_back();
      if (id >= b.nodes.size()) return printf("FAIL: node index\n"), 1;
      const BvhNode& nd = b.nodes[id];
      const uint32_t ch[2] = {nd.c0, nd.c1};
      for (int c = 0; c < 2; c++) {
        if (ch[c] == kEmptyChild) continue;
        float bl[3] = {nd.lo[0][c], nd.lo[1][c], nd.lo[2][c]}, bh[3] = {nd.hi[0][c], nd.hi[1][c], nd.hi[2][c]};
        if (ch[c] & kLeafBit) {
          uint32_t first = (ch[c] & 0x3FFFFFFFu) >> 3, cnt = (ch[c] & 7u) + 1u;
          if (first + cnt > n || cnt > (uint32_t)kMaxLeaf) return printf("FAIL: leaf range\n"), 1;
          for (uint32_t s = first; s < first + cnt; s++) {
            uint32_t g = b.slot_gid[s];
            if ((kinds[g] != 0) != ((ch[c] & kCurveBit) != 0)) return printf("FAIL: leaf kind\n"), 1;
            if (!inside(bl, bh, &lo[3 * g], &hi[3 * g])) return printf("FAIL: leaf box\n"), 1;
            leaf_first[s] = first, leaf_cnt[s] = cnt;
          }
          leaves_prims += cnt;
        } else stack.push_back(ch[c]);
      }
    }
    if (leaves_prims != n) return printf("FAIL: %zu prims in leaves, %u expected\n", leaves_prims, n), 1;
    // Slot words as the scene commit writes them (dscene.h): a triangle's corners inside its box, a curve piece's end points and
    // its index in the cubic; every slot carries a recognisable routing code in slots[4k + 2].w.
    std::vector<float4> slots(4 * (size_t)n, make_float4(0.f, 0.f, 0.f, 0.f));
    auto code = [&](uint32_t k) { return k | ((b.slot_gid[k] * 0x9E3779B1u) & ~kHitSlotMask); };
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t g = b.slot_gid[k];
      const float* l = &lo[3 * g]; const float* h = &hi[3 * g];
      float4* sl = &slots[4 * (size_t)k];
      sl[0] = make_float4(l[0], l[1], l[2], 0.f), sl[1] = make_float4(h[0], kinds[g] ? h[1] : l[1], h[2], 0.f);
      sl[2] = kinds[g] ? make_float4(__builtin_bit_cast(float, g & 3u), 0.f, 0.f, 0.f) : make_float4(l[0], h[1], h[2], 0.f);
      sl[2].w = __builtin_bit_cast(float, code(k) & ~kHitSlotMask);
    }
    // The Q tree collapsed from it and its leaves packed as the scene commit packs them (build_qlayout).  Checked: every primitive
    // in exactly one leaf, every node reachable once, every quantised child box -- rebuilt with the device's expression
    // fmaf(q, s, org) -- contains the binary tree's widened box of each of its primitives, the reported stack need is the true
    // maximum; triangle leaves (TriPair / 48-byte) and curve records decode back to their binary leaf's slots and hit codes.
    QLayout q;
    build_qlayout(b, slots, kinds, &q);
    const std::vector<QNode>& w = q.nodes;
    if (w.empty() || w.size() > b.nodes.size()) return printf("FAIL: wide node count\n"), 1;
    if (q.tri.size() % 4) return printf("FAIL: q_pt0 = 4 x nodes + %zu triangle words is not a multiple of 4\n", q.tri.size()), 1;
    if (q.pts.size() < 8 || q.pts.size() % 2 || q.hit.size() != q.pts.size()) return printf("FAIL: point / hit code array sizes\n"), 1;
    if (std::any_of(&q.pts.back().x - 12, &q.pts.back().x + 4, [](float v) { return v != 0.f; })) return printf("FAIL: trailing point words\n"), 1;
    const bool tri_pairs = std::all_of(kinds.begin(), kinds.end(), [](uint8_t kd) { return kd == 0; });
    auto bits = [](float f) { return __builtin_bit_cast(uint32_t, f); };
    std::vector<int> visited(w.size(), 0), prim_seen(n, 0);
    std::vector<uint32_t> parent(w.size(), kNone), prim_node(n, kNone), prim_leaf(n, kNone);
    struct It { uint32_t id, pending; };
    std::vector<It> st2{{0u, 0u}};
    uint32_t need = 0;
    size_t wide_prims = 0;
    while (!st2.empty()) {
      It it = st2.back(); st2.pop_back();
      if (it.id >= w.size() || visited[it.id]++) return printf("FAIL: wide node index / revisit\n"), 1;
      const QNode& nd = w[it.id];
      const float sc[3] = {nd.sx, nd.sy, nd.sz};
      const uint32_t ql[3] = {nd.qlo_x, nd.qlo_y, nd.qlo_z}, qh[3] = {nd.qhi_x, nd.qhi_y, nd.qhi_z};
      int used = 0;
      for (int c = 0; c < 4; c++) used += nd.c[c] != kEmptyChild;
      if (used == 0) return printf("FAIL: wide node without children\n"), 1;
      need = std::max(need, it.pending + (uint32_t)used - 1u);
      for (int c = 0; c < 4; c++) {
        const uint32_t ref = nd.c[c];
        if (ref == kEmptyChild) continue;
        float bl[3], bh[3];
        for (int a = 0; a < 3; a++) {
          if (!(sc[a] > 0.f) || !std::isfinite(sc[a])) return printf("FAIL: step\n"), 1;
          bl[a] = fmaf((float)((ql[a] >> (8 * c)) & 255u), sc[a], nd.org[a]), bh[a] = fmaf((float)((qh[a] >> (8 * c)) & 255u), sc[a], nd.org[a]);
        }
        auto check_prim = [&](uint32_t g) {
          for (int a = 0; a < 3; a++)
            if (!(bl[a] <= BvhNode::widen_lo(lo[3 * g + a]) && bh[a] >= BvhNode::widen_hi(hi[3 * g + a]))) return false;
          return true;
        };
        if (!(ref & kLeafBit)) {
          if (ref < w.size()) parent[ref] = it.id;
          st2.push_back({ref, it.pending + (uint32_t)used - 1u});
          continue;
        }
        // decode the leaf into the slots it holds
        const uint32_t first = (ref & 0x3FFFFFFFu) >> 3;
        uint32_t ks[2], cnt;
        if (ref & kCurveBit) {  // a curve record: kLeafBit | kCurveBit | (P | i_a) << 3 | (pair ? kCurvePairBit | i_b : 0)
          const uint32_t P = first & ~3u;
          cnt = (ref & kCurvePairBit) ? 2u : 1u;
          if (cnt == 1 && (ref & 3u)) return printf("FAIL: curve record of one piece with a second index\n"), 1;
          if (P >= (1u << 27) || P + 2 * cnt > q.pts.size() - 4) return printf("FAIL: curve record position %u\n", P), 1;
          for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t hc = q.hit[P + 2 * i], k = ks[i] = hc & kHitSlotMask;
            if (k >= n || hc != code(k)) return printf("FAIL: hit code at point %u\n", P + 2 * i), 1;
            if (memcmp(&q.pts[P + 2 * i], &slots[4 * (size_t)k], 32)) return printf("FAIL: record words\n"), 1;
            if ((i ? ref : first) % 4 != (bits(slots[4 * (size_t)k + 2].x) & 3u)) return printf("FAIL: piece index in the reference\n"), 1;
          }
        } else {  // triangles: a TriPair (five words, the two interleaved coordinate by coordinate) or 48 bytes each (code in .w)
          cnt = (ref & 7u) + 1u;
          const size_t at0 = (size_t)first * (tri_pairs ? kTriPairWords : 3u);
          if (at0 + (tri_pairs ? kTriPairWords : 3u * cnt) > q.tri.size()) return printf("FAIL: triangle leaf range\n"), 1;
          const float* t = &q.tri[at0].x;
          auto at = [&](uint32_t i, int c, int j) { return tri_pairs ? t[(3 * c + j) * 2 + i] : t[12 * i + 4 * c + j]; };
          for (uint32_t i = 0; i < (tri_pairs ? 2u : cnt); i++) {
            const uint32_t hc = bits(tri_pairs ? t[18 + i] : t[12 * i + 11]), k = ks[i] = hc & kHitSlotMask;
            if (i == cnt) {  // a TriPair of one triangle stores it twice, the copy with code kNone
              for (int c = 0; c < 9; c++) if (hc != kNone || at(1, c / 3, c % 3) != at(0, c / 3, c % 3)) return printf("FAIL: TriPair copy\n"), 1;
              continue;
            }
            if (k >= n || hc != code(k)) return printf("FAIL: triangle code\n"), 1;
            for (int c = 0; c < 9; c++)
              if (at(i, c / 3, c % 3) != (&slots[4 * (size_t)k + c / 3].x)[c % 3]) return printf("FAIL: triangle corners\n"), 1;
          }
        }
        // the leaf is exactly one binary leaf, in slot order
        if (leaf_first[ks[0]] != ks[0] || leaf_cnt[ks[0]] != cnt || (cnt == 2 && ks[1] != ks[0] + 1u)) return printf("FAIL: Q leaf is not its binary leaf\n"), 1;
        for (uint32_t i = 0; i < cnt; i++) {
          const uint32_t g = b.slot_gid[ks[i]];
          if (prim_seen[g]++) return printf("FAIL: primitive in two wide leaves\n"), 1;
          if ((kinds[g] != 0) != ((ref & kCurveBit) != 0)) return printf("FAIL: wide leaf kind\n"), 1;
          if (!check_prim(g)) return printf("FAIL: quantised box does not contain its primitive\n"), 1;
          prim_node[g] = it.id, prim_leaf[g] = ref;
        }
        wide_prims += cnt;
      }
    }
    if (wide_prims != n) return printf("FAIL: %zu prims in wide leaves, %u expected\n", wide_prims, n), 1;
    for (int v : visited) if (v != 1) return printf("FAIL: unreachable wide node\n"), 1;
    if (q.stack_need != need) return printf("FAIL: stack need %u reported, %u found\n", q.stack_need, need), 1;
    // Where random walks start (build_sss_entries), for instances made of the primitives of ninst slices along x, an instance
    // with no primitive and one random box.  Checked: the entry is an inner node (or there is none), at most max_foreign foreign
    // references, and every primitive whose box meets the widened region lies under the entry or under a foreign reference.
    const uint32_t ninst = 1u + (uint32_t)it % 6u, max_foreign = (uint32_t)it % (kSssMaxForeign + 1u);
    std::vector<float> ilo(3 * (ninst + 2), INFINITY), ihi(3 * (ninst + 2), -INFINITY);
    for (uint32_t g = 0; g < n; g++) {
      const uint32_t i = std::min(ninst - 1u, (uint32_t)std::max(0.f, (lo[3 * g] + 1.f) * 0.5f * (float)ninst));
      for (int a = 0; a < 3; a++) ilo[3 * i + a] = std::min(ilo[3 * i + a], lo[3 * g + a]), ihi[3 * i + a] = std::max(ihi[3 * i + a], hi[3 * g + a]);
    }
    for (int a = 0; a < 3; a++) ilo[3 * (ninst + 1) + a] = -0.5f + 0.5f * U(rng), ihi[3 * (ninst + 1) + a] = 0.5f + 0.5f * U(rng);
    const std::vector<SssEntry> E = build_sss_entries(w, ilo, ihi, max_foreign);
    if (E.size() != ninst + 2) return printf("FAIL: SSS entry count\n"), 1;
    for (size_t i = 0; i < E.size(); i++) {
      if (E[i].entry == 0 && E[i].nforeign) return printf("FAIL: SSS foreign references without an entry\n"), 1;
      if (E[i].entry == 0) continue;
      if ((E[i].entry & kLeafBit) || E[i].entry >= w.size()) return printf("FAIL: SSS entry is not an inner node\n"), 1;
      if (E[i].nforeign > max_foreign) return printf("FAIL: %u SSS foreign references, at most %u\n", E[i].nforeign, max_foreign), 1;
      float m2 = 0.f;  // (how far beyond the region a primitive's box can matter: build_sss_entries)
      for (int a = 0; a < 3; a++) m2 = std::max(m2, 2e-3f * (ihi[3 * i + a] - ilo[3 * i + a]));
      for (uint32_t g = 0; g < n; g++) {
        bool meets = true;
        for (int a = 0; a < 3; a++) meets = meets && lo[3 * g + a] <= E[i].hi[a] + m2 && hi[3 * g + a] >= E[i].lo[a] - m2;
        if (!meets) continue;
        bool covered = false;  // (its leaf, then the nodes above it)
        for (uint32_t v = prim_leaf[g], up = prim_node[g]; v != kNone && !covered; v = up, up = (up == 0 || up == kNone) ? kNone : parent[up])
          for (uint32_t f = 0; f <= E[i].nforeign && !covered; f++) covered = v == (f ? E[i].foreign[f - 1].ref : E[i].entry);
        if (!covered) return printf("FAIL: primitive %u meets instance %zu's region but is under no entry reference\n", g, i), 1;
      }
    }
    cases++;
  }
  printf("bvh builder: %zu cases ok\n", cases);
  return 0;
}
