// dknearest.h -- the k-nearest contract and its traversal: what knearest.hip's k_knearest runs per query.  The candidate
// of (point, unit) is dnearest.h's (tri_nearest, piece_nearest: §19's D2, u, v, q with the validation clamp), the node loop, the stack
// and the leaf decode are dtrace.h's (walk_tree, leaf_units); here is what is done at a box and with a candidate.  Device code only; all
// arithmetic is float32 without contraction.
//
// C(p) = the units with D2 <= max_dist^2 (a NaN never qualifies), ordered by the key (D2; then the canonical id ShadeRec::gid).  A gid
// names a UNIT: commit.cpp::flatten_prims numbers the units in (instance, geometry, primitive, sub) order, sub being a piece's index
// inside its cubic, so the gid alone makes the order total and, within one cubic, it is the order of sub -- the contract's third key
// (D2, gid, sub) never decides.  (u could not stand in for it: pieces k and k + 1 of a cubic meet in a joint, and a point nearest to that
// joint gives both the same D2 and the same u.)  Per query: |C(p)| and the first K of the order.
//
// The list of the K best lives in the query's own output rows (global memory, the rows of a wave are L2-resident), insertion-sorted by
// the key: a list in registers would be an indexed register array, i.e. scratch.  While the kernel runs word 3 of an ident entry holds
// the bits of D2, the sort key; knearest_finish turns it into sqrtf(D2).  A gid is fetched only when two D2 compare equal.
#pragma once

#include "dnearest.h"
#include "dshade.h"
#include "dtrace.h"

namespace pb {

struct KList {
  uint4* row;     // the query's K entries (slot, bits of u, v, D2); not read or written when K == 0
  float4* cl;     // ... and their closest rows (q | D2), moved in step; null: not wanted
  uint32_t K;     // entries the rows hold
  uint32_t len;   // ... of which filled: min(cnt, K)
  uint32_t cnt;   // candidates within the radius so far
  float md2;      // max_dist^2: the radius
  float kth;      // md2 until the list is full, then the D2 of its last entry: a larger D2 cannot enter the list
};

// One candidate.  `slot`: the unit's slot as the identity format names it.
__device__ __forceinline__ void knearest_offer(const DScene& sc, KList& L, const NearCand& c, uint32_t slot) {
  if (!(c.d2 <= L.md2)) return;  // (a NaN is never accepted)
  L.cnt++;
  if (L.K == 0u || c.d2 > L.kth) return;
  // whether the candidate sorts before entry e
  auto before = [&](const uint4& e) {
    const float ed2 = __uint_as_float(e.w);
    if (c.d2 != ed2) return c.d2 < ed2;
    return sc.shade[slot].gid < sc.shade[e.x].gid;  // (no two units share a gid)
  };
  uint32_t pos;
  if (L.len == L.K) {  // full, and D2 <= the last entry's: the candidate replaces it or is dropped
    pos = L.K - 1u;
    if (!before(L.row[pos])) return;
  } else {
    pos = L.len++;
  }
  while (pos > 0u) {
    const uint4 e = L.row[pos - 1u];
    if (!before(e)) break;
    L.row[pos] = e;
    if (L.cl) L.cl[pos] = L.cl[pos - 1u];
    pos--;
  }
  L.row[pos] = make_uint4(slot, __float_as_uint(c.u), __float_as_uint(c.v), __float_as_uint(c.d2));
  if (L.cl) L.cl[pos] = make_float4(c.q.x, c.q.y, c.q.z, c.d2);
  if (L.len == L.K) L.kth = pos == L.K - 1u ? c.d2 : __uint_as_float(L.row[L.K - 1u].w);
}

// the rows as the callers read them: word 3 of a listed entry becomes sqrtf(D2), the entries past the list misses and zeros
__device__ __forceinline__ void knearest_finish(const KList& L) {
  for (uint32_t j = 0; j < L.len; j++) {
    uint4 e = L.row[j];
    e.w = __float_as_uint(sqrtf(__uint_as_float(e.w)));
    L.row[j] = e;
  }
  for (uint32_t j = L.len; j < L.K; j++) {
    L.row[j] = make_uint4(kNone, 0u, 0u, 0u);
    if (L.cl) L.cl[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// one leaf of either tree (dtrace.h::leaf_units): every unit's candidate offered once, the halves of a TriPair a, then b
template <bool CURVES, bool WIDE>
__device__ __forceinline__ void knearest_leaf(const DScene& sc, uint32_t leaf, V3 p, KList& L) {
  leaf_units<CURVES, WIDE>(
      sc, leaf,
      [&](const float4& w0, const float4& w1, const float4& w2, const float4& w3, const float4& w4) {  // triangles a and b interleaved coordinate by coordinate
        const uint32_t code_a = __float_as_uint(w4.z), code_b = __float_as_uint(w4.w);
        knearest_offer(sc, L, tri_nearest(p, V3(w0.x, w0.z, w1.x), V3(w1.z, w2.x, w2.z), V3(w3.x, w3.z, w4.x)), code_a & kHitSlotMask);
        if (code_b != kNone) knearest_offer(sc, L, tri_nearest(p, V3(w0.y, w0.w, w1.y), V3(w1.w, w2.y, w2.w), V3(w3.y, w3.w, w4.y)), code_b & kHitSlotMask);
        return false;
      },
      [&](const float4& a, const float4& b, const float4& c, uint32_t s) {
        knearest_offer(sc, L, tri_nearest(p, ld3(a), ld3(b), ld3(c)), WIDE ? __float_as_uint(c.w) & kHitSlotMask : s);
        return false;
      },
      [&](const float4& a, const float4& b, uint32_t sub, uint32_t s, uint32_t) {
        knearest_offer(sc, L, piece_nearest(p, a, b, sub), WIDE ? sc.q_hitcode[s] & kHitSlotMask : s);
        return false;
      });
}

// The walker (dtrace.h::walk_tree) with nearest_traverse's box step: children in ascending order of the squared distance from the point
// to their stored box.  COUNT: the bound stays max_dist^2, so every box within the radius is entered and every candidate counted.
// Otherwise the bound is L.kth: once the list is full a box is skipped only when its distance EXCEEDS the K-th entry's D2 -- an equal
// one may hold the smaller gid of a tie --, which with K = 1 is the nearest-point traversal.
template <bool COUNT, bool CURVES, bool WIDE>
__device__ __forceinline__ void knearest_traverse(const DScene& sc, V3 p, KList& L, uint32_t* stack, uint32_t stride, uint32_t* overflow, uint32_t* spill,
                                                  uint32_t spill_stride) {
  walk_tree<WIDE>(
      sc, SimpleStack{stack, stride, spill, spill_stride, overflow},
      [&](const float4& w0, const float4& w1, const float4& w2, const float4& refs, uint32_t k[4]) {
        const float bound = COUNT ? L.md2 : L.kth;
        const uint32_t qlx = __float_as_uint(w1.z), qly = __float_as_uint(w1.w), qlz = __float_as_uint(w2.x);
        const uint32_t qhx = __float_as_uint(w2.y), qhy = __float_as_uint(w2.z), qhz = __float_as_uint(w2.w);
        const uint32_t r[4] = {__float_as_uint(refs.x), __float_as_uint(refs.y), __float_as_uint(refs.z), __float_as_uint(refs.w)};
#pragma unroll
        for (int i = 0; i < 4; i++) {  // a bound is rebuilt as box_test4q rebuilds it: fma(q, s, org)
          auto byte = [i](uint32_t w) { return (float)((w >> (8 * i)) & 255u); };
          const V3 lo(__builtin_fmaf(byte(qlx), w0.w, w0.x), __builtin_fmaf(byte(qly), w1.x, w0.y), __builtin_fmaf(byte(qlz), w1.y, w0.z));
          const V3 hi(__builtin_fmaf(byte(qhx), w0.w, w0.x), __builtin_fmaf(byte(qhy), w1.x, w0.y), __builtin_fmaf(byte(qhz), w1.y, w0.z));
          const float d = box_dist2(lo, hi, p);
          k[i] = (r[i] != kEmptyChild && d <= bound) ? (__float_as_uint(d) & ~3u) | (uint32_t)i : kWideMiss;  // (d >= 0: its bits order like its value)
        }
        wide_sort_keys(k);
      },
      [&](const float4& n0, const float4& n1, const float4& n2, uint32_t c0, uint32_t c1, bool& h0, bool& h1) {
        const float bound = COUNT ? L.md2 : L.kth;
        const float d0 = box_dist2(V3(n0.x, n0.z, n1.x), V3(n1.z, n2.x, n2.z), p), d1 = box_dist2(V3(n0.y, n0.w, n1.y), V3(n1.w, n2.y, n2.w), p);
        h0 = c0 != kEmptyChild && d0 <= bound, h1 = c1 != kEmptyChild && d1 <= bound;
        return d1 < d0;
      },
      [&](uint32_t leaf) {
        knearest_leaf<CURVES, WIDE>(sc, leaf, p, L);
        return false;
      });
}

}  // namespace pb
