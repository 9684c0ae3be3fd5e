// dallhits.h -- the all-hits contract and its traversal: what allhits.hip's k_all_hits runs per ray.  Device code only;
// all arithmetic is float32 without contraction.
//
// A UNIT is what a leaf tests once: a triangle (dtrace.h::tri_test / tri_test_pair) or one linear piece of a curve's cubic
// (segment_test).  A unit's hit is ACCEPTED exactly when the closest-hit traversal could accept it: the primitive test passes,
// tmin < t <= tmax, and hit_inside validates t against the unit's own box -- the functions, the operations and the bits of t, u, v are
// dtrace.h's.  H = the accepted hits of all units, ordered by the key (t; then the canonical primitive id ShadeRec::gid; then u): two
// pieces of one cubic share a gid and can tie in t, and differ in u.  Per ray: the number of hits |H| and the first K of the order.
//
// The list of the K best lives in the ray's own output row (global memory, the rows of a wave are L2-resident), insertion-sorted by the
// key: a list in registers would be an indexed register array, i.e. scratch.  A gid is fetched only when two t compare equal.
#pragma once

#include "dshade.h"
#include "dtrace.h"

namespace pb {

struct AllList {
  uint4* row;     // the ray's K entries (slot, bits of u, v, t); not read or written when K == 0
  uint32_t K;     // entries the row holds
  uint32_t len;   // ... of which filled: min(cnt, K)
  uint32_t cnt;   // accepted hits so far
  float kth;      // the ray's tmax until the list is full, then the t of its last entry: a larger t cannot enter the list
};

// One accepted hit (t <= the ray's tmax; the caller has checked it).  `slot`: the hit's slot as the identity format names it.
__device__ __forceinline__ void all_offer(const DScene& sc, AllList& L, float t, float u, float v, uint32_t slot) {
  L.cnt++;
  if (L.K == 0u || t > L.kth) return;
  // whether the candidate sorts before entry e
  auto before = [&](const uint4& e) {
    const float et = __uint_as_float(e.w);
    if (t != et) return t < et;
    const uint32_t g = sc.shade[slot].gid, eg = sc.shade[e.x].gid;
    if (g != eg) return g < eg;
    return u < __uint_as_float(e.y);
  };
  uint32_t pos;
  if (L.len == L.K) {  // full, and t <= the last entry's: the candidate replaces it or is dropped
    pos = L.K - 1u;
    if (!before(L.row[pos])) return;
  } else {
    pos = L.len++;
  }
  while (pos > 0u) {
    const uint4 e = L.row[pos - 1u];
    if (!before(e)) break;
    L.row[pos] = e;
    pos--;
  }
  L.row[pos] = make_uint4(slot, __float_as_uint(u), __float_as_uint(v), __float_as_uint(t));
  if (L.len == L.K) L.kth = pos == L.K - 1u ? t : __uint_as_float(L.row[L.K - 1u].w);
}

// one leaf of either tree: the leaf formats are dtrace.h::leaf_test's, every unit offered once
template <bool CURVES, bool WIDE>
__device__ __forceinline__ void all_leaf(const DScene& sc, uint32_t leaf, V3 o, V3 d, V3 inv, float tmin, float tmax, AllList& L) {
  uint32_t first = (leaf & 0x3FFFFFFFu) >> 3, count = (leaf & 7u) + 1u;
  const bool is_curve = (leaf & kCurveBit) != 0;
  if (WIDE && !CURVES) {  // one TriPair (dscene.h): both triangles in one packed test, each half offered on its own
    const float4* g = sc.wide + sc.q_tri0 + (size_t)first * kTriPairWords;
    const float4 w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3], w4 = g[4];
    bool ok_a, ok_b;
    f2 t, u, v;
    tri_test_pair(w0, w1, w2, w3, w4, o.x, o.y, o.z, d.x, d.y, d.z, inv.x, inv.y, inv.z, tmin, ok_a, ok_b, t, u, v);
    const uint32_t code_a = __float_as_uint(w4.z), code_b = __float_as_uint(w4.w);
    if (ok_a && t.x <= tmax) all_offer(sc, L, t.x, u.x, v.x, code_a & kHitSlotMask);
    if (ok_b && code_b != kNone && t.y <= tmax) all_offer(sc, L, t.y, u.y, v.y, code_b & kHitSlotMask);  // (a leaf of one triangle stores it twice)
    return;
  }
  const bool rec = WIDE && CURVES && is_curve;  // a curve record of the Q tree: one or two pieces at points P, P + 2
  const uint32_t sub_a = first & 3u, sub_b = leaf & 3u;
  if (rec) first &= ~3u, count = (leaf & kCurvePairBit) ? 2u : 1u;
  for (uint32_t k = 0; k < count; k++) {
    const uint32_t s = first + (rec ? 2u * k : k);
    float t, u, v;
    if (WIDE) {
      if (!is_curve) {
        const float4* g = sc.wide + sc.q_tri0 + (size_t)s * 3;
        const float4 a = g[0], b = g[1], c = g[2];
        if (tri_test(ld3(a), ld3(b), ld3(c), o, d, inv, tmin, t, u, v) && t <= tmax) all_offer(sc, L, t, u, v, __float_as_uint(c.w) & kHitSlotMask);
      } else {
        const float4* g = sc.wide + sc.q_pt0 + s;
        const float4 a = g[0], b = g[1];
        if (segment_test(a, b, k ? sub_b : sub_a, o, d, inv, tmin, tmax, t, u, v)) all_offer(sc, L, t, u, v, sc.q_hitcode[s] & kHitSlotMask);
      }
    } else {
      const float4* g = sc.slots + (size_t)s * 4;
      const float4 a = g[0], b = g[1], c = g[2];
      if (!CURVES || !is_curve) {
        if (tri_test(ld3(a), ld3(b), ld3(c), o, d, inv, tmin, t, u, v) && t <= tmax) all_offer(sc, L, t, u, v, s);
      } else {
        if (segment_test(a, b, __float_as_uint(c.x), o, d, inv, tmin, tmax, t, u, v)) all_offer(sc, L, t, u, v, s);
      }
    }
  }
}

// dtrace.h::traverse_mode's stack discipline and loop.  COUNT: the interval stays [tmin, tmax], so every box the ray crosses within it
// is entered and every accepted hit is counted.  Otherwise the interval ends at L.kth: once the list is full a box is skipped only when
// its entry distance EXCEEDS the K-th entry's t -- an equal entry may hold the smaller gid of a tie --, which with K = 1 is the
// closest-hit traversal.
template <bool COUNT, bool CURVES, bool WIDE>
__device__ __forceinline__ void all_traverse(const DScene& sc, V3 o, V3 d, float tmin, float tmax, AllList& L, uint32_t* stack, uint32_t stride,
                                             uint32_t* overflow, uint32_t* spill, uint32_t spill_stride) {
  auto push = [&](int& sp, uint32_t v) {
    if (sp < kSimpleLdsStack) stack[(uint32_t)sp * stride] = v, sp++;
    else if (sp < kStackDepth) spill[(uint32_t)(sp - kSimpleLdsStack) * spill_stride] = v, sp++;
    else *overflow = 1u;
  };
  auto pop = [&](int& sp) {
    sp--;
    return sp < kSimpleLdsStack ? stack[(uint32_t)sp * stride] : spill[(uint32_t)(sp - kSimpleLdsStack) * spill_stride];
  };
  if (sc.num_nodes == 0) return;
  const V3 inv(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  int sp = 0;
  uint32_t cur = 0;
  for (;;) {
    const float bound = COUNT ? tmax : L.kth;
    uint32_t next = kEmptyChild;
    if (WIDE) {
      const float4* np = sc.wide + (size_t)cur * 4u;
      const float4 w0 = np[0], w1 = np[1], w2 = np[2], refs = np[3];
      uint32_t k[4];
      wide_node_keys(w0, w1, w2, refs, o, make_float4(inv.x, inv.y, inv.z, 0.f), tmin, bound, k);
#pragma unroll
      for (int j = 3; j >= 1; j--) {
        if (k[j] == kWideMiss) continue;
        push(sp, wide_ref(refs, k[j]));
      }
      if (k[0] != kWideMiss) next = wide_ref(refs, k[0]);
    } else {
      const float4* np = reinterpret_cast<const float4*>(sc.nodes + cur);
      const float4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
      const uint32_t c0 = __float_as_uint(n3.x), c1 = __float_as_uint(n3.y);
      float t0, t1;
      bool h0, h1;
      box_test2(n0, n1, n2, o, inv, tmin, bound, h0, h1, t0, t1);
      if (h0 && h1) {
        uint32_t nearc = c0, farc = c1;
        if (t1 < t0) nearc = c1, farc = c0;
        push(sp, farc);
        next = nearc;
      } else if (h0) {
        next = c0;
      } else if (h1) {
        next = c1;
      }
    }
    for (;;) {
      if (next == kEmptyChild) {
        if (sp == 0) return;
        next = pop(sp);
      }
      if (!(next & kLeafBit)) break;
      all_leaf<CURVES, WIDE>(sc, next, o, d, inv, tmin, tmax, L);
      next = kEmptyChild;
    }
    cur = next;
  }
}

}  // namespace pb
