// dallhits.h -- the all-hits contract and its traversal: what allhits.hip's k_all_hits runs per ray.  The node loop, the
// stack and the leaf decode are dtrace.h's (walk_tree, leaf_units); here is what is done at a box and with a unit.  Device code only; all
// arithmetic is float32 without contraction.
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

// one leaf of either tree (dtrace.h::leaf_units): every unit tested against [tmin, tmax] and offered once
template <bool CURVES, bool WIDE>
__device__ __forceinline__ void all_leaf(const DScene& sc, uint32_t leaf, V3 o, V3 d, V3 inv, float tmin, float tmax, AllList& L) {
  leaf_units<CURVES, WIDE>(
      sc, leaf,
      [&](const float4& w0, const float4& w1, const float4& w2, const float4& w3, const float4& w4) {  // one packed test, each half offered on its own
        bool ok_a, ok_b;
        f2 t, u, v;
        tri_test_pair(w0, w1, w2, w3, w4, o.x, o.y, o.z, d.x, d.y, d.z, inv.x, inv.y, inv.z, tmin, ok_a, ok_b, t, u, v);
        const uint32_t code_a = __float_as_uint(w4.z), code_b = __float_as_uint(w4.w);
        if (ok_a && t.x <= tmax) all_offer(sc, L, t.x, u.x, v.x, code_a & kHitSlotMask);
        if (ok_b && code_b != kNone && t.y <= tmax) all_offer(sc, L, t.y, u.y, v.y, code_b & kHitSlotMask);  // (a leaf of one triangle stores it twice)
        return false;
      },
      [&](const float4& a, const float4& b, const float4& c, uint32_t s) {
        float t, u, v;
        if (tri_test(ld3(a), ld3(b), ld3(c), o, d, inv, tmin, t, u, v) && t <= tmax) all_offer(sc, L, t, u, v, WIDE ? __float_as_uint(c.w) & kHitSlotMask : s);
        return false;
      },
      [&](const float4& a, const float4& b, uint32_t sub, uint32_t s, uint32_t) {
        float t, u, v;
        if (segment_test(a, b, sub, o, d, inv, tmin, tmax, t, u, v)) all_offer(sc, L, t, u, v, WIDE ? sc.q_hitcode[s] & kHitSlotMask : s);
        return false;
      });
}

// The walker (dtrace.h::walk_tree) with the closest-hit traversal's box tests.  COUNT: the interval stays [tmin, tmax], so every box the
// ray crosses within it is entered and every accepted hit is counted.  Otherwise the interval ends at L.kth: once the list is full a box
// is skipped only when its entry distance EXCEEDS the K-th entry's t -- an equal entry may hold the smaller gid of a tie --, which with
// K = 1 is the closest-hit traversal.
template <bool COUNT, bool CURVES, bool WIDE>
__device__ __forceinline__ void all_traverse(const DScene& sc, V3 o, V3 d, float tmin, float tmax, AllList& L, uint32_t* stack, uint32_t stride,
                                             uint32_t* overflow, uint32_t* spill, uint32_t spill_stride) {
  const V3 inv(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  walk_tree<WIDE>(
      sc, SimpleStack{stack, stride, spill, spill_stride, overflow},
      [&](const float4& w0, const float4& w1, const float4& w2, const float4& refs, uint32_t k[4]) {
        wide_node_keys(w0, w1, w2, refs, o, make_float4(inv.x, inv.y, inv.z, 0.f), tmin, COUNT ? tmax : L.kth, k);
      },
      [&](const float4& n0, const float4& n1, const float4& n2, uint32_t, uint32_t, bool& h0, bool& h1) {
        float t0, t1;
        box_test2(n0, n1, n2, o, inv, tmin, COUNT ? tmax : L.kth, h0, h1, t0, t1);
        return t1 < t0;
      },
      [&](uint32_t leaf) {
        all_leaf<CURVES, WIDE>(sc, leaf, o, d, inv, tmin, tmax, L);
        return false;
      });
}

}  // namespace pb
