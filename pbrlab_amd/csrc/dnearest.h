// dnearest.h -- the nearest-point contract, operation for operation, and its traversal by distance: what query.hip's
// k_query_nearest and sdf.hip's signed kernels share.  The leaf decode is dtrace.h's (leaf_units); the node loop and the
// stack are written out in nearest_traverse, which says why.  Device code only; all arithmetic is float32 without contraction.
//
// Beside the contract's answer a candidate carries the FEATURE of its triangle that won (kFeat*): the signed kernels keep it in the
// best-so-far record and fetch that feature's pseudonormal once, in their epilogue.  k_query_nearest never reads it, so none of it is
// left in its code.
#pragma once

#include "dshade.h"
#include "dtrace_pv.h"
#include "feature_kernels.h"

namespace pb {

// the winning feature of a triangle (a, b, c), in the row order of the pseudonormal table; kFeatCurve: a curve piece (no normal)
constexpr uint32_t kFeatAB = 0u, kFeatBC = 1u, kFeatCA = 2u, kFeatA = 3u, kFeatB = 4u, kFeatC = 5u, kFeatFace = 6u, kFeatCurve = 7u;

// squared distance from p to the box [lo, hi]: per axis m = max(max(lo - p, p - hi), 0), summed as dot sums.  Monotone in the box.
__device__ __forceinline__ float box_dist2(V3 lo, V3 hi, V3 p) {
  const float mx = __builtin_fmaxf(__builtin_fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
  const float my = __builtin_fmaxf(__builtin_fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
  const float mz = __builtin_fmaxf(__builtin_fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
  return mx * mx + my * my + mz * mz;
}
// ... to a primitive's own box widened by vbox_lo / vbox_hi (dtrace.h): the validation bound L of the contract
__device__ __forceinline__ float own_box_dist2(V3 lo, V3 hi, V3 p) {
  return box_dist2(V3(vbox_lo(lo.x), vbox_lo(lo.y), vbox_lo(lo.z)), V3(vbox_hi(hi.x), vbox_hi(hi.y), vbox_hi(hi.z)), p);
}
// the clamped segment distance: t = clamp(dot(p - x, e) / dot(e, e), 0, 1), 0 when dot(e, e) is not > 0; q = x + t e; d2 = |p - q|^2
__device__ __forceinline__ float seg_dist2(V3 p, V3 x, V3 y, float& t, V3& q) {
  const V3 e = y - x;
  const float ee = dot(e, e);
  t = 0.0f;
  if (ee > 0.0f) t = __builtin_fminf(__builtin_fmaxf(dot(p - x, e) / ee, 0.0f), 1.0f);
  q = x + t * e;
  const V3 d = p - q;
  return dot(d, d);
}
// the feature a segment's clamped t names: the edge when 0 < t < 1, else the vertex at that end (a segment without length has t = 0)
__device__ __forceinline__ uint32_t seg_feature(float t, uint32_t edge, uint32_t v0, uint32_t v1) {
  return t > 0.0f ? (t < 1.0f ? edge : v1) : v0;
}
struct NearCand {
  float d2, u, v;
  V3 q;
  uint32_t feat;
};
// triangle (a, b, c): the minimum of the three edge distances (ab, bc, ca; a strict < replaces) and, last and again by strict <, the
// plane term where the point projects inside; (u, v) = the closest point's barycentrics of b and c; then the validation clamp
__device__ __forceinline__ NearCand tri_nearest(V3 p, V3 a, V3 b, V3 c) {
  NearCand r;
  float t;
  V3 q;
  r.d2 = seg_dist2(p, a, b, t, r.q);
  r.u = t, r.v = 0.0f, r.feat = seg_feature(t, kFeatAB, kFeatA, kFeatB);
  float d2 = seg_dist2(p, b, c, t, q);
  if (d2 < r.d2) r.d2 = d2, r.q = q, r.u = 1.0f - t, r.v = t, r.feat = seg_feature(t, kFeatBC, kFeatB, kFeatC);
  d2 = seg_dist2(p, c, a, t, q);
  if (d2 < r.d2) r.d2 = d2, r.q = q, r.u = 0.0f, r.v = 1.0f - t, r.feat = seg_feature(t, kFeatCA, kFeatC, kFeatA);
  const V3 n = cross(b - a, c - a);
  const float nn = dot(n, n);
  const float s_ab = dot(cross(b - a, p - a), n), s_bc = dot(cross(c - b, p - b), n), s_ca = dot(cross(a - c, p - c), n);
  if (nn > 0.0f && s_ab >= 0.0f && s_bc >= 0.0f && s_ca >= 0.0f) {
    const float h = dot(p - a, n), w = h / nn;  // (h / nn) * h, not (h * h) / nn: fourth order in length, not sixth over fourth
    d2 = w * h;
    if (d2 < r.d2) r.d2 = d2, r.q = p - w * n, r.u = s_ca / nn, r.v = s_ab / nn, r.feat = kFeatFace;
  }
  const V3 lo(__builtin_fminf(__builtin_fminf(a.x, b.x), c.x), __builtin_fminf(__builtin_fminf(a.y, b.y), c.y), __builtin_fminf(__builtin_fminf(a.z, b.z), c.z));
  const V3 hi(__builtin_fmaxf(__builtin_fmaxf(a.x, b.x), c.x), __builtin_fmaxf(__builtin_fmaxf(a.y, b.y), c.y), __builtin_fmaxf(__builtin_fmaxf(a.z, b.z), c.z));
  const float L = own_box_dist2(lo, hi, p);
  r.d2 = r.d2 < L ? L : r.d2;
  return r;
}
// curve piece `sub` of its cubic, end points a, b (xyz + radius): the distance to the axis (the radius is ignored, as pbrhip_render_motion
// ignores the ribbon's width); u = (sub + t) / 4, v = 0; the own box is segment_test's (the end points widened by the larger radius)
__device__ __forceinline__ NearCand piece_nearest(V3 p, const float4& a, const float4& b, uint32_t sub) {
  NearCand r;
  float t;
  r.d2 = seg_dist2(p, ld3(a), ld3(b), t, r.q);
  r.u = ((float)sub + t) * 0.25f, r.v = 0.0f, r.feat = kFeatCurve;
  const float rm = __builtin_fmaxf(fabsf(a.w), fabsf(b.w));
  const V3 lo(__builtin_fminf(a.x, b.x) - rm, __builtin_fminf(a.y, b.y) - rm, __builtin_fminf(a.z, b.z) - rm);
  const V3 hi(__builtin_fmaxf(a.x, b.x) + rm, __builtin_fmaxf(a.y, b.y) + rm, __builtin_fmaxf(a.z, b.z) + rm);
  const float L = own_box_dist2(lo, hi, p);
  r.d2 = r.d2 < L ? L : r.d2;
  return r;
}

struct Nearest {
  float d2, u, v;  // d2: the best D2 so far (before the first candidate: max_dist^2)
  V3 q;
  uint32_t slot;   // kNone: none yet
  uint32_t feat;   // the winner's feature (kFeat*)
};
// acceptance: D2 <= best (a NaN is never accepted); equal D2 goes to the smaller canonical id
__device__ __forceinline__ void nearest_offer(const DScene& sc, const NearCand& c, uint32_t slot, Nearest& best) {
  bool acc = c.d2 <= best.d2;
  if (acc && c.d2 == best.d2 && best.slot != kNone) acc = sc.shade[slot].gid < sc.shade[best.slot].gid;
  if (acc) best.d2 = c.d2, best.u = c.u, best.v = c.v, best.q = c.q, best.slot = slot, best.feat = c.feat;
}

// before the first candidate: nothing found within max_dist (pt.w)
__device__ __forceinline__ Nearest nearest_none(const float4& pt) {
  Nearest best;
  best.d2 = pt.w * pt.w, best.u = 0.0f, best.v = 0.0f, best.q = V3(0.0f), best.slot = kNone, best.feat = kFeatCurve;
  return best;
}
// the answer of query i as the callers read it: ident = (slot, bits of u, v, distance), closest = (point | D2); either may be null
__device__ __forceinline__ void nearest_store(const Nearest& best, uint32_t i, uint4* ident, float4* closest) {
  const bool found = best.slot != kNone;
  if (ident) ident[i] = found ? make_uint4(best.slot, __float_as_uint(best.u), __float_as_uint(best.v), __float_as_uint(sqrtf(best.d2))) : make_uint4(kNone, 0u, 0u, 0u);
  if (closest) closest[i] = found ? make_float4(best.q.x, best.q.y, best.q.z, best.d2) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// one leaf of either tree (dtrace.h::leaf_units): every unit's candidate offered once
template <bool CURVES, bool WIDE>
__device__ __forceinline__ void nearest_leaf(const DScene& sc, uint32_t leaf, V3 p, Nearest& best) {
  leaf_units<CURVES, WIDE>(
      sc, leaf,
      [&](const float4& w0, const float4& w1, const float4& w2, const float4& w3, const float4& w4) {  // triangles a and b interleaved coordinate by coordinate
        const uint32_t code_a = __float_as_uint(w4.z), code_b = __float_as_uint(w4.w);
        nearest_offer(sc, tri_nearest(p, V3(w0.x, w0.z, w1.x), V3(w1.z, w2.x, w2.z), V3(w3.x, w3.z, w4.x)), code_a & kHitSlotMask, best);
        if (code_b != kNone) nearest_offer(sc, tri_nearest(p, V3(w0.y, w0.w, w1.y), V3(w1.w, w2.y, w2.w), V3(w3.y, w3.w, w4.y)), code_b & kHitSlotMask, best);
        return false;
      },
      [&](const float4& a, const float4& b, const float4& c, uint32_t s) {
        nearest_offer(sc, tri_nearest(p, ld3(a), ld3(b), ld3(c)), WIDE ? __float_as_uint(c.w) & kHitSlotMask : s, best);
        return false;
      },
      [&](const float4& a, const float4& b, uint32_t sub, uint32_t s, uint32_t) {
        nearest_offer(sc, piece_nearest(p, a, b, sub), WIDE ? sc.q_hitcode[s] & kHitSlotMask : s, best);
        return false;
      });
}

// A traversal by distance: children in ascending order of the squared distance L from the point to their stored box, a box skipped only
// when L exceeds the best D2 so far.  The loop is dtrace.h::walk_tree's and the stack rule dtrace.h::TravStack's, both WRITTEN OUT here and
// kept in step by hand: as a call of the walker, and again with the shared stack alone, k_query_nearest came out 2 % slower on the Q tree
// (the backend turns the pop's select between LDS and spill into a branch; profiles/README.md, "One stack, one walker").  With this text
// the nearest and signed kernels compile to the instructions they had before the walker existed.  Whoever edits walk_tree or TravStack
// edits this too; a drift shows as a bit-exact failure in tests/test_query_gpu.py (test_nearest_point_equals_the_brute_force on the
// tie-heavy soups, test_comb_reaches_the_spill_part_of_the_stack for the spill half of the stack) and tests/test_sdf_gpu.py.
template <bool CURVES, bool WIDE>
__device__ __forceinline__ void nearest_traverse(const DScene& sc, V3 p, Nearest& best, uint32_t* stack, uint32_t stride, uint32_t* overflow,
                                                 uint32_t* spill, uint32_t spill_stride) {
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
  int sp = 0;
  uint32_t cur = 0;
  for (;;) {
    uint32_t next = kEmptyChild;
    if (WIDE) {
      const float4* np = sc.wide + (size_t)cur * 4u;
      const float4 w0 = np[0], w1 = np[1], w2 = np[2], refs = np[3];
      const uint32_t qlx = __float_as_uint(w1.z), qly = __float_as_uint(w1.w), qlz = __float_as_uint(w2.x);
      const uint32_t qhx = __float_as_uint(w2.y), qhy = __float_as_uint(w2.z), qhz = __float_as_uint(w2.w);
      const uint32_t r[4] = {__float_as_uint(refs.x), __float_as_uint(refs.y), __float_as_uint(refs.z), __float_as_uint(refs.w)};
      uint32_t k[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {  // a bound is rebuilt as box_test4q rebuilds it: fma(q, s, org)
        auto byte = [i](uint32_t w) { return (float)((w >> (8 * i)) & 255u); };
        const V3 lo(__builtin_fmaf(byte(qlx), w0.w, w0.x), __builtin_fmaf(byte(qly), w1.x, w0.y), __builtin_fmaf(byte(qlz), w1.y, w0.z));
        const V3 hi(__builtin_fmaf(byte(qhx), w0.w, w0.x), __builtin_fmaf(byte(qhy), w1.x, w0.y), __builtin_fmaf(byte(qhz), w1.y, w0.z));
        const float L = box_dist2(lo, hi, p);
        k[i] = (r[i] != kEmptyChild && L <= best.d2) ? (__float_as_uint(L) & ~3u) | (uint32_t)i : kWideMiss;  // (L >= 0: its bits order like its value)
      }
      wide_sort_keys(k);
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
      const float L0 = box_dist2(V3(n0.x, n0.z, n1.x), V3(n1.z, n2.x, n2.z), p), L1 = box_dist2(V3(n0.y, n0.w, n1.y), V3(n1.w, n2.y, n2.w), p);
      const bool h0 = c0 != kEmptyChild && L0 <= best.d2, h1 = c1 != kEmptyChild && L1 <= best.d2;
      if (h0 && h1) {
        uint32_t nearc = c0, farc = c1;
        if (L1 < L0) nearc = c1, farc = c0;
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
      nearest_leaf<CURVES, WIDE>(sc, next, p, best);
      next = kEmptyChild;
    }
    cur = next;
  }
}

// an inactive query: a NaN or infinite coordinate, max_dist NaN or below 0
__device__ __forceinline__ bool point_active(const float4& pt) { return isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z) && pt.w >= 0.0f; }

}  // namespace pb
