// refit_gpu.hip -- the committed trees REFITTED on the device after vertex or transform edits (pbrhip_scene_refit): the topology of the
// binary tree and of the Q tree stays whatever their builder made it, every stored box and every geometry word of a leaf record is
// recomputed from the moved slots ("The refit, exactly"; tests/_refit_model.py restates it):
//
//   tight box    of a slot: a triangle's float min / max of its three corners; a curve piece's min(a, b) - r and max(a, b) + r with
//                r = max(|a.w|, |b.w|) -- what commit.cpp::slot_tight_box computes from the very numbers the slot holds
//   W(box)       BvhNode::widen_lo / widen_hi per bound
//   binary tree  every child reference but kEmptyChild: W(union of the tight boxes of the slots below it), as both builders store it.  The
//                union of a subtree is kept UNWIDENED in a working array (six floats per node) and widened where it is stored: the union
//                of widened boxes is NOT always the widened union -- below |v| ~ 1e-30 the absolute term makes W() non-monotone
//                (tests/test_refit_model_cpu.py has the counter-example)
//   leaf records the geometry words of every TriPair / 48-byte triangle slot / curve record, from the slots their own codes name
//   Q nodes      child i's box: W(union of the tight boxes of the slots below it) -- a leaf's from its record's one or two slots, an inner
//                child's from the working array of the Q nodes' own unwidened unions (never taken back from quantised bytes); then
//                qquant.h::quantise_node
//
// Kernels: k_rf_scatter (the dirty slots and ShadeRecs from one packed upload), k_rf_plan (one launch per level, top down: the nodes
// of every level, which is the refit plan -- built once per committed tree), k_rf_pack (leaf records), k_rf_bin / k_rf_q (one launch
// per level, deepest first).  No kernel waits for another block and nothing is handed between blocks inside a launch: a dependency
// between levels is a new launch, as in qtree_gpu.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include <chrono>

#include "host_scene.h"
#include "qquant.h"

namespace pb {
namespace {

constexpr int kThreads = 256;

// BvhNode::widen_lo / widen_hi (dscene.h), spelled out for the device as bvh_gpu.hip does
__device__ __forceinline__ float wlo(float v) { return v - (fabsf(v) * 1.52587890625e-05f + 1e-30f); }
__device__ __forceinline__ float whi(float v) { return v + (fabsf(v) * 1.52587890625e-05f + 1e-30f); }

__device__ __forceinline__ QBox tight_box(const float4* __restrict__ slots, uint32_t k, bool curve) {
  const float4 a = slots[4 * (size_t)k], b = slots[4 * (size_t)k + 1];
  QBox o;
  if (curve) {
    const float r = fmaxf(fabsf(a.w), fabsf(b.w));
    o.lo[0] = fminf(a.x, b.x) - r, o.lo[1] = fminf(a.y, b.y) - r, o.lo[2] = fminf(a.z, b.z) - r;
    o.hi[0] = fmaxf(a.x, b.x) + r, o.hi[1] = fmaxf(a.y, b.y) + r, o.hi[2] = fmaxf(a.z, b.z) + r;
  } else {
    const float4 c = slots[4 * (size_t)k + 2];
    o.lo[0] = fminf(fminf(a.x, b.x), c.x), o.lo[1] = fminf(fminf(a.y, b.y), c.y), o.lo[2] = fminf(fminf(a.z, b.z), c.z);
    o.hi[0] = fmaxf(fmaxf(a.x, b.x), c.x), o.hi[1] = fmaxf(fmaxf(a.y, b.y), c.y), o.hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
  }
  return o;
}
__device__ __forceinline__ void unite(QBox& o, const QBox& b) {
#pragma unroll
  for (int a = 0; a < 3; a++) o.lo[a] = fminf(o.lo[a], b.lo[a]), o.hi[a] = fmaxf(o.hi[a], b.hi[a]);
}
__device__ __forceinline__ QBox widened(const QBox& b) {
  QBox o;
#pragma unroll
  for (int a = 0; a < 3; a++) o.lo[a] = wlo(b.lo[a]), o.hi[a] = whi(b.hi[a]);
  return o;
}

// The union of the tight boxes of the one or two slots behind a leaf reference of the Q tree, found through the codes its record holds
// (code_a / code_b of a TriPair, .w of the third word of a 48-byte slot, q_hitcode of a curve record).  false: an index out of range.
__device__ __forceinline__ bool q_leaf_box(uint32_t ref, const float4* __restrict__ slots, uint32_t ns, uint32_t tri_pairs,
                                           const float4* __restrict__ tri, uint32_t tri_words, const uint32_t* __restrict__ hit, uint32_t npts,
                                           QBox* out) {
  const uint32_t rec = (ref & 0x3FFFFFFFu) >> 3;
  QBox b;
  if (ref & kCurveBit) {
    const uint32_t P = rec & ~3u;
    if (P + 4u > npts) return false;
    const uint32_t sa = hit[P] & kHitSlotMask;
    if (sa >= ns) return false;
    b = tight_box(slots, sa, true);
    if (ref & kCurvePairBit) {
      const uint32_t sb = hit[P + 2] & kHitSlotMask;
      if (sb >= ns) return false;
      unite(b, tight_box(slots, sb, true));
    }
  } else if (tri_pairs) {
    if ((size_t)rec * kTriPairWords + kTriPairWords > tri_words) return false;
    const float4 w = tri[(size_t)rec * kTriPairWords + 4];
    const uint32_t ca = __float_as_uint(w.z), cb = __float_as_uint(w.w);
    if ((ca & kHitSlotMask) >= ns) return false;
    b = tight_box(slots, ca & kHitSlotMask, false);
    if (cb != kNone) {
      if ((cb & kHitSlotMask) >= ns) return false;
      unite(b, tight_box(slots, cb & kHitSlotMask, false));
    }
  } else {
    const uint32_t count = (ref & 7u) + 1u;
    if (3 * ((size_t)rec + count) > tri_words) return false;
    for (uint32_t i = 0; i < count; i++) {
      const uint32_t sa = __float_as_uint(tri[3 * ((size_t)rec + i) + 2].w) & kHitSlotMask;
      if (sa >= ns) return false;
      const QBox t = tight_box(slots, sa, false);
      if (i == 0) b = t;
      else unite(b, t);
    }
  }
  *out = b;
  return true;
}

}  // namespace

// (the kernels have external names: the code-object tables of the tests list them by name)
// The dirty slots: `packed` holds m slot indices (padded to whole 16-byte words), then m x 64 B of slot, then m x 128 B of ShadeRec;
// one thread per 16-byte word of an entry.
__global__ void __launch_bounds__(kThreads) k_rf_scatter(const float4* __restrict__ packed, uint32_t m, uint32_t ns, float4* slots, float4* shade) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t e = t / 12u;
  const uint32_t w = (uint32_t)(t % 12u);
  if (e >= m) return;
  const uint32_t k = reinterpret_cast<const uint32_t*>(packed)[e];
  if (k >= ns) return;
  const float4* src_slots = packed + (m + 3u) / 4u;
  const float4* src_shade = src_slots + 4 * (size_t)m;
  if (w < 4u) slots[4 * (size_t)k + w] = src_slots[4 * e + w];
  else shade[8 * (size_t)k + (w - 4u)] = src_shade[8 * e + (w - 4u)];
}

// One level of either tree, top down: node in[i] appends its inner children to `out` (the next level).  Both node formats are 64 B
// with the child references in the last 16-byte word (two of them for a BvhNode, four for a QNode: `fan`).  A node has one parent,
// so a valid tree fills exactly its node count; `room` only keeps a broken one inside the list.
__global__ void __launch_bounds__(kThreads) k_rf_plan(const uint4* __restrict__ items, uint32_t nitems, uint32_t fan, const uint32_t* __restrict__ in,
                                                      uint32_t nin, uint32_t* out, uint32_t room, uint32_t* count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nin) return;
  const uint32_t v = in[i];
  if (v >= nitems) return;
  const uint4 c = items[4 * (size_t)v + 3];
  const uint32_t ref[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if ((uint32_t)k >= fan || (ref[k] & kLeafBit) || ref[k] >= nitems) continue;  // (kEmptyChild has the leaf bit)
    const uint32_t at = atomicAdd(count, 1u);
    if (at < room) out[at] = ref[k];
  }
}

// The leaf records of the Q tree, one thread per child reference: what bvh_build.cpp's tri_leaf / curve_leaf would write from the new
// slots.  Codes, q_hitcode, the padding and the zero points stay.  (A leaf has one parent: no record is written twice.)
__global__ void __launch_bounds__(kThreads) k_rf_pack(const QNode* __restrict__ q, uint32_t nq, const float4* __restrict__ slots, uint32_t ns,
                                                      uint32_t tri_pairs, float4* tri, uint32_t tri_words, float4* pts,
                                                      const uint32_t* __restrict__ hit, uint32_t npts, uint32_t* fail) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * (size_t)nq) return;
  const uint32_t ref = reinterpret_cast<const uint32_t*>(q)[16 * (t >> 2) + 12 + (t & 3)];
  if (ref == kEmptyChild || !(ref & kLeafBit)) return;
  const uint32_t rec = (ref & 0x3FFFFFFFu) >> 3;
  bool ok = true;
  if (ref & kCurveBit) {
    const uint32_t P = rec & ~3u;
    ok = P + 4u <= npts;
    const uint32_t sa = ok ? hit[P] & kHitSlotMask : 0u;
    const uint32_t sb = ok && (ref & kCurvePairBit) ? hit[P + 2] & kHitSlotMask : sa;
    ok = ok && sa < ns && sb < ns;
    if (ok) {
      pts[P] = slots[4 * (size_t)sa], pts[P + 1] = slots[4 * (size_t)sa + 1];
      if (ref & kCurvePairBit) pts[P + 2] = slots[4 * (size_t)sb], pts[P + 3] = slots[4 * (size_t)sb + 1];
    }
  } else if (tri_pairs) {
    float4* o = tri + kTriPairWords * (size_t)rec;
    ok = (size_t)rec * kTriPairWords + kTriPairWords <= tri_words;
    const float4 w4 = ok ? o[4] : make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t ca = __float_as_uint(w4.z), cb = __float_as_uint(w4.w);
    const uint32_t sa = ca & kHitSlotMask, sb = cb == kNone ? sa : (cb & kHitSlotMask);  // (one triangle: stored twice)
    ok = ok && sa < ns && sb < ns;
    if (ok) {
      const float4* a = slots + 4 * (size_t)sa;
      const float4* b = slots + 4 * (size_t)sb;
      const float4 a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
      o[0] = make_float4(a0.x, b0.x, a0.y, b0.y), o[1] = make_float4(a0.z, b0.z, a1.x, b1.x), o[2] = make_float4(a1.y, b1.y, a1.z, b1.z);
      o[3] = make_float4(a2.x, b2.x, a2.y, b2.y), o[4] = make_float4(a2.z, b2.z, w4.z, w4.w);
    }
  } else {
    const uint32_t count = (ref & 7u) + 1u;
    ok = 3 * ((size_t)rec + count) <= tri_words;
    for (uint32_t i = 0; ok && i < count; i++) {
      float4* o = tri + 3 * ((size_t)rec + i);
      const float code = o[2].w;
      const uint32_t sa = __float_as_uint(code) & kHitSlotMask;
      if (sa >= ns) {
        ok = false;
        break;
      }
      const float4* a = slots + 4 * (size_t)sa;
      float4 w2 = a[2];
      w2.w = code;
      o[0] = a[0], o[1] = a[1], o[2] = w2;
    }
  }
  if (!ok) atomicOr(fail, 2u);
}

// One level of the binary tree, deepest first: the boxes node list[i] stores for its children, and its own unwidened union into the
// working array bbox (two 16-byte words per node).  The level below is finished (it was an earlier launch); references, pad and the NaN
// box of an empty child stay as they are.
__global__ void __launch_bounds__(kThreads) k_rf_bin(BvhNode* nodes, uint32_t nb, const float4* __restrict__ slots, uint32_t ns, float4* bbox,
                                                     const uint32_t* __restrict__ list, uint32_t count, uint32_t* fail) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t v = list[i];
  if (v >= nb) return;
  BvhNode nd = nodes[v];
  QBox own;
  bool any = false;
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t ref = c ? nd.c1 : nd.c0;
    if (ref == kEmptyChild) continue;
    QBox b;
    if (ref & kLeafBit) {
      const uint32_t first = (ref & 0x3FFFFFFFu) >> 3, cnt = (ref & 7u) + 1u;
      if (first + cnt > ns) {
        atomicOr(fail, 2u);
        continue;
      }
      b = tight_box(slots, first, (ref & kCurveBit) != 0u);
      for (uint32_t j = 1; j < cnt; j++) unite(b, tight_box(slots, first + j, (ref & kCurveBit) != 0u));
    } else {
      if (ref >= nb) {
        atomicOr(fail, 2u);
        continue;
      }
      const float4 l = bbox[2 * (size_t)ref], h = bbox[2 * (size_t)ref + 1];
      b.lo[0] = l.x, b.lo[1] = l.y, b.lo[2] = l.z, b.hi[0] = h.x, b.hi[1] = h.y, b.hi[2] = h.z;
    }
    if (any) unite(own, b);
    else own = b;
    any = true;
    const QBox w = widened(b);
#pragma unroll
    for (int a = 0; a < 3; a++) nd.lo[a][c] = w.lo[a], nd.hi[a][c] = w.hi[a];
  }
  if (!any) return;
  nodes[v] = nd;
  bbox[2 * (size_t)v] = make_float4(own.lo[0], own.lo[1], own.lo[2], 0.f);
  bbox[2 * (size_t)v + 1] = make_float4(own.hi[0], own.hi[1], own.hi[2], 0.f);
}

// One level of the Q tree, deepest first: the boxes of the children of Q node list[i] (a leaf's from its record's slots, an inner
// child's from the working array qbox -- the unwidened union below a Q node, two 16-byte words each, that the child's own launch
// filled), widened and quantised by qquant.h.  c[4] stays.
__global__ void __launch_bounds__(kThreads) k_rf_q(QNode* q, uint32_t nq, const float4* __restrict__ slots, uint32_t ns, uint32_t tri_pairs,
                                                   const float4* __restrict__ tri, uint32_t tri_words, const uint32_t* __restrict__ hit, uint32_t npts,
                                                   float4* qbox, const uint32_t* __restrict__ list, uint32_t count, uint32_t* fail) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t v = list[i];
  if (v >= nq) return;
  const uint4 cw = reinterpret_cast<const uint4*>(q)[4 * (size_t)v + 3];
  const uint32_t ref[4] = {cw.x, cw.y, cw.z, cw.w};
  QBox box[4] = {}, u = {};
  int n = 0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (n != k || ref[k] == kEmptyChild) continue;  // (the children are a prefix)
    n = k + 1;
    QBox b = {};
    if (ref[k] & kLeafBit) {
      ok = q_leaf_box(ref[k], slots, ns, tri_pairs, tri, tri_words, hit, npts, &b) && ok;
    } else if (ref[k] < nq) {
      const float4 l = qbox[2 * (size_t)ref[k]], h = qbox[2 * (size_t)ref[k] + 1];
      b.lo[0] = l.x, b.lo[1] = l.y, b.lo[2] = l.z, b.hi[0] = h.x, b.hi[1] = h.y, b.hi[2] = h.z;
    } else {
      ok = false;
    }
    if (k == 0) u = b;
    else unite(u, b);
    box[k] = widened(b);
  }
  if (!ok || n == 0) {
    atomicOr(fail, 2u);
    return;
  }
  QNode nd;
  if (!quantise_node(box, n, &nd)) {
    atomicOr(fail, 1u);
    return;
  }
  uint4* o = reinterpret_cast<uint4*>(q) + 4 * (size_t)v;
  o[0] = make_uint4(__float_as_uint(nd.org[0]), __float_as_uint(nd.org[1]), __float_as_uint(nd.org[2]), __float_as_uint(nd.sx));
  o[1] = make_uint4(__float_as_uint(nd.sy), __float_as_uint(nd.sz), nd.qlo_x, nd.qlo_y);
  o[2] = make_uint4(nd.qlo_z, nd.qhi_x, nd.qhi_y, nd.qhi_z);
  qbox[2 * (size_t)v] = make_float4(u.lo[0], u.lo[1], u.lo[2], 0.f);
  qbox[2 * (size_t)v + 1] = make_float4(u.hi[0], u.hi[1], u.hi[2], 0.f);
}

namespace {

#define GPU_CHK(x)                   \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return e_; \
  } while (0)

uint32_t grid(size_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

// the levels of one tree into list[0 .. nitems): every launch is sized by the exact count of the level before it
hipError_t plan_levels(hipStream_t st, const void* items, uint32_t nitems, uint32_t fan, uint32_t* list, uint32_t* d_count, std::vector<uint32_t>* off) {
  off->assign(1, 0u);
  const uint32_t root[1] = {0u};
  GPU_CHK(hipMemcpyAsync(list, root, 4, hipMemcpyHostToDevice, st));
  uint32_t at = 0, nin = 1;
  while (nin > 0) {
    off->push_back(at + nin);
    const uint32_t room = nitems - (at + nin);
    if (room == 0) break;
    GPU_CHK(hipMemsetAsync(d_count, 0, 4, st));
    hipLaunchKernelGGL(k_rf_plan, dim3(grid(nin)), dim3(kThreads), 0, st, reinterpret_cast<const uint4*>(items), nitems, fan, list + at, nin,
                       list + at + nin, room, d_count);
    GPU_CHK(hipGetLastError());
    uint32_t next = 0;
    GPU_CHK(hipMemcpyAsync(&next, d_count, 4, hipMemcpyDeviceToHost, st));
    GPU_CHK(hipStreamSynchronize(st));
    at += nin;
    nin = next < room ? next : room;
  }
  return hipSuccess;
}

}  // namespace

void RefitPlan::release() {
  if (d_list) (void)hipFree(d_list);
  if (d_qbox) (void)hipFree(d_qbox);
  if (d_bbox) (void)hipFree(d_bbox);
  if (d_cnt) (void)hipFree(d_cnt);
  d_list = nullptr, d_qbox = nullptr, d_bbox = nullptr, d_cnt = nullptr;
  bin_off.clear(), q_off.clear();
  built = false;
}

hipError_t scatter_slots_gpu(hipStream_t st, const float4* d_packed, uint32_t m, uint32_t ns, float4* d_slots, float4* d_shade) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rf_scatter, dim3(grid(12 * (size_t)m)), dim3(kThreads), 0, st, d_packed, m, ns, d_slots, d_shade);
  return hipGetLastError();
}

hipError_t refit_tree_gpu(hipStream_t st, const RefitTree& t, bool timed, RefitPlan* plan, RefitTimes* out) {
  *out = RefitTimes();
  if (t.ns == 0 || t.nb == 0) return hipSuccess;
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const float4* slots = reinterpret_cast<const float4*>(t.nodes + t.nb);
  if (!plan->built) {
    if (timed) GPU_CHK(hipStreamSynchronize(st));
    const auto t0 = now();
    plan->release();
    GPU_CHK(hipMalloc((void**)&plan->d_list, 4 * ((size_t)t.nb + t.nq + 1)));
    GPU_CHK(hipMalloc((void**)&plan->d_qbox, 32 * ((size_t)t.nq + 1)));
    GPU_CHK(hipMalloc((void**)&plan->d_bbox, 32 * ((size_t)t.nb + 1)));
    GPU_CHK(hipMalloc((void**)&plan->d_cnt, 8));
    GPU_CHK(plan_levels(st, t.nodes, t.nb, 2u, plan->d_list, plan->d_cnt, &plan->bin_off));
    if (t.nq) GPU_CHK(plan_levels(st, t.q, t.nq, 4u, plan->d_list + t.nb, plan->d_cnt, &plan->q_off));
    plan->built = true;
    out->plan_ms = ms(t0, now());
  }
  const auto t1 = now();
  uint32_t* d_fail = plan->d_cnt + 1;
  GPU_CHK(hipMemsetAsync(d_fail, 0, 4, st));
  for (size_t l = plan->bin_off.size() - 1; l-- > 0;) {
    const uint32_t first = plan->bin_off[l], count = plan->bin_off[l + 1] - first;
    hipLaunchKernelGGL(k_rf_bin, dim3(grid(count)), dim3(kThreads), 0, st, t.nodes, t.nb, slots, t.ns, plan->d_bbox, plan->d_list + first, count, d_fail);
  }
  out->bin_levels = (uint32_t)plan->bin_off.size() - 1;
  if (t.nq) {
    hipLaunchKernelGGL(k_rf_pack, dim3(grid(4 * (size_t)t.nq)), dim3(kThreads), 0, st, t.q, t.nq, slots, t.ns, t.tri_pairs ? 1u : 0u, t.tri,
                       (uint32_t)t.tri_words, t.pts, t.hit, (uint32_t)t.npts, d_fail);
    for (size_t l = plan->q_off.size() - 1; l-- > 0;) {
      const uint32_t first = plan->q_off[l], count = plan->q_off[l + 1] - first;
      hipLaunchKernelGGL(k_rf_q, dim3(grid(count)), dim3(kThreads), 0, st, t.q, t.nq, slots, t.ns, t.tri_pairs ? 1u : 0u, t.tri, (uint32_t)t.tri_words,
                         t.hit, (uint32_t)t.npts, plan->d_qbox, plan->d_list + t.nb + first, count, d_fail);
    }
    out->q_levels = (uint32_t)plan->q_off.size() - 1;
  }
  GPU_CHK(hipGetLastError());
  GPU_CHK(hipMemcpyAsync(&out->failed, d_fail, 4, hipMemcpyDeviceToHost, st));
  GPU_CHK(hipStreamSynchronize(st));  // (the flag decides whether the scene may be used: the one synchronise of the trees)
  out->trees_ms = ms(t1, now());
  return hipSuccess;
}

}  // namespace pb
