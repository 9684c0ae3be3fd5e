// qtree_gpu.hip -- the binary tree of the GPU builder (bvh_gpu.hip) collapsed ON THE DEVICE into the 4-wide quantised tree the
// production traversal kernels read (dscene.h::QNode, TriPair leaves, curve records, q_hitcode): builder PBRHIP_BVH_GPU_LBVH_WIDE.
// The host collapse (bvh_build.cpp::build_qtree) chooses frontiers bottom-up by dynamic programming; this one is a greedy rule
// that every binary node can evaluate on its own ("The collapse, exactly"; tests/_qcollapse_model.py restates it):
//
//   heads     binary node 0 is a head.  The frontier F of a head starts as its children (without kEmptyChild); while |F| < 4 and F has
//             an inner member, the inner member with the largest area A = dx*dy + dy*dz + dz*dx (float32, each step rounded; ties:
//             the earliest) is replaced in place by its two children.  The inner members of the final F are heads.
//   numbering heads in ascending binary index are Q nodes 0, 1, ...; child i of a Q node is F[i]
//   leaves    one record per leaf reference of the binary tree, records of a kind in ascending order of the leaf's first slot
//
// Kernels: k_qc_mark (one launch per level of the Q tree: the frontier of every head of the level marks the heads below it and the
// leaves' slots), two rocPRIM scans (head numbers; record offsets), k_qc_emit (frontier again, quantised by qquant.h, references
// renumbered), k_qc_pack (leaf records from the slots behind the binary nodes).  No kernel waits for another block: a dependency
// between levels is a new launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <chrono>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "host_scene.h"
#include "qquant.h"

namespace pb {
namespace {

constexpr int kThreads = 256;

// per-slot mark: bits 0..1 = primitives of the leaf that STARTS at this slot (0: none starts here), bit 2 = the slot is a curve piece
constexpr uint32_t kMarkCurve = 4u;

__device__ __forceinline__ QBox child_box(const BvhNode& nd, int c) {
  QBox b;
  for (int a = 0; a < 3; a++) b.lo[a] = nd.lo[a][c], b.hi[a] = nd.hi[a][c];
  return b;
}
__device__ __forceinline__ float box_area(const QBox& b) {
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  return dx * dy + dy * dz + dz * dx;
}
__device__ __forceinline__ QBox pick(bool s, const QBox& x, const QBox& y) {
  QBox b;
  for (int a = 0; a < 3; a++) b.lo[a] = s ? x.lo[a] : y.lo[a], b.hi[a] = s ? x.hi[a] : y.hi[a];
  return b;
}

// The frontier of binary node v: references of the binary tree and the boxes their parents store.  Every index below is a
// compile-time constant after unrolling (the arrays live in registers).  An inner child beyond the tree (never in a valid tree) is not
// expanded.
__device__ __forceinline__ int frontier(const BvhNode* __restrict__ nodes, uint32_t nb, uint32_t v, uint32_t ref[4], QBox box[4]) {
  const BvhNode nd = nodes[v];
  const bool e0 = nd.c0 == kEmptyChild, e1 = nd.c1 == kEmptyChild;
  const QBox b0 = child_box(nd, 0), b1 = child_box(nd, 1);
  ref[0] = e0 ? nd.c1 : nd.c0, box[0] = pick(e0, b1, b0);
  ref[1] = (e0 || e1) ? kEmptyChild : nd.c1, box[1] = b1;
  ref[2] = ref[3] = kEmptyChild, box[2] = box[3] = b1;
  int n = 2 - (e0 ? 1 : 0) - (e1 ? 1 : 0);
#pragma unroll
  for (int step = 0; step < 3; step++) {
    int m = -1;
    float best = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float A = box_area(box[i]);
      if (i < n && !(ref[i] & kLeafBit) && ref[i] < nb && (m < 0 || A > best)) m = i, best = A;
    }
    if (n >= 4 || m < 0) break;
    const uint32_t u = m == 0 ? ref[0] : (m == 1 ? ref[1] : ref[2]);
    const BvhNode cn = nodes[u];
    const QBox c0 = child_box(cn, 0), c1 = child_box(cn, 1);
#pragma unroll
    for (int i = 3; i >= 0; i--) {
      if (i == m) ref[i] = cn.c0, box[i] = c0;
      else if (i == m + 1) ref[i] = cn.c1, box[i] = c1;
      else if (i > m + 1) ref[i] = ref[i > 0 ? i - 1 : 0], box[i] = box[i > 0 ? i - 1 : 0];
    }
    n++;
  }
  return n;
}

}  // namespace

// (the kernels have external names: the code-object tables of the tests list them by name)
// One level of the Q tree: head qin[i] marks the inner members of its frontier as heads (they are the next level: qout) and the slots
// of its leaves (lmark).  A node has one parent, so nothing is written twice; the exchange only keeps a broken tree from looping.
__global__ void __launch_bounds__(kThreads) k_qc_mark(const BvhNode* __restrict__ nodes, uint32_t nb, uint32_t ns, const uint32_t* __restrict__ qin, uint32_t nin,
                          uint32_t* qout, uint32_t* nout, uint32_t* flag, uint32_t* lmark) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nin) return;
  uint32_t ref[4];
  QBox box[4];
  const int n = frontier(nodes, nb, qin[i], ref, box);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k >= n) continue;
    const uint32_t r = ref[k];
    if (r & kLeafBit) {
      const uint32_t first = (r & 0x3FFFFFFFu) >> 3, count = (r & 7u) + 1u, curve = (r & kCurveBit) ? kMarkCurve : 0u;
      if (count <= 2u && first + count <= ns) {
        lmark[first] = count | curve;
        if (count == 2u) lmark[first + 1] = curve;
      }
    } else if (r < nb && atomicExch(&flag[r], 1u) == 0u) {
      const uint32_t at = atomicAdd(nout, 1u);
      if (at < nb) qout[at] = r;
    }
  }
}

// what a slot adds to the two record counters: triangle records in the high word (TriPair scenes: one per leaf; scenes with curves: one
// 48-byte slot per triangle), curve records in the low word
struct MarkToCount {
  uint32_t tri_pairs;
  __host__ __device__ unsigned long long operator()(uint32_t m) const {
    const bool curve = (m & kMarkCurve) != 0u, start = (m & 3u) != 0u;
    const unsigned long long tri = curve ? 0ull : ((tri_pairs ? start : true) ? 1ull : 0ull);
    return (tri << 32) | ((curve && start) ? 1ull : 0ull);
  }
};

__device__ __forceinline__ uint32_t slot_code(const float4* __restrict__ slots, uint32_t k) {  // slot | routing bits
  return k | __float_as_uint(slots[4 * (size_t)k + 2].w);
}

__global__ void __launch_bounds__(kThreads) k_qc_emit(const BvhNode* __restrict__ nodes, uint32_t nb, uint32_t ns, const float4* __restrict__ slots,
                          const uint32_t* __restrict__ flag, const uint32_t* __restrict__ qidx,
                          const unsigned long long* __restrict__ rec, QNode* out, uint32_t nq, uint32_t* fail) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nb || !flag[v]) return;
  const uint32_t q = qidx[v];
  if (q >= nq) return;
  uint32_t ref[4];
  QBox box[4];
  const int n = frontier(nodes, nb, v, ref, box);
  QNode nd;
  if (n == 0 || !quantise_node(box, n, &nd)) atomicOr(fail, 1u);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t r = kEmptyChild;
    if (k < n) {
      r = ref[k];
      if (!(r & kLeafBit)) {
        r = r < nb ? qidx[r] : 0u;
      } else {
        const uint32_t first = (r & 0x3FFFFFFFu) >> 3, count = (r & 7u) + 1u;
        if (first + count > ns) {
          atomicOr(fail, 2u);
        } else if (r & kCurveBit) {
          const uint32_t P = 4u + 4u * (uint32_t)(rec[first] & 0xFFFFFFFFull);
          const uint32_t sa = __float_as_uint(slots[4 * (size_t)first + 2].x) & 3u;
          const uint32_t sb = count == 2u ? (__float_as_uint(slots[4 * (size_t)(first + 1) + 2].x) & 3u) : 0u;
          r = kLeafBit | kCurveBit | ((P | sa) << 3) | (count == 2u ? (kCurvePairBit | sb) : 0u);
        } else {
          r = kLeafBit | ((uint32_t)(rec[first] >> 32) << 3) | (count - 1u);
        }
      }
    }
    nd.c[k] = r;
  }
  out[q] = nd;
}

// leaf records: tri = the triangle area (TriPair of five words per leaf, or three words per triangle), pts / hit = the curve records
__global__ void __launch_bounds__(kThreads) k_qc_pack(uint32_t ns, const float4* __restrict__ slots, const uint32_t* __restrict__ lmark,
                          const unsigned long long* __restrict__ rec, uint32_t tri_pairs, float4* tri, float4* pts, uint32_t* hit) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ns) return;
  const uint32_t m = lmark[k], count = m & 3u;
  const float4* a = slots + 4 * (size_t)k;
  if (m & kMarkCurve) {
    if (!count) return;
    const uint32_t P = 4u + 4u * (uint32_t)(rec[k] & 0xFFFFFFFFull);
    pts[P] = a[0], pts[P + 1] = a[1];
    hit[P] = slot_code(slots, k);
    if (count == 2u) {
      pts[P + 2] = a[4], pts[P + 3] = a[5];
      hit[P + 2] = slot_code(slots, k + 1);
    }
    return;
  }
  const uint32_t r = (uint32_t)(rec[k] >> 32);
  if (!tri_pairs) {
    float4 w2 = a[2];
    w2.w = __uint_as_float(slot_code(slots, k));
    tri[3 * (size_t)r] = a[0], tri[3 * (size_t)r + 1] = a[1], tri[3 * (size_t)r + 2] = w2;
    return;
  }
  if (!count) return;
  const float4* b = count == 2u ? a + 4 : a;  // (one triangle: stored twice, the copy is no candidate)
  const float ca = __uint_as_float(slot_code(slots, k)), cb = __uint_as_float(count == 2u ? slot_code(slots, k + 1) : kNone);
  const float4 a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
  float4* o = tri + kTriPairWords * (size_t)r;
  o[0] = make_float4(a0.x, b0.x, a0.y, b0.y), o[1] = make_float4(a0.z, b0.z, a1.x, b1.x), o[2] = make_float4(a1.y, b1.y, a1.z, b1.z);
  o[3] = make_float4(a2.x, b2.x, a2.y, b2.y), o[4] = make_float4(a2.z, b2.z, ca, cb);
}

namespace {

#define GPU_CHK(x)                   \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return e_; \
  } while (0)

template <typename T>
struct Tmp {
  T* p = nullptr;
  ~Tmp() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)); }
};

}  // namespace

hipError_t collapse_qtree_gpu(hipStream_t st, const BvhNode* d_nodes, uint32_t n, const float4* d_slots, bool tri_pairs,
                              const std::function<hipError_t(size_t, size_t, float4**, uint32_t**)>& alloc, QCollapse* out) {
  *out = QCollapse();
  if (n == 0) return hipSuccess;
  const uint32_t nb = n > 1 ? n - 1 : 1, ns = n;
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto t0 = now();
  Tmp<uint32_t> d_flag, d_qidx, d_lmark, d_queue, d_cnt;
  Tmp<unsigned long long> d_rec;
  GPU_CHK(d_flag.alloc((size_t)nb + 1)); GPU_CHK(d_qidx.alloc((size_t)nb + 1)); GPU_CHK(d_lmark.alloc((size_t)ns + 1));
  GPU_CHK(d_queue.alloc(2 * (size_t)nb)); GPU_CHK(d_cnt.alloc(2)); GPU_CHK(d_rec.alloc((size_t)ns + 1));
  out->alloc_ms += ms(t0, now());
  GPU_CHK(hipMemsetAsync(d_flag.p, 0, 4 * ((size_t)nb + 1), st));
  GPU_CHK(hipMemsetAsync(d_lmark.p, 0, 4 * ((size_t)ns + 1), st));
  GPU_CHK(hipMemsetAsync(d_cnt.p, 0, 8, st));
  const uint32_t root[1] = {0u}, one[1] = {1u};
  GPU_CHK(hipMemcpyAsync(d_queue.p, root, 4, hipMemcpyHostToDevice, st));
  GPU_CHK(hipMemcpyAsync(d_flag.p, one, 4, hipMemcpyHostToDevice, st));
  // the heads, level by level: every launch is sized by the exact count of the level before it
  uint32_t nin = 1, side = 0;
  for (uint32_t level = 0; nin > 0 && level <= nb; level++) {
    uint32_t* qin = d_queue.p + (size_t)side * nb;
    uint32_t* qout = d_queue.p + (size_t)(1 - side) * nb;
    hipLaunchKernelGGL(k_qc_mark, dim3((nin + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_nodes, nb, ns, qin, nin, qout, d_cnt.p,
                       d_flag.p, d_lmark.p);
    GPU_CHK(hipGetLastError());
    GPU_CHK(hipMemcpyAsync(&nin, d_cnt.p, 4, hipMemcpyDeviceToHost, st));
    GPU_CHK(hipMemsetAsync(d_cnt.p, 0, 4, st));
    GPU_CHK(hipStreamSynchronize(st));
    nin = nin < nb ? nin : nb;
    side = 1 - side;
    out->levels = level + 1;
  }
  // head numbers and record offsets
  size_t tmp_a = 0, tmp_b = 0;
  auto counts = rocprim::make_transform_iterator(d_lmark.p, MarkToCount{tri_pairs ? 1u : 0u});
  GPU_CHK(rocprim::exclusive_scan(nullptr, tmp_a, d_flag.p, d_qidx.p, 0u, (size_t)nb + 1, rocprim::plus<uint32_t>(), st));
  GPU_CHK(rocprim::exclusive_scan(nullptr, tmp_b, counts, d_rec.p, 0ull, (size_t)ns + 1, rocprim::plus<unsigned long long>(), st));
  Tmp<unsigned char> d_tmp;
  t0 = now();
  GPU_CHK(d_tmp.alloc(tmp_a > tmp_b ? tmp_a : tmp_b));
  out->alloc_ms += ms(t0, now());
  GPU_CHK(rocprim::exclusive_scan(d_tmp.p, tmp_a, d_flag.p, d_qidx.p, 0u, (size_t)nb + 1, rocprim::plus<uint32_t>(), st));
  GPU_CHK(rocprim::exclusive_scan(d_tmp.p, tmp_b, counts, d_rec.p, 0ull, (size_t)ns + 1, rocprim::plus<unsigned long long>(), st));
  uint32_t nq = 0;
  unsigned long long recs = 0;
  GPU_CHK(hipMemcpyAsync(&nq, d_qidx.p + nb, 4, hipMemcpyDeviceToHost, st));
  GPU_CHK(hipMemcpyAsync(&recs, d_rec.p + ns, 8, hipMemcpyDeviceToHost, st));
  GPU_CHK(hipStreamSynchronize(st));
  const size_t ntri = (size_t)(recs >> 32), ncurve = (size_t)(recs & 0xFFFFFFFFull);
  size_t tri_words = ntri * (tri_pairs ? (size_t)kTriPairWords : 3u);
  tri_words = (tri_words + 3u) & ~(size_t)3u;  // (q_pt0 a multiple of 4: the low bits of a curve record's address are free)
  const size_t npts = 4 + 4 * ncurve + 4;      // points 0..3 zero, one 64-byte record per curve leaf, four zero points
  out->nodes = nq, out->tri_words = tri_words, out->pts = npts;
  if (ntri >= (1u << 27) || npts >= (1u << 27)) return hipSuccess;  // (a record index beyond its reference's bits: fits stays false)
  out->fits = true;
  float4* d_wide = nullptr;
  uint32_t* d_hit = nullptr;
  t0 = now();
  GPU_CHK(alloc((size_t)nq * 4 + tri_words + npts, npts, &d_wide, &d_hit));
  out->alloc_ms += ms(t0, now());
  float4* d_tri = d_wide + (size_t)nq * 4;
  float4* d_pts = d_tri + tri_words;
  GPU_CHK(hipMemsetAsync(d_tri, 0, 16 * (tri_words + npts), st));
  GPU_CHK(hipMemsetAsync(d_hit, 0xFF, 4 * npts, st));  // kNone wherever no piece starts
  hipLaunchKernelGGL(k_qc_emit, dim3((nb + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_nodes, nb, ns, d_slots, d_flag.p, d_qidx.p,
                     d_rec.p, reinterpret_cast<QNode*>(d_wide), nq, d_cnt.p + 1);
  hipLaunchKernelGGL(k_qc_pack, dim3((ns + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ns, d_slots, d_lmark.p, d_rec.p,
                     tri_pairs ? 1u : 0u, d_tri, d_pts, d_hit);
  GPU_CHK(hipGetLastError());
  uint32_t failed = 0;
  GPU_CHK(hipMemcpyAsync(&failed, d_cnt.p + 1, 4, hipMemcpyDeviceToHost, st));
  GPU_CHK(hipStreamSynchronize(st));
  out->quantised = failed == 0;
  return hipSuccess;
}

}  // namespace pb
