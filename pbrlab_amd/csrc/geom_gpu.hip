// geom_gpu.hip -- device geometry mode (geom_gpu.h; DESIGN.md section 8, "Staging on the device"): the dirty instances' slots, ShadeRecs
// and bounds re-derived ON THE DEVICE from the library's device copy of the meshes, instead of commit.cpp::slot_and_shade and
// scene_bounds on the host followed by a packed upload.
//
// The topology is fixed between commits, so the slot and the ShadeRec already on the device hold everything that does not depend on
// positions: instance / geom / prim ids, gid, lightrec, matflags, texcoords, the routing bits (.w of the slot's third word) and a curve
// piece's `sub` (.x of it).  k_dg_stage reads those and rewrites in place exactly what slot_and_shade derives from positions, with the
// functions the host calls (dmath.h, geom_math.h: IEEE single precision, no contraction, correctly rounded divide and square root):
//
//   triangle     slot words 0..2: the world corners (xf_point unless the instance's matrix is the identity as bits); ShadeRec: ng,
//                ns_flat of the LOCAL corners and, with kSlotHasNormals, the three corner normals
//   curve piece  slot words 0..1: the end points of piece `sub` of the world control points (curve_piece); ShadeRec words 8..23: the
//                LOCAL control points
//
// and per instance two boxes: the LOCAL one of commit.cpp::scene_bounds (triangles by the corners their faces use, a curve by the hull
// of its four control points widened by their largest |r|) and the WORLD one, the union of slot_tight_box over its slots.  A block
// reduces its bounds on an order-preserving integer encoding of the float and combines them with one atomic minimum / maximum per bound:
// over finite floats neither depends on the order.  (A bound over both zeros is -0 as a minimum and +0 as a maximum here; the host's
// fminf chain gives whichever came last.)
//
// Kernels: k_dg_check (the caller's array: finite?  and the library's copy of it), k_dg_init (the bounds' neutral elements), k_dg_stage
// (one thread per slot of ONE dirty instance: a launch per dirty instance).  Every index taken from a table is checked against its
// array's size before it is used; one out of range sets the flag and the thread writes nothing.
#include <hip/hip_runtime.h>
#include <math.h>

#include "dscene.h"
#include "geom_gpu.h"
#include "geom_math.h"

namespace pb {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// floats ordered as unsigned integers: negative values reversed below the positive ones (-0 < +0)
__device__ __forceinline__ uint32_t dg_encode(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

}  // namespace

// (the kernels have external names: the code-object tables of the tests list them by name)
__global__ void __launch_bounds__(kThreads) k_dg_check(const float4* __restrict__ src, size_t n, float4* __restrict__ dst, uint32_t* flag) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float4 v = src[t];
  if (dst) dst[t] = v;
  if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(kThreads) k_dg_init(uint32_t* bounds, uint32_t ninst) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ninst * kDgBoundWords) return;
  const uint32_t w = t % kDgBoundWords;
  bounds[t] = dg_encode((w < 3u || (w >= 6u && w < 9u)) ? INFINITY : -INFINITY);
}

__global__ void __launch_bounds__(kThreads) k_dg_stage(DgScene d, uint32_t inst, uint32_t first, uint32_t count) {
  __shared__ uint32_t part[kWaves][kDgBoundWords];
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  // local lo, local hi, world lo, world hi of this thread's primitive (the neutral elements for a thread without one)
  float bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY};
  float wl[3] = {INFINITY, INFINITY, INFINITY}, wh[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  const uint32_t slot = e < count ? d.slot_list[first + e] : kNone;
  if (e < count && slot >= d.ns) bad = true;
  if (e < count && !bad) {
    float4* sl = d.slots + 4 * (size_t)slot;
    float4* sr = d.shade + 8 * (size_t)slot;
    const float4 s0 = sr[0], ids = sr[6];  // (ng, matflags); (gid, instance, geom, prim)
    const uint32_t flags = __float_as_uint(s0.w) >> 24, geom = __float_as_uint(ids.z), prim = __float_as_uint(ids.w);
    const DgXf& X = d.xf[inst];
    const bool identity = X.identity != 0;
    const uint32_t ig = d.ig_off[inst] + geom;
    const uint32_t mesh = ig < d.ngeoms ? d.geom_mesh[ig] : kNone;
    if (__float_as_uint(ids.y) != inst || mesh == kNone) bad = true;
    if (!bad) {
      const DgMeshRec r = d.recs[mesh];
      if (!(flags & kSlotIsCurve)) {
        uint32_t vi[3] = {0, 0, 0};
        if ((size_t)prim * 3 + 2 < r.nidx) {
#pragma unroll
          for (int c = 0; c < 3; c++) vi[c] = d.vidx[r.idx_off + prim * 3 + c];
        } else bad = true;
        if (vi[0] >= r.nverts || vi[1] >= r.nverts || vi[2] >= r.nverts) bad = true;
        uint32_t ni[3] = {0, 0, 0};
        if (!bad && (flags & kSlotHasNormals)) {
#pragma unroll
          for (int c = 0; c < 3; c++) ni[c] = d.nidx[r.nid_off + prim * 3 + c];
          if (ni[0] >= r.nnorm || ni[1] >= r.nnorm || ni[2] >= r.nnorm) bad = true;
        }
        if (!bad) {
          V3 v[3], w[3];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const float4 p = d.verts[r.vert_off + vi[c]];
            v[c] = V3(p.x, p.y, p.z);
            w[c] = identity ? v[c] : xf_point(X.m, v[c]);
          }
          const float route = sl[2].w;
          sl[0] = make_float4(w[0].x, w[0].y, w[0].z, 0.f);
          sl[1] = make_float4(w[1].x, w[1].y, w[1].z, 0.f);
          sl[2] = make_float4(w[2].x, w[2].y, w[2].z, route);
          const V3 ng = normalize_raw(cross(v[1] - v[0], v[2] - v[0]));
          const V3 nf = vnormalize(cross(v[1] - v[0], v[2] - v[1]));  // CalcGeometryNormal, triangle-mesh.cc:181-184
          const float4 s1 = sr[1];
          sr[0] = make_float4(ng.x, ng.y, ng.z, s0.w);
          sr[1] = make_float4(nf.x, nf.y, nf.z, s1.w);
          if (flags & kSlotHasNormals) {
            const float4 n0 = d.normals[r.norm_off + ni[0]], n1 = d.normals[r.norm_off + ni[1]], n2 = d.normals[r.norm_off + ni[2]];
            const float4 s4 = sr[4];  // (n[8], pad0, uv[0], uv[1])
            sr[2] = make_float4(n0.x, n0.y, n0.z, n1.x);
            sr[3] = make_float4(n1.y, n1.z, n2.x, n2.y);
            sr[4] = make_float4(n2.z, s4.y, s4.z, s4.w);
          }
#pragma unroll
          for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
              bl[k] = fminf(bl[k], v[c][k]), bh[k] = fmaxf(bh[k], v[c][k]);
              wl[k] = fminf(wl[k], w[c][k]), wh[k] = fmaxf(wh[k], w[c][k]);
            }
        }
      } else {
        const uint32_t c0 = prim < r.nidx ? d.vidx[r.idx_off + prim] : kNone;
        const uint32_t sub = __float_as_uint(sl[2].x);
        if (c0 == kNone || (size_t)c0 + 4 > r.nverts || sub > 3u) bad = true;
        if (!bad) {
          float cps[16], wcps[16];
          float rmax = 0.f;
#pragma unroll
          for (int c = 0; c < 4; c++) {
            const float4 p = d.verts[r.vert_off + c0 + c];
            sr[2 + c] = p;  // the cubic itself, local: the tangent shading uses
            cps[4 * c] = p.x, cps[4 * c + 1] = p.y, cps[4 * c + 2] = p.z, cps[4 * c + 3] = p.w;
            V3 q(p.x, p.y, p.z);
            if (!identity) q = xf_point(X.m, q);
            wcps[4 * c] = q.x, wcps[4 * c + 1] = q.y, wcps[4 * c + 2] = q.z, wcps[4 * c + 3] = p.w;  // (the radius is not scaled)
            rmax = fmaxf(rmax, fabsf(p.w));
          }
          float a[4], b[4];
          curve_piece(wcps, sub, a, b);
          sl[0] = make_float4(a[0], a[1], a[2], a[3]);
          sl[1] = make_float4(b[0], b[1], b[2], b[3]);
          const float rr = smax(fabsf(a[3]), fabsf(b[3]));
#pragma unroll
          for (int k = 0; k < 3; k++) {
            float cl = INFINITY, ch = -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; c++) cl = fminf(cl, cps[4 * c + k]), ch = fmaxf(ch, cps[4 * c + k]);
            bl[k] = cl - rmax, bh[k] = ch + rmax;
            wl[k] = smin(a[k], b[k]) - rr, wh[k] = smax(a[k], b[k]) + rr;
          }
        }
      }
    }
  }
  if (bad) {  // (its bounds stay neutral: the host refuses the refit on the flag)
    atomicOr(d.flag, 2u);
#pragma unroll
    for (int k = 0; k < 3; k++) bl[k] = wl[k] = INFINITY, bh[k] = wh[k] = -INFINITY;
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t a = wave_min(dg_encode(bl[k])), b = wave_max(dg_encode(bh[k]));
    const uint32_t c = wave_min(dg_encode(wl[k])), f = wave_max(dg_encode(wh[k]));
    if (lane == 0) part[wave][k] = a, part[wave][3 + k] = b, part[wave][6 + k] = c, part[wave][9 + k] = f;
  }
  __syncthreads();
  if (threadIdx.x < kDgBoundWords) {
    const uint32_t w = threadIdx.x;
    const bool is_min = w < 3u || (w >= 6u && w < 9u);
    uint32_t v = part[0][w];
#pragma unroll
    for (int i = 1; i < kWaves; i++) v = is_min ? min(v, part[i][w]) : max(v, part[i][w]);
    uint32_t* dst = d.bounds + (size_t)inst * kDgBoundWords + w;
    if (is_min) atomicMin(dst, v);
    else atomicMax(dst, v);
  }
}

hipError_t dg_check_gpu(hipStream_t st, const void* src, size_t n, float4* dst, uint32_t* flag) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_dg_check, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, reinterpret_cast<const float4*>(src), n, dst, flag);
  return hipGetLastError();
}
hipError_t dg_init_bounds_gpu(hipStream_t st, uint32_t* bounds, uint32_t ninst) {
  if (!ninst) return hipSuccess;
  hipLaunchKernelGGL(k_dg_init, dim3((ninst * kDgBoundWords + kThreads - 1) / kThreads), dim3(kThreads), 0, st, bounds, ninst);
  return hipGetLastError();
}
hipError_t dg_stage_gpu(hipStream_t st, const DgScene& d, uint32_t inst, uint32_t first, uint32_t count) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(k_dg_stage, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d, inst, first, count);
  return hipGetLastError();
}

}  // namespace pb
