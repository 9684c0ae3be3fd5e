// temporal.hip -- motion vectors across a refit and the reprojecting accumulation (pbrhip_render_motion, pbrhip_temporal_accumulate,
// DESIGN.md §16).
//
// k_motion: lane = pixel, k_features' shape (features.hip): the pixel-centre pinhole ray of the current camera (dcamera_pixel.h) -> the
// one-ray-per-lane traversal (dtrace.h::traverse, the first kSimpleLdsStack stack entries in LDS, the rest in the spill area) ->
// make_surface for the guide; then the hit's barycentrics applied to the SNAPSHOT's slot (a refit keeps slot order) and that point
// projected through the snapshot's camera.  k_temporal: lane = pixel, four 16-byte gathers from each of the two history images.
// A translation unit of its own: the render kernels' code objects do not depend on it.
#include <type_traits>

#include "dcamera_pixel.h"
#include "dshade.h"
#include "feature_kernels.h"
#include "temporal_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_motion(DScene sc, MotionArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  TravStats st = {};
  uint32_t overflow = 0u;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.npix; j += gridDim.x * kBlock) {
    const uint32_t gpix = a.pix[j];
    const uint32_t x = gpix % a.width, y = gpix / a.width;
    V3 o, d;
    if (a.user) user_camera_ray_at(a.ucam, x, y, a.width, a.height, 0.5f, 0.5f, o, d);
    else reference_camera_ray_at(a.cam, x, y, 0.5f, 0.5f, o, d);
    Hit h;
    traverse<false, false, CURVES, WIDE>(sc, o, d, 0.0f, kInf, h, stk + threadIdx.x, kBlock, st, &overflow,
                                         a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
    float4 M = make_float4(0.f, 0.f, 0.f, 0.f), G = M;
    uint4 I = make_uint4(kNone, 0u, 0u, 0u);
    if (h.slot != kNone) {
      const uint32_t slot = h.slot & kHitSlotMask;
      const Surface s = make_surface(sc, o, d, h);
      const bool curve = (s.flags & kSlotIsCurve) != 0;
      V3 n = s.n_s;
      if (!curve && dot(d, n) > 0.0f) n = -n;  // towards the viewer; a curve's tangent stays as it is
      G = make_float4(n.x, n.y, n.z, h.t);
      I = make_uint4(slot, __float_as_uint(h.u), __float_as_uint(h.v), __float_as_uint(h.t));
      if (a.motion) {
        const float4* ps = a.prev_slots + 4 * (size_t)slot;
        const float4 w0 = ps[0], w1 = ps[1], w2 = ps[2];
        V3 X;
        if (curve) {  // the piece's axis: a = B(sub / 4), b = B((sub + 1) / 4) of the snapshot, at the piece's own parameter 4 u - sub
          const float sp = h.u * 4.0f - (float)__float_as_uint(w2.x);
          X = ld3(w0) + sp * (ld3(w1) - ld3(w0));
        } else {
          X = lerp3(ld3(w0), ld3(w1), ld3(w2), h.u, h.v);
        }
        float px, py, dist;
        const bool front = a.user_prev ? user_camera_project(a.ucam_prev, a.width, a.height, X, px, py, dist)
                                       : reference_camera_project(a.cam_prev, X, px, py, dist);
        if (front) M = make_float4(px - ((float)x + 0.5f), py - ((float)y + 0.5f), dist, curve ? kMotionCurve : 1.0f);
      }
    }
    if (a.motion) a.motion[gpix] = M;
    if (a.guide) a.guide[gpix] = G;
    if (a.ident) a.ident[gpix] = I;
  }
  if (overflow) *a.overflow = 1u;
}

// the <CURVES, WIDE> of launch_features (features.hip)
void launch_motion(hipStream_t s, const DScene& sc, const MotionArgs& a, const Knobs& k) {
  if (!a.npix) return;
  const uint32_t g = feature_grid<kBlock>(a.npix);
  with_hook_tree([&](auto c, auto w) { hipLaunchKernelGGL((k_motion<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, sc, k);
}

// ------------------------------------------------------------------ k_temporal
// The definition is include/pbrhip.h's (pbrhip_temporal_accumulate); float32, every operation rounded once, the taps in the order
// (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).
__global__ __launch_bounds__(kBlock) void k_temporal(TemporalArgs a) {
  const size_t npx = (size_t)a.width * a.height;
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < npx; p += (size_t)gridDim.x * kBlock) {
    const uint32_t cnt = a.count[p];
    if (cnt == 0u) {
      a.out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const float4 sum = a.rgba[p];
    const float fc = (float)cnt;
    const float cr = sum.x / fc, cg = sum.y / fc, cb = sum.z / fc;
    float4 out = make_float4(cr, cg, cb, 1.0f);
    const float4 m = a.motion[p];
    // (a q that is NaN or beyond every image fails the comparison: no tap, no conversion of a huge float)
    const float qx = (float)(uint32_t)(p % a.width) + m.x, qy = (float)(uint32_t)(p / a.width) + m.y;
    if (a.hist_rgba && m.w != 0.0f && fabsf(qx) < 2.0e9f && fabsf(qy) < 2.0e9f) {
      const float4 g = a.guide[p];
      const float x0f = floorf(qx), y0f = floorf(qy);
      const float fx = qx - x0f, fy = qy - y0f;
      const long long x0 = (long long)x0f, y0 = (long long)y0f;
      const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
      const bool curve = m.w == kMotionCurve;
      float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const long long tx = x0 + (t & 1), ty = y0 + (t >> 1);
        if (tx < 0 || ty < 0 || tx >= (long long)a.width || ty >= (long long)a.height) continue;
        const size_t q = (size_t)ty * a.width + (size_t)tx;
        const float4 H = a.hist_rgba[q], HG = a.hist_guide[q];
        float nd = HG.x * g.x + HG.y * g.y + HG.z * g.z;
        if (curve) nd = fabsf(nd);
        const bool ok = H.w > 0.0f && HG.w > 0.0f && fabsf(HG.w - m.z) <= a.sigma_depth * m.z && nd >= a.normal_cos_min;
        if (!ok) continue;
        const float w = wx[t & 1] * wy[t >> 1];
        S += w, hr += w * H.x, hg += w * H.y, hb += w * H.z, hn += w * H.w;
      }
      if (S > 0.0f) {
        hr = hr / S, hg = hg / S, hb = hb / S, hn = hn / S;
        const float len = __builtin_fminf(hn + 1.0f, a.max_history);
        const float al = __builtin_fmaxf(1.0f / len, a.alpha_min);
        out = make_float4(hr + al * (cr - hr), hg + al * (cg - hg), hb + al * (cb - hb), len);
      }
    }
    a.out[p] = out;
  }
}

void launch_temporal(hipStream_t s, const TemporalArgs& a) {
  const size_t npx = (size_t)a.width * a.height;
  if (!npx) return;
  const size_t g = (npx + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_temporal, dim3((uint32_t)(g < 8192 ? g : 8192)), dim3(kBlock), 0, s, a);
}

}  // namespace pb
