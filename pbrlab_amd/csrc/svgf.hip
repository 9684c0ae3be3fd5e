// svgf.hip -- spatiotemporal variance-guided filtering (Schied et al. 2017) beside temporal.hip and denoise.hip: pbrhip_scene_object_ids,
// pbrhip_svgf_accumulate, pbrhip_svgf_filter.
//
//   k_object_ids        lane = pixel: one gather of a ShadeRec word through the identity buffer's slot, the slot checked against the scene's
//   k_svgf_accumulate   k_temporal's taps and acceptance (temporal.hip) on albedo-demodulated illumination, one more test (the object id)
//                       and one more channel: the exponentially weighted central variance of the luminance
//   k_svgf_prepare      illum, var -> one float4 image e(0).rgb | v(0); v < 0 marks a pixel that is not live.  A pixel younger than four
//                       frames takes its variance from its 7 x 7 neighbourhood instead
//   k_svgf_iteration    e(i), v(i) -> e(i+1), v(i+1) with step 2^i over denoise.hip's 25 taps, the luminance weight scaled by the 3 x 3
//                       Gaussian of v(i); the first one also writes the feedback image, the last one multiplies the albedo back
//
// A tap reads 16 bytes of e | v, 16 bytes of the caller's guide and 4 bytes of the caller's ids: nothing is copied that is already an
// image.  denoise.hip's shape: a thread per pixel, 64 x 4 tiles, one launch per iteration, nothing returns to the host in between.
// All arithmetic is float32 without contraction, in the order include/pbrhip.h states; exp is the library's (f_exp).
#include "dmath.h"
#include "svgf_kernels.h"
#include "temporal_kernels.h"

namespace pb {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 4;
constexpr float kLumEps = 1e-4f;  // PBRHIP_SVGF_LUM_EPS

__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// max(a_p, 1e-3) with denoise.hip's a_p: (sum of albedo + one white per miss) / samples; 1 without features or without samples
__device__ __forceinline__ V3 clamped_albedo(const float4* __restrict__ albedo_hits, const uint32_t* __restrict__ feature_count, size_t p) {
  if (!albedo_hits) return V3(1.0f);
  const uint32_t m = feature_count[p];
  if (m == 0u) return V3(1.0f);
  const float4 ah = albedo_hits[p];
  const float fm = (float)m, miss = fm - ah.w;
  return V3(smax((ah.x + miss) / fm, 1e-3f), smax((ah.y + miss) / fm, 1e-3f), smax((ah.z + miss) / fm, 1e-3f));
}

// ------------------------------------------------------------------ k_object_ids
__global__ __launch_bounds__(kBlock) void k_object_ids(const uint32_t* __restrict__ shade_words, uint32_t num_slots, const uint32_t* __restrict__ ident,
                                                       size_t npx, uint32_t word, uint32_t* __restrict__ ids) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < npx; p += (size_t)gridDim.x * kBlock) {
    const uint32_t slot = ident[4 * p];
    // the buffer is the caller's: a slot the scene does not have (kNone, the miss, among them) reads nothing
    ids[p] = slot < num_slots ? shade_words[(size_t)slot * (sizeof(ShadeRec) / 4) + word] : kNone;
  }
}

void launch_object_ids(hipStream_t s, const ShadeRec* shade, uint32_t num_slots, const uint4* ident, size_t npx, uint32_t what, uint32_t* ids) {
  if (!npx) return;
  const size_t g = (npx + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_object_ids, dim3((uint32_t)(g < 8192 ? g : 8192)), dim3(kBlock), 0, s, reinterpret_cast<const uint32_t*>(shade), num_slots,
                     reinterpret_cast<const uint32_t*>(ident), npx, 24u + what, ids);
}

// ------------------------------------------------------------------ k_svgf_accumulate
// k_temporal (temporal.hip) statement for statement where the two agree: without ids and albedo out_illum is its out, bit for bit.
__global__ __launch_bounds__(kBlock) void k_svgf_accumulate(SvgfAccumArgs a) {
  const size_t npx = (size_t)a.width * a.height;
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < npx; p += (size_t)gridDim.x * kBlock) {
    const uint32_t cnt = a.count[p];
    if (cnt == 0u) {
      a.out_illum[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      a.out_var[p] = 0.0f;
      continue;
    }
    const float4 sum = a.rgba[p];
    const float fc = (float)cnt;
    const V3 al3 = clamped_albedo(a.albedo_hits, a.feature_count, p);
    const float er = (sum.x / fc) / al3.x, eg = (sum.y / fc) / al3.y, eb = (sum.z / fc) / al3.z;
    float4 out = make_float4(er, eg, eb, 1.0f);
    float var = 0.0f;
    const float4 m = a.motion[p];
    const float qx = (float)(uint32_t)(p % a.width) + m.x, qy = (float)(uint32_t)(p / a.width) + m.y;
    if (a.hist_illum && m.w != 0.0f && fabsf(qx) < 2.0e9f && fabsf(qy) < 2.0e9f) {
      const float4 g = a.guide[p];
      const uint32_t idp = a.ids ? a.ids[p] : 0u;
      const float x0f = floorf(qx), y0f = floorf(qy);
      const float fx = qx - x0f, fy = qy - y0f;
      const long long x0 = (long long)x0f, y0 = (long long)y0f;
      const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
      const bool curve = m.w == kMotionCurve;
      float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, hv = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const long long tx = x0 + (t & 1), ty = y0 + (t >> 1);
        if (tx < 0 || ty < 0 || tx >= (long long)a.width || ty >= (long long)a.height) continue;
        const size_t q = (size_t)ty * a.width + (size_t)tx;
        const float4 H = a.hist_illum[q], HG = a.hist_guide[q];
        float nd = HG.x * g.x + HG.y * g.y + HG.z * g.z;
        if (curve) nd = fabsf(nd);
        bool ok = H.w > 0.0f && HG.w > 0.0f && fabsf(HG.w - m.z) <= a.sigma_depth * m.z && nd >= a.normal_cos_min;
        if (ok && a.ids) ok = a.hist_ids[q] == idp;
        if (!ok) continue;
        const float w = wx[t & 1] * wy[t >> 1];
        S += w, hr += w * H.x, hg += w * H.y, hb += w * H.z, hn += w * H.w, hv += w * a.hist_var[q];
      }
      if (S > 0.0f) {
        hr = hr / S, hg = hg / S, hb = hb / S, hn = hn / S, hv = hv / S;
        const float len = __builtin_fminf(hn + 1.0f, a.max_history);
        const float al = __builtin_fmaxf(1.0f / len, a.alpha_min);
        const float d = lum(er, eg, eb) - lum(hr, hg, hb);
        out = make_float4(hr + al * (er - hr), hg + al * (eg - hg), hb + al * (eb - hb), len);
        var = (1.0f - al) * (hv + (al * d) * d);
      }
    }
    a.out_illum[p] = out;
    a.out_var[p] = var;
  }
}

void launch_svgf_accumulate(hipStream_t s, const SvgfAccumArgs& a) {
  const size_t npx = (size_t)a.width * a.height;
  if (!npx) return;
  const size_t g = (npx + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_svgf_accumulate, dim3((uint32_t)(g < 8192 ? g : 8192)), dim3(kBlock), 0, s, a);
}

// ------------------------------------------------------------------ the filter
// w_n and the depth term x_z of the pair (p, q) of two surfaces, denoise.hip's expressions; zr = sigma_depth z_p step |(dx, dy)|
__device__ __forceinline__ void surface_pair(const SvgfFilterArgs& a, const float4& gp, const float4& gq, float zr, float& w, float& arg) {
  w = smax(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
  for (uint32_t k = 0; k < a.normal_squarings; k++) w = w * w;
  const float dz = fabsf(gp.w - gq.w);
  if (a.sigma_depth > 0.0f && dz != 0.0f) arg = dz / zr;
}

__global__ __launch_bounds__(kTileW * kTileH) void k_svgf_prepare(SvgfFilterArgs a, float4* __restrict__ ev) {
  const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= a.width || y >= a.height) return;
  const uint32_t p = y * a.width + x;
  const float4 ip = a.illum[p];
  if (!(ip.w > 0.0f)) {
    ev[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    return;
  }
  float v = smax(a.var[p], 0.0f);  // (the sign is the mark of a pixel that is not live)
  if (ip.w < 4.0f) {
    // the spatial estimate over 7 x 7: two passes with the same weights g = w_n w_z w_id, g_p = 1
    const float4 gp = a.guide[p];
    const bool bg_p = gp.w == 0.0f;
    const uint32_t idp = a.ids ? a.ids[p] : 0u;
    const float lp = lum(ip.x, ip.y, ip.z);
    const float zden = a.sigma_depth * gp.w;
    float m = lp;
    for (int pass = 0; pass < 2; pass++) {
      float num = 0.0f, den = 1.0f;
      if (pass == 1) num = (lp - m) * (lp - m);
      for (int dy = -3; dy <= 3; dy++) {
        const int64_t qy = (int64_t)y + dy;
        if (qy < 0 || qy >= (int64_t)a.height) continue;
        for (int dx = -3; dx <= 3; dx++) {
          const int64_t qx = (int64_t)x + dx;
          if (qx < 0 || qx >= (int64_t)a.width || (dx == 0 && dy == 0)) continue;
          const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
          const float4 iq = a.illum[q];
          if (!(iq.w > 0.0f)) continue;
          const float4 gq = a.guide[q];
          if (bg_p != (gq.w == 0.0f)) continue;
          if (a.ids && a.ids[q] != idp) continue;
          float g = 1.0f, arg = 0.0f;
          if (!bg_p) surface_pair(a, gp, gq, zden * sqrtf((float)(dx * dx + dy * dy)), g, arg);
          g = g * f_exp(-arg);
          const float lq = lum(iq.x, iq.y, iq.z);
          if (pass == 0) num += g * (lq - lp);
          else num += g * ((lq - m) * (lq - m));
          den += g;
        }
      }
      if (pass == 0) m = lp + num / den;
      else v = ((num / den) * 4.0f) / ip.w;
    }
  }
  ev[p] = make_float4(ip.x, ip.y, ip.z, v);
}

template <bool LAST>
__global__ __launch_bounds__(kTileW * kTileH) void k_svgf_iteration(SvgfFilterArgs a, uint32_t step, const float4* __restrict__ src,
                                                                    float4* __restrict__ dst, float4* __restrict__ feedback) {
  const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= a.width || y >= a.height) return;
  const uint32_t p = y * a.width + x;
  const float4 ep = src[p];
  if (ep.w < 0.0f) {
    dst[p] = make_float4(0.0f, 0.0f, 0.0f, LAST ? 0.0f : -1.0f);
    if (feedback) feedback[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  // the 3 x 3 Gaussian of the variance over the live neighbours at distance 1, whatever the step
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int64_t qy = (int64_t)y + dy;
    if (qy < 0 || qy >= (int64_t)a.height) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int64_t qx = (int64_t)x + dx;
      if (qx < 0 || qx >= (int64_t)a.width) continue;
      const float vq = (dx == 0 && dy == 0) ? ep.w : src[(uint32_t)qy * a.width + (uint32_t)qx].w;
      if (vq < 0.0f) continue;
      const float k = (float)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
      gs += k * vq, gw += k;
    }
  }
  const float Sp = a.sigma_lum * sqrtf(gs / gw) + kLumEps;
  const float4 gp = a.guide[p];
  const bool bg_p = gp.w == 0.0f;
  const uint32_t idp = a.ids ? a.ids[p] : 0u;
  const float lp = lum(ep.x, ep.y, ep.z);
  const float zden = a.sigma_depth * gp.w * (float)step;  // x |(dx, dy)| per tap
  const float kH[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int64_t qy = (int64_t)y + (int64_t)dy * step;
    if (qy < 0 || qy >= (int64_t)a.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int64_t qx = (int64_t)x + (int64_t)dx * step;
      if (qx < 0 || qx >= (int64_t)a.width) continue;
      const float h = kH[dx + 2] * kH[dy + 2];
      if (dx == 0 && dy == 0) {  // w(p, p) = 1
        sw += h, sv += (h * h) * ep.w;
        continue;
      }
      const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
      const float4 eq = src[q];
      if (eq.w < 0.0f) continue;
      const float4 gq = a.guide[q];
      if (bg_p != (gq.w == 0.0f)) continue;  // exactly one of the two is background
      if (a.ids && a.ids[q] != idp) continue;
      float w = 1.0f, arg = 0.0f;
      if (!bg_p) surface_pair(a, gp, gq, zden * sqrtf((float)(dx * dx + dy * dy)), w, arg);
      if (a.sigma_lum > 0.0f) {
        const float dl = fabsf(lp - lum(eq.x, eq.y, eq.z));
        if (dl != 0.0f) arg += dl / Sp;
      }
      w = w * f_exp(-arg) * h;  // w_z w_l = exp(-(depth term + luminance term))
      sx += w * (eq.x - ep.x), sy += w * (eq.y - ep.y), sz += w * (eq.z - ep.z), sw += w, sv += (w * w) * eq.w;
    }
  }
  // denoise.hip's form of the weighted mean: a constant neighbourhood comes back as it is, to the bit
  const float ox = ep.x + sx / sw, oy = ep.y + sy / sw, oz = ep.z + sz / sw;
  if (feedback) feedback[p] = make_float4(ox, oy, oz, a.illum[p].w);
  if (LAST) {
    const V3 al = clamped_albedo(a.albedo_hits, a.feature_count, p);  // what the accumulation divided by
    dst[p] = make_float4(ox * al.x, oy * al.y, oz * al.z, 1.0f);
  } else {
    dst[p] = make_float4(ox, oy, oz, sv / (sw * sw));
  }
}

static inline dim3 svgf_grid(const SvgfFilterArgs& a) { return dim3((a.width + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH); }

void launch_svgf_prepare(hipStream_t s, const SvgfFilterArgs& a, float4* ev) {
  hipLaunchKernelGGL(k_svgf_prepare, svgf_grid(a), dim3(kTileW, kTileH), 0, s, a, ev);
}
void launch_svgf_iteration(hipStream_t s, const SvgfFilterArgs& a, uint32_t i, bool last, const float4* src, float4* dst, float4* feedback) {
  if (last) hipLaunchKernelGGL(k_svgf_iteration<true>, svgf_grid(a), dim3(kTileW, kTileH), 0, s, a, 1u << i, src, dst, feedback);
  else hipLaunchKernelGGL(k_svgf_iteration<false>, svgf_grid(a), dim3(kTileW, kTileH), 0, s, a, 1u << i, src, dst, feedback);
}

}  // namespace pb
