// denoise.hip -- the edge-avoiding A-trous filter of pbrhip_denoise (Dammertz et al. 2010) on albedo-demodulated colour.
//
//   k_denoise_prepare    the five input images -> two float4 images: e(0).rgb | kind and N.xyz | z, so that a tap is two 16-byte loads
//   k_denoise_iteration  e(i) -> e(i+1) with step 2^i over the 25 taps; the last one multiplies the albedo back and writes the output
//
// One launch per iteration, nothing returns to the host in between.  A thread is a pixel, a block a 64 x 4 tile: the taps of a wave are
// five rows of 64 consecutive pixels, 16 bytes each -- coalesced global loads served by the L2 (a 1080p image is 33 MB).
// All arithmetic is float32 without contraction; exp is the library's (f_exp).
#include "dmath.h"
#include "feature_kernels.h"

namespace pb {

constexpr int kTileW = 64, kTileH = 4;
constexpr float kKindHole = 0.0f, kKindSurface = 1.0f, kKindBackground = 2.0f;  // e.w: count == 0 | has a first hit | has none

// a_p: (sum of albedo + one white per miss) / samples; 1 without features, without samples or with PBRHIP_DENOISE_NO_ALBEDO
__device__ __forceinline__ V3 denoise_albedo(const DenoiseArgs& a, uint32_t p) {
  if (a.no_albedo || !a.albedo_hits) return V3(1.0f);
  const uint32_t m = a.feature_count[p];
  if (m == 0u) return V3(1.0f);
  const float4 ah = a.albedo_hits[p];
  const float fm = (float)m, miss = fm - ah.w;
  return V3((ah.x + miss) / fm, (ah.y + miss) / fm, (ah.z + miss) / fm);
}

__global__ __launch_bounds__(kTileW * kTileH) void k_denoise_prepare(DenoiseArgs a, float4* __restrict__ e0, float4* __restrict__ guide) {
  const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= a.width || y >= a.height) return;
  const uint32_t p = y * a.width + x;
  const uint32_t n = a.count[p];
  float4 e = make_float4(0.0f, 0.0f, 0.0f, kKindHole), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (n != 0u) {
    const float4 c = a.rgba[p];
    const float fn = (float)n;
    const V3 al = denoise_albedo(a, p);
    e.x = (c.x / fn) / smax(al.x, 1e-3f), e.y = (c.y / fn) / smax(al.y, 1e-3f), e.z = (c.z / fn) / smax(al.z, 1e-3f);
    e.w = kKindBackground;
    if (a.normal_depth) {
      const float4 nd = a.normal_depth[p];
      const float k = a.albedo_hits ? a.albedo_hits[p].w : 0.0f;
      const float len = sqrtf(nd.x * nd.x + nd.y * nd.y + nd.z * nd.z);
      if (k > 0.0f && len > 0.0f) g = make_float4(nd.x / len, nd.y / len, nd.z / len, nd.w / k), e.w = kKindSurface;
    }
  }
  e0[p] = e, guide[p] = g;
}

template <bool LAST>
__global__ __launch_bounds__(kTileW * kTileH) void k_denoise_iteration(DenoiseArgs a, uint32_t step, float inv_sc2, const float4* __restrict__ src,
                                                                       const float4* __restrict__ guide, float4* __restrict__ dst) {
  const uint32_t x = blockIdx.x * kTileW + threadIdx.x, y = blockIdx.y * kTileH + threadIdx.y;
  if (x >= a.width || y >= a.height) return;
  const uint32_t p = y * a.width + x;
  const float4 ep = src[p];
  if (ep.w == kKindHole) {
    dst[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 gp = guide[p];
  const bool bg_p = ep.w == kKindBackground;
  const float zden = a.sigma_depth * gp.w * (float)step;  // x |(dx, dy)| per tap
  const float kH[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
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
        sw += h;
        continue;
      }
      const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
      const float4 eq = src[q];
      if (eq.w == kKindHole) continue;
      const bool bg_q = eq.w == kKindBackground;
      if (bg_p != bg_q) continue;  // exactly one of the two is background: w_n = 0
      float w = 1.0f, arg = 0.0f;
      if (!bg_p) {
        const float4 gq = guide[q];
        w = smax(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
        for (uint32_t k = 0; k < a.normal_squarings; k++) w = w * w;
        const float dz = fabsf(gp.w - gq.w);
        if (a.sigma_depth > 0.0f && dz != 0.0f) arg = dz / (zden * sqrtf((float)(dx * dx + dy * dy)));
      }
      const float cx = eq.x - ep.x, cy = eq.y - ep.y, cz = eq.z - ep.z;
      if (a.sigma_color > 0.0f) {
        const float d2 = cx * cx + cy * cy + cz * cz;
        if (d2 != 0.0f) arg += d2 * inv_sc2;
      }
      w = w * f_exp(-arg) * h;  // w_z w_c = exp(-(depth term + colour term))
      sx += w * cx, sy += w * cy, sz += w * cz, sw += w;
    }
  }
  // the weighted mean as e_p + sum w (e_q - e_p) / sum w: a constant neighbourhood comes back as it is, to the bit
  float4 out = make_float4(ep.x + sx / sw, ep.y + sy / sw, ep.z + sz / sw, ep.w);
  if (LAST) {
    const V3 al = denoise_albedo(a, p);  // the unclamped albedo: a black one stays black
    out = make_float4(out.x * al.x, out.y * al.y, out.z * al.z, 1.0f);
  }
  dst[p] = out;
}

static inline dim3 denoise_grid(const DenoiseArgs& a) { return dim3((a.width + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH); }

void launch_denoise_prepare(hipStream_t s, const DenoiseArgs& a, float4* e0, float4* guide) {
  hipLaunchKernelGGL(k_denoise_prepare, denoise_grid(a), dim3(kTileW, kTileH), 0, s, a, e0, guide);
}
void launch_denoise_iteration(hipStream_t s, const DenoiseArgs& a, uint32_t i, bool last, const float4* src, const float4* guide, float4* dst) {
  // 1 / (sigma_color 2^-i)^2, in float as the model states it
  const float sc = a.sigma_color * (1.0f / (float)(1u << i));
  const float inv_sc2 = a.sigma_color > 0.0f ? 1.0f / (sc * sc) : 0.0f;
  if (last) hipLaunchKernelGGL(k_denoise_iteration<true>, denoise_grid(a), dim3(kTileW, kTileH), 0, s, a, 1u << i, inv_sc2, src, guide, dst);
  else hipLaunchKernelGGL(k_denoise_iteration<false>, denoise_grid(a), dim3(kTileW, kTileH), 0, s, a, 1u << i, inv_sc2, src, guide, dst);
}

}  // namespace pb
