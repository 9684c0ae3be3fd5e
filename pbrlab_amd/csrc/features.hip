// features.hip -- first-hit feature buffers (pbrhip_render_features): per pixel the sums, over a range of passes, of
// what the camera ray of each sample saw first -- albedo, viewer-facing shading normal, distance -- and the number of samples.
//
// Shape: lane = pixel.  A lane walks its pixel's passes in ascending order: the renderer's own camera ray of (pixel, pass)
// (dcamera.h) -> the one-ray-per-lane traversal (dtrace.h::traverse, the first kSimpleLdsStack stack entries in LDS, the rest in
// the spill area) -> make_surface (dshade.h) -> albedo, and adds the sample to the pixel's sums, which it holds in registers
// between one load and one store.  The float sums therefore run in pass order whatever the chunking; no per-sample state exists in
// HBM; the pixels of a wave are an 8 x 8 patch (ensure_pixels' order) looking at one pass at a time.
// A translation unit of its own: the render kernels' code objects do not depend on it.
#include <type_traits>

#include "dcamera.h"
#include "dshade.h"
#include "feature_kernels.h"

namespace pb {

constexpr int kBlock = 256;

template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_features(DScene sc, FeatureArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  TravStats st = {};
  uint32_t overflow = 0u;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.npix; j += gridDim.x * kBlock) {
    const uint32_t gpix = a.pix[j];
    const uint32_t x = gpix % a.width, y = gpix / a.width;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), N = A;
    uint32_t cnt = 0u;
    if (a.albedo_hits) A = a.albedo_hits[gpix];
    if (a.normal_depth) N = a.normal_depth[gpix];
    if (a.count) cnt = a.count[gpix];
    for (uint32_t pass = a.first_pass; pass != a.first_pass + a.npass; pass++) {
      Rng rng = rng_seed(((uint64_t)pass << 32) + (uint64_t)gpix, a.seed_seq);
      V3 o, d;
      if (a.user) user_camera_ray(a.ucam, x, y, a.width, a.height, rng, o, d);
      else reference_camera_ray(a.cam, x, y, rng, o, d);
      Hit h;
      traverse<false, false, CURVES, WIDE>(sc, o, d, 0.0f, kInf, h, stk + threadIdx.x, kBlock, st, &overflow,
                                           a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
      cnt++;
      if (h.slot == kNone) continue;
      const Surface s = make_surface(sc, o, d, h);
      V3 n = s.n_s;
      if (!(s.flags & kSlotIsCurve) && dot(d, n) > 0.0f) n = -n;  // towards the viewer; a curve's tangent stays as it is
      N.x += n.x, N.y += n.y, N.z += n.z, N.w += h.t;
      if (a.albedo_hits) {
        V3 c(0.0f);
        if (s.material != kNone) {
          const float4 m = a.mat_albedo[s.material];
          const uint32_t tex = __float_as_uint(m.w);
          c = tex != kNone ? texture_fetch3(sc, tex, s.tu, s.tv) : V3(m.x, m.y, m.z);
        }
        A.x += c.x, A.y += c.y, A.z += c.z, A.w += 1.0f;
      }
    }
    if (a.albedo_hits) a.albedo_hits[gpix] = A;
    if (a.normal_depth) a.normal_depth[gpix] = N;
    if (a.count) a.count[gpix] = cnt;
  }
  if (overflow) *a.overflow = 1u;
}

// the <CURVES, WIDE> of the tree the render of this scene walks; the binary tree's instance always carries the curve code (the hooks' rule)
void launch_features(hipStream_t s, const DScene& sc, const FeatureArgs& a, const Knobs& k) {
  if (!a.npix || !a.npass) return;
  uint32_t g = (a.npix + kBlock - 1) / kBlock;
  g = g < kFeatureGridCap ? g : kFeatureGridCap;
  const bool wide = sc.wide != nullptr && k.wide;
  if (!wide) hipLaunchKernelGGL((k_features<true, false>), dim3(g), dim3(kBlock), 0, s, sc, a);
  else if (sc.num_curves != 0) hipLaunchKernelGGL((k_features<true, true>), dim3(g), dim3(kBlock), 0, s, sc, a);
  else hipLaunchKernelGGL((k_features<false, true>), dim3(g), dim3(kBlock), 0, s, sc, a);
}

}  // namespace pb
