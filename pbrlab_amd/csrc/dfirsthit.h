// dfirsthit.h -- the pixel loop of the first-hit feature kernels (k_features, k_features_emission, k_features_rays; DESIGN.md §12, §14,
// §18), written once.
//
// Shape: lane = pixel.  A lane walks its pixel's passes in ascending order: the sample's ray from the kernel's ray source -> the
// one-ray-per-lane traversal (dtrace.h::traverse, the first kSimpleLdsStack stack entries in LDS, the rest in the spill area) ->
// make_surface (dshade.h) -> albedo, and adds the sample to the pixel's sums, which it holds in registers between one load and one store.
// The float sums therefore run in pass order whatever the chunking; no per-sample state exists in HBM; the pixels of a wave are an 8 x 8
// patch (ensure_pixels' order) looking at one pass at a time.
//
// A ray source is a functor: source(gpix) gives the pixel's own functor, and that one, called with (pass, o, d, tmin, tmax), gives the
// sample's ray or returns false for a sample without one (it counts, and misses).
#pragma once

#include "dcamera.h"
#include "dshade.h"
#include "feature_kernels.h"

namespace pb {

// the renderer's own camera ray of (pixel, pass) (dcamera.h), from 0 to infinity
struct CameraRays {
  const FeatureArgs& a;
  struct Pixel {
    const FeatureArgs& a;
    uint32_t gpix, x, y;
    __device__ __forceinline__ bool operator()(uint32_t pass, V3& o, V3& d, float& tmin, float& tmax) const {
      Rng rng = rng_seed(((uint64_t)pass << 32) + (uint64_t)gpix, a.seed_seq);
      if (a.user) user_camera_ray(a.ucam, x, y, a.width, a.height, rng, o, d);
      else reference_camera_ray(a.cam, x, y, rng, o, d);
      tmin = 0.0f, tmax = kInf;
      return true;
    }
  };
  __device__ __forceinline__ Pixel operator()(uint32_t gpix) const { return {a, gpix, gpix % a.width, gpix / a.width}; }
};

// `a`: FeatureArgs or FeatureRayArgs (the members the loop reads have the same names in both).  stk: the block's LDS stack,
// kSimpleLdsStack words per thread of the block: its size says how many threads the kernel is launched with.  emission (EMISSION only,
// may be null): one more sum, what the renderer adds to L at depth 0 (kernels.hip::path_head with first == true: weight 1, throughput 1;
// env_miss_path for a camera ray), and the number of samples that added it.
template <bool CURVES, bool WIDE, bool EMISSION, class Args, class Source, uint32_t WORDS>
__device__ __forceinline__ void first_hit_walk(const DScene& sc, const Args& a, float4* emission, uint32_t (&stk)[WORDS], const Source& source) {
  constexpr uint32_t kBlock = WORDS / kSimpleLdsStack;
  TravStats st = {};
  uint32_t overflow = 0u;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.npix; j += gridDim.x * kBlock) {
    const uint32_t gpix = a.pix[j];
    const auto ray = source(gpix);
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), N = A, E = A;
    uint32_t cnt = 0u;
    if (a.albedo_hits) A = a.albedo_hits[gpix];
    if (a.normal_depth) N = a.normal_depth[gpix];
    if (a.count) cnt = a.count[gpix];
    if constexpr (EMISSION)
      if (emission) E = emission[gpix];
    for (uint32_t pass = a.first_pass; pass != a.first_pass + a.npass; pass++) {
      V3 o, d;
      float tmin, tmax;
      cnt++;
      if (!ray(pass, o, d, tmin, tmax)) continue;
      Hit h;
      traverse<false, false, CURVES, WIDE>(sc, o, d, tmin, tmax, h, stk + threadIdx.x, kBlock, st, &overflow,
                                           a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
      if (h.slot == kNone) {
        if constexpr (EMISSION)
          if (emission && sc.env_texels) {  // env_miss_path, first == true: L += 1 * texel * 1
            const float4 L = sc.env_texels[env_texel_index(env_from_world(sc.env_m, d), sc.env_w, sc.env_h)];
            E.x += L.x, E.y += L.y, E.z += L.z, E.w += 1.0f;
          }
        continue;
      }
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
      if constexpr (EMISSION)
        if (emission && s.face == kFront && s.lightrec != kNone) {  // path_head, first == true: L += 1 * lr[4].xyz * 1
          const float4 le = reinterpret_cast<const float4*>(sc.lrecs + s.lightrec)[4];
          E.x += le.x, E.y += le.y, E.z += le.z, E.w += 1.0f;
        }
    }
    if (a.albedo_hits) a.albedo_hits[gpix] = A;
    if (a.normal_depth) a.normal_depth[gpix] = N;
    if (a.count) a.count[gpix] = cnt;
    if constexpr (EMISSION)
      if (emission) emission[gpix] = E;
  }
  if (overflow) *a.overflow = 1u;
}

}  // namespace pb
