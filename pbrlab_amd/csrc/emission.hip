// emission.hip -- the first-hit emission layer (pbrhip_render_features_emission, pbrhip_emission_split, pbrhip_emission_merge;
// DESIGN.md §18): the light the camera sees directly, kept apart from the light surfaces reflect, so that only the latter is divided
// by the albedo.
//
//   k_features_emission  features.hip::k_features statement for statement -- lane = pixel, the passes in ascending order, the renderer's
//                        own camera ray (dcamera.h), the one-ray-per-lane traversal with kSimpleLdsStack entries in LDS and the rest in
//                        the spill area, make_surface, the sums in registers between one load and one store, a grid-stride loop under
//                        the grid cap -- and one more sum: what the renderer adds to L at depth 0 (kernels.hip::path_head with
//                        first == true: weight 1, throughput 1; env_miss_path for a camera ray), and the number of samples that added it
//   k_emission_split     per pixel: the sums minus the emission sums, clamped at 0; the albedo sums with hits := samples (a miss is black)
//   k_emission_merge     per pixel: filtered + emission / samples
//
// A translation unit of its own: no other code object depends on it.  All arithmetic is float32 without contraction.
#include "dcamera.h"
#include "dshade.h"
#include "emission_kernels.h"

namespace pb {

constexpr int kBlock = 256;

template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_features_emission(DScene sc, FeatureArgs a, float4* emission) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  TravStats st = {};
  uint32_t overflow = 0u;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.npix; j += gridDim.x * kBlock) {
    const uint32_t gpix = a.pix[j];
    const uint32_t x = gpix % a.width, y = gpix / a.width;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), N = A, E = A;
    uint32_t cnt = 0u;
    if (a.albedo_hits) A = a.albedo_hits[gpix];
    if (a.normal_depth) N = a.normal_depth[gpix];
    if (a.count) cnt = a.count[gpix];
    if (emission) E = emission[gpix];
    for (uint32_t pass = a.first_pass; pass != a.first_pass + a.npass; pass++) {
      Rng rng = rng_seed(((uint64_t)pass << 32) + (uint64_t)gpix, a.seed_seq);
      V3 o, d;
      if (a.user) user_camera_ray(a.ucam, x, y, a.width, a.height, rng, o, d);
      else reference_camera_ray(a.cam, x, y, rng, o, d);
      Hit h;
      traverse<false, false, CURVES, WIDE>(sc, o, d, 0.0f, kInf, h, stk + threadIdx.x, kBlock, st, &overflow,
                                           a.spill + blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
      cnt++;
      if (h.slot == kNone) {
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
      if (emission && s.face == kFront && s.lightrec != kNone) {  // path_head, first == true: L += 1 * lr[4].xyz * 1
        const float4 le = reinterpret_cast<const float4*>(sc.lrecs + s.lightrec)[4];
        E.x += le.x, E.y += le.y, E.z += le.z, E.w += 1.0f;
      }
    }
    if (a.albedo_hits) a.albedo_hits[gpix] = A;
    if (a.normal_depth) a.normal_depth[gpix] = N;
    if (a.count) a.count[gpix] = cnt;
    if (emission) emission[gpix] = E;
  }
  if (overflow) *a.overflow = 1u;
}

// launch_features' grid and its rule for <CURVES, WIDE> (features.hip)
void launch_features_emission(hipStream_t s, const DScene& sc, const FeatureArgs& a, float4* emission, const Knobs& k) {
  if (!a.npix || !a.npass) return;
  uint32_t g = (a.npix + kBlock - 1) / kBlock;
  g = g < kFeatureGridCap ? g : kFeatureGridCap;
  const bool wide = sc.wide != nullptr && k.wide;
  if (!wide) hipLaunchKernelGGL((k_features_emission<true, false>), dim3(g), dim3(kBlock), 0, s, sc, a, emission);
  else if (sc.num_curves != 0) hipLaunchKernelGGL((k_features_emission<true, true>), dim3(g), dim3(kBlock), 0, s, sc, a, emission);
  else hipLaunchKernelGGL((k_features_emission<false, true>), dim3(g), dim3(kBlock), 0, s, sc, a, emission);
}

// ------------------------------------------------------------------ split and merge
// The definitions are include/pbrhip.h's.  A thread reads its pixel before it writes it: out_rgba may be rgba, out_albedo_hits may be
// albedo_hits, out may be filtered (hence no __restrict__ on those).
__device__ __forceinline__ float pos_part(float d) { return d > 0.0f ? d : 0.0f; }  // (a NaN difference gives 0)

__global__ __launch_bounds__(kBlock) void k_emission_split(EmissionSplitArgs a) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < a.npx; p += (size_t)gridDim.x * kBlock) {
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.count[p] != 0u) {
      const float4 c = a.rgba[p], e = a.emission[p];
      out = make_float4(pos_part(c.x - e.x), pos_part(c.y - e.y), pos_part(c.z - e.z), c.w);
    }
    a.out_rgba[p] = out;
    if (a.out_albedo_hits) {
      const float4 ah = a.albedo_hits[p];
      a.out_albedo_hits[p] = make_float4(ah.x, ah.y, ah.z, (float)a.feature_count[p]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_emission_merge(EmissionMergeArgs a) {
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < a.npx; p += (size_t)gridDim.x * kBlock) {
    float4 out = a.filtered[p];
    const uint32_t cnt = a.count[p];
    if (cnt != 0u) {
      const float4 e = a.emission[p];
      const float fc = (float)cnt;
      out.x = out.x + e.x / fc, out.y = out.y + e.y / fc, out.z = out.z + e.z / fc;
    }
    a.out[p] = out;
  }
}

static inline uint32_t pixel_grid(size_t npx) {
  const size_t g = (npx + kBlock - 1) / kBlock;
  return (uint32_t)(g < 8192 ? g : 8192);
}
void launch_emission_split(hipStream_t s, const EmissionSplitArgs& a) {
  if (!a.npx) return;
  hipLaunchKernelGGL(k_emission_split, dim3(pixel_grid(a.npx)), dim3(kBlock), 0, s, a);
}
void launch_emission_merge(hipStream_t s, const EmissionMergeArgs& a) {
  if (!a.npx) return;
  hipLaunchKernelGGL(k_emission_merge, dim3(pixel_grid(a.npx)), dim3(kBlock), 0, s, a);
}

}  // namespace pb
