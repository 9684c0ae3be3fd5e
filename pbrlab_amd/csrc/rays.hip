// rays.hip -- rendering along caller-supplied rays (pbrhip_render_rays).
//
// A path does not care where its first ray came from: k_generate_rays stores the first ray of every path of a group from a buffer,
// exactly where k_generate_camera (kernels.hip) stores a user camera's, and the group's first bounce runs through the ordinary kernels
// (PathState::first = 0).  k_project_rays writes such a buffer for three projections the pinhole cannot express (lat-long panorama,
// equidistant fisheye, orthographic), k_features_rays is the feature kernel (features.hip) over the same rays.
// Streaming kernels: two 16-byte words per ray, grid-stride, no LDS but the feature kernel's stack, no scratch.
// A translation unit of its own: the render kernels' code objects do not depend on it.
#include "denv.h"
#include "dfirsthit.h"
#include "rays_kernels.h"
#include "variants.h"

namespace pb {

constexpr int kBlock = 256;

// word index of the ray of (pixel gpix, pass)
__device__ __forceinline__ size_t ray_word(const RaySource& r, uint32_t width, uint32_t gpix, uint32_t pass) {
  const size_t plane = r.ray_passes == 1u ? 0u : (size_t)(pass - r.base_pass);
  return 2u * (plane * ((size_t)width * r.height) + gpix);
}

// ------------------------------------------------------------------ k_generate_rays
// Path order, stores and generator seed are k_generate_camera's.  The generator is advanced by camera_draws draws, what a camera that
// built the ray from the sample's own generator consumed (2: jitter; 4: jitter + lens), so that the path's draws continue behind them.
// An inactive ray: throughput 0 alone is not enough -- the head of a path's shading has no black test before its Russian roulette, and a
// hit with a first draw of exactly 0 would divide by 0 --, so the ray is replaced by one that misses for certain: tmin = FLT_MAX > tmax
// = 0 fails every primitive test (t > tmin && t <= tmax, dtrace.h) and every slab test of a finite box (exit >= tmin); its miss adds
// 0 x the environment.
__global__ __launch_bounds__(kBlock) void k_generate_rays(PathState P, RaySource r, uint32_t npaths) {
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < npaths; j += gridDim.x * kBlock) {
    const uint32_t R = P.pass_run, q = j / R;  // (camera_sample's path order, kernels.hip)
    const uint32_t pass = P.first_pass + (q / P.npix) * R + j % R;
    const uint32_t gpix = P.pix_index[q % P.npix];
    const size_t w = ray_word(r, P.width, gpix, pass);
    float4 o = r.rays[w], d = r.rays[w + 1];
    Rng rng = rng_seed(((uint64_t)pass << 32) + (uint64_t)gpix, P.seed_seq);
    for (uint32_t i = 0; i < r.camera_draws; i++) rng.state = rng.state * 6364136223846793005ULL + rng.inc;  // (pcg32's step)
    float thr = 1.0f;
    if (!ray_active(o, d)) o = make_float4(0.0f, 0.0f, 0.0f, kFltMax), d = make_float4(0.0f, 0.0f, 1.0f, 0.0f), thr = 0.0f;
    const uint32_t p = P.slot0 + j;
    P.L[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    P.ray_o[p] = o;
    P.ray_d[p] = d;
    P.thr[p] = make_float4(thr, thr, thr, __builtin_huge_valf());
    P.rng4[p] = make_uint4((uint32_t)rng.state, (uint32_t)(rng.state >> 32), 0u, 0u);
    P.q_in[j] = p;
  }
}

// ------------------------------------------------------------------ k_project_rays
// The ray of every (pixel, pass) of a pass range, lane = one sample; jx, jy are the first two draws of the sample's generator as in every
// camera here (render with camera_draws = 2), sx = 2 (x + jx) / W - 1, sy = 1 - 2 (y + jy) / H, aspect = W / H.
//   lat-long  phi = 2 pi (x + jx) / W - pi, theta = pi (y + jy) / H, d = sin theta sin phi r + cos theta u + sin theta cos phi f: the
//             inverse of env_texel_index's mapping (denv.h) with the image centre along f
//   fisheye   equidistant: rho = sqrt((sx aspect)^2 + sy^2), angle = rho x half the field of view,
//             d = sin(angle) (sx aspect r + sy u) / rho + cos(angle) f; rho > 1: an inactive ray (direction 0); rho = 0: f
//   ortho     origin eye + sx aspect half r + sy half u, direction f
// Directions go through normalize_raw; sines and cosines are denv.h's (the same bits on host and device).
__global__ __launch_bounds__(kBlock) void k_project_rays(ProjectArgs a) {
  const size_t npx = (size_t)a.width * a.height, n = npx * a.npass;
  const V3 f(a.cam.f[0], a.cam.f[1], a.cam.f[2]), r(a.cam.r[0], a.cam.r[1], a.cam.r[2]), u(a.cam.u[0], a.cam.u[1], a.cam.u[2]);
  const V3 eye(a.cam.eye[0], a.cam.eye[1], a.cam.eye[2]);
  const float aspect = (float)a.width / (float)a.height;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const uint32_t gpix = (uint32_t)(i % npx), pass = a.first_pass + (uint32_t)(i / npx);
    const uint32_t x = gpix % a.width, y = gpix / a.width;
    Rng rng = rng_seed(((uint64_t)pass << 32) + (uint64_t)gpix, a.seed_seq);
    const float jx = draw(rng);
    const float jy = draw(rng);
    const float fx = (float)x + jx, fy = (float)y + jy;
    V3 o = eye, d = f;
    bool active = true;
    if (a.projection == kProjLatLong) {
      const float phi = 2.0f * kPi * (fx / (float)a.width) - kPi, theta = kPi * (fy / (float)a.height);
      const float st = env_sin(theta), ct = env_cos(theta);
      d = normalize_raw((st * env_sin(phi)) * r + ct * u + (st * env_cos(phi)) * f);
    } else {
      const float sx = (2.0f * fx / (float)a.width - 1.0f) * aspect;
      const float sy = 1.0f - 2.0f * fy / (float)a.height;
      if (a.projection == kProjFisheye) {
        const float rho = sqrtf(sx * sx + sy * sy);
        active = rho <= 1.0f;
        if (rho > 0.0f) {
          const float ang = rho * a.param, k = env_sin(ang) / rho;
          d = normalize_raw((k * sx) * r + (k * sy) * u + env_cos(ang) * f);
        }
      } else {
        o = eye + (sx * a.param) * r + (sy * a.param) * u;
        d = normalize_raw(f);
      }
    }
    a.rays[2 * i] = make_float4(o.x, o.y, o.z, 0.0f);
    a.rays[2 * i + 1] = active ? make_float4(d.x, d.y, d.z, kInf) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// ------------------------------------------------------------------ k_features_rays
// k_features' walker (dfirsthit.h::first_hit_walk) with the ray of (pixel, pass) loaded: the same one-ray-per-lane traversal and LDS
// stack, the same pass-ordered sums; the traversal starts from the caller's tmin and tmax, an inactive ray counts as a sample and a miss.
struct ListRays {
  const FeatureRayArgs& a;
  struct Pixel {
    const FeatureRayArgs& a;
    uint32_t gpix;
    __device__ __forceinline__ bool operator()(uint32_t pass, V3& o, V3& d, float& tmin, float& tmax) const {
      const size_t w = ray_word(a.src, a.width, gpix, pass);
      const float4 ro = a.src.rays[w], rd = a.src.rays[w + 1];
      o = V3(ro.x, ro.y, ro.z), d = V3(rd.x, rd.y, rd.z), tmin = ro.w, tmax = rd.w;
      return ray_active(ro, rd);
    }
  };
  __device__ __forceinline__ Pixel operator()(uint32_t gpix) const { return {a, gpix}; }
};
template <bool CURVES, bool WIDE>
__global__ __launch_bounds__(kBlock, kFeatureBlocksPerCU) void k_features_rays(DScene sc, FeatureRayArgs a) {
  __shared__ uint32_t stk[kSimpleLdsStack * kBlock];
  first_hit_walk<CURVES, WIDE, false>(sc, a, nullptr, stk, ListRays{a});
}

// ------------------------------------------------------------------ launches
static uint32_t grid_for(size_t n, uint32_t cap) {
  const size_t g = (n + kBlock - 1) / kBlock;
  return (uint32_t)(g < cap ? (g ? g : 1) : cap);
}

void launch_generate_rays(hipStream_t s, const PathState& P, const RaySource& r, uint32_t npaths) {
  hipLaunchKernelGGL(k_generate_rays, dim3(grid_for(npaths, 8192)), dim3(kBlock), 0, s, P, r, npaths);
}

void launch_project_rays(hipStream_t s, const ProjectArgs& a) {
  const size_t n = (size_t)a.width * a.height * a.npass;
  if (!n) return;
  hipLaunchKernelGGL(k_project_rays, dim3(grid_for(n, 8192)), dim3(kBlock), 0, s, a);
}

// the <CURVES, WIDE> of launch_features (features.hip)
void launch_features_rays(hipStream_t s, const DScene& sc, const FeatureRayArgs& a, const Knobs& k) {
  if (!a.npix || !a.npass) return;
  const uint32_t g = grid_for(a.npix, kFeatureGridCap);
  with_hook_tree([&](auto c, auto w) { hipLaunchKernelGGL((k_features_rays<c, w>), dim3(g), dim3(kBlock), 0, s, sc, a); }, sc, k);
}

}  // namespace pb
