// image.cpp -- the image-space entry points of the C ABI: first-hit feature buffers and the edge-avoiding filter, the
// feature pass over caller-supplied rays and the projections (§14), motion vectors and temporal accumulation (§16), object ids and
// variance-guided filtering (§17), the first-hit emission layer (§18).  Host C++ only; the kernels are features.hip's, denoise.hip's,
// rays.hip's, temporal.hip's, svgf.hip's and emission.hip's.
//
// Every family has a device variant (device pointers, the work) and a host variant: checks, stage, the device variant's body, finish.
#include <math.h>

#include <deque>

#include "emission_kernels.h"
#include "feature_kernels.h"
#include "scene_impl.h"
#include "svgf_kernels.h"
#include "temporal_kernels.h"

using namespace pb;

// ------------------------------------------------------------------ staging
// The device copies of a host entry point's arrays, for the length of the call.  Bound to a scene's stream (asynchronous copies, one
// synchronise in finish) or to nothing: the current device's null stream, synchronous copies.  A null host pointer gives a null device
// pointer.  The first failure sticks: every later request gives null, and ready() reports it before anything is launched.
class Staging {
 public:
  Staging() = default;
  explicit Staging(hipStream_t st) : st_(st), async_(true) {}
  template <typename T>
  const T* in(const T* host, size_t n) { return static_cast<const T*>(stage(const_cast<T*>(host), n * sizeof(T), true, false)); }
  // preload: the output starts from the host's values (PBRHIP_RENDER_NO_CLEAR)
  template <typename T>
  T* out(T* host, size_t n, bool preload = false) { return static_cast<T*>(stage(host, n * sizeof(T), preload, true)); }
  int ready() const { return rc_; }
  // the outputs go back to the host
  int finish() {
    for (const Out& o : outs_) HIPCHK(copy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    if (async_) HIPCHK(hipStreamSynchronize(st_));
    return PBRHIP_OK;
  }

 private:
  struct Out {
    void *host, *dev;
    size_t bytes;
  };
  hipError_t copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    return async_ ? hipMemcpyAsync(dst, src, bytes, kind, st_) : hipMemcpy(dst, src, bytes, kind);
  }
  void* stage(void* host, size_t bytes, bool upload, bool download) {
    if (!host || rc_) return nullptr;
    rc_ = [&]() -> int {
      bufs_.emplace_back();
      HIPCHK(bufs_.back().reserve(bytes));
      if (upload) HIPCHK(copy(bufs_.back().p, host, bytes, hipMemcpyHostToDevice));
      if (download) outs_.push_back({host, bufs_.back().p, bytes});
      return PBRHIP_OK;
    }();
    return rc_ ? nullptr : bufs_.back().p;
  }
  hipStream_t st_ = nullptr;
  bool async_ = false;
  int rc_ = PBRHIP_OK;
  std::deque<DevBuf<unsigned char>> bufs_;
  std::vector<Out> outs_;
};

// ------------------------------------------------------------------ what the entry points on a device index check
// the image's size, where the entry point's argument checks have it ...
static int check_image(const char* who, uint32_t width, uint32_t height) {
  if (width == 0 || height == 0) return fail(PBRHIP_EINVAL, "%s: empty image", who);
  if ((uint64_t)width * height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "%s: image too large", who);
  return PBRHIP_OK;
}
// ... and, after every argument check, a device to work on
static int check_device(const char* who, int device) {
  int n = 0;
  if (int rc = pbrhip_device_count(&n)) return rc;
  if (n <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
  if (device < 0 || device >= n) return fail(PBRHIP_EINVAL, "%s: device %d out of range (%d devices)", who, device, n);
  return PBRHIP_OK;
}

// ------------------------------------------------------------------ feature buffers and denoiser
// What a first hit on a material adds to the albedo sum: rgb | the base-colour map's id (kNone: the rgb stands).  Principled: base_color.
// Hair: base_color when it is coloured by RGB; for melanin the colour whose sigma_a under hair_param_to_bsdf's RGB mapping
// (sigma_a = (log c / poly(beta_n))^2) is the material's: c = exp(-sqrt(sigma_a) poly(beta_n)), in double, rounded once.
static float4 feature_albedo(const HostMaterial& hm) {
  if (hm.kind == kMatPrincipled) return make_float4(hm.pr.base_color[0], hm.pr.base_color[1], hm.pr.base_color[2], __builtin_bit_cast(float, hm.pr.base_color_tex_id));
  const float none = __builtin_bit_cast(float, kNone);
  if (hm.hr.coloring_hair == 0) return make_float4(hm.hr.base_color[0], hm.hr.base_color[1], hm.hr.base_color[2], none);
  const V3 sa = hair_param_to_bsdf(hm.hr).sigma_a;
  const double bn = hm.hr.azimuthal_roughness;
  const double poly = 5.969 - 0.215 * bn + 2.532 * bn * bn - 10.73 * bn * bn * bn + 5.574 * bn * bn * bn * bn + 0.245 * bn * bn * bn * bn * bn;
  return make_float4((float)exp(-sqrt((double)sa.x) * poly), (float)exp(-sqrt((double)sa.y) * poly), (float)exp(-sqrt((double)sa.z) * poly), none);
}

// the body of pbrhip_render_features_device: device pointers on the scene's device, each may be null
// rays: null, or the caller's rays in place of the scene's camera (k_features_rays)
// with_emission: the pass of pbrhip_render_features_emission (k_features_emission; not with rays); d_emission may be null
static int features_impl(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_albedo_hits, float* d_normal_depth, uint32_t* d_count,
                         const RaySource* rays = nullptr, bool with_emission = false, float* d_emission = nullptr) {
  if (int rc = check_render_desc(s, d)) return rc;
  if (d->num_sample == 0) return fail(PBRHIP_EINVAL, "render_features: no samples");
  if ((uint64_t)d->first_pass + d->num_sample > (1ull << 32)) return fail(PBRHIP_EINVAL, "render_features: the passes do not fit 32 bits");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t npx_img = (size_t)d->width * d->height;
  if (!(d->flags & PBRHIP_RENDER_NO_CLEAR)) {
    if (d_albedo_hits) HIPCHK(hipMemsetAsync(d_albedo_hits, 0, npx_img * 4 * sizeof(float), st));
    if (d_normal_depth) HIPCHK(hipMemsetAsync(d_normal_depth, 0, npx_img * 4 * sizeof(float), st));
    if (d_count) HIPCHK(hipMemsetAsync(d_count, 0, npx_img * sizeof(uint32_t), st));
    if (d_emission) HIPCHK(hipMemsetAsync(d_emission, 0, npx_img * 4 * sizeof(float), st));
  }
  if (int rc = ensure_pixels(s, k, d->width, d->height, d->tile_rank, d->tile_world ? d->tile_world : 1, d->shard_block)) return rc;
  const uint32_t npix = s->pk_npix;
  if (npix == 0 || (!d_albedo_hits && !d_normal_depth && !d_count && !d_emission)) {
    HIPCHK(hipStreamSynchronize(st));
    return PBRHIP_OK;
  }
  std::vector<float4> albedo(std::max<size_t>(s->materials.size(), 1), make_float4(0.f, 0.f, 0.f, 0.f));
  for (size_t i = 0; i < s->materials.size(); i++) albedo[i] = feature_albedo(s->materials[i]);  // (from the host model: material updates are seen)
  HIPCHK(s->feat_albedo.upload(albedo, st));
  if (int rc = prepare_traversal(s)) return rc;
  FeatureArgs a;
  a.user = s->cam_set ? 1u : 0u;
  a.ucam = s->cam_set ? make_user_camera(s, d->width, d->height) : UserCamera{};
  a.cam = s->cam_set ? Camera{} : make_camera(s, d->width, d->height);
  a.width = d->width, a.height = d->height, a.seed_seq = d->seed_seq;
  a.pix = s->path_pix.p, a.npix = npix;
  a.mat_albedo = s->feat_albedo.p;
  a.albedo_hits = reinterpret_cast<float4*>(d_albedo_hits), a.normal_depth = reinterpret_cast<float4*>(d_normal_depth), a.count = d_count;
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  // max_paths_in_flight bounds the samples of one launch as it bounds the paths of a render's chunk; a pixel's sums continue from
  // chunk to chunk in pass order, so the split is invisible in the result
  uint32_t chunk = d->num_sample;
  if (d->max_paths_in_flight) chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(d->num_sample, d->max_paths_in_flight / npix));
  FeatureRayArgs ra{};
  if (rays) {
    ra.src = *rays, ra.src.base_pass = d->first_pass, ra.src.height = d->height;
    ra.width = d->width, ra.pix = a.pix, ra.npix = npix, ra.mat_albedo = a.mat_albedo;
    ra.albedo_hits = a.albedo_hits, ra.normal_depth = a.normal_depth, ra.count = a.count, ra.overflow = a.overflow, ra.spill = a.spill;
  }
  for (uint32_t done = 0; done < d->num_sample; done += chunk) {
    a.first_pass = ra.first_pass = d->first_pass + done, a.npass = ra.npass = std::min(chunk, d->num_sample - done);
    if (rays) launch_features_rays(st, s->dscene, ra, k);
    else if (with_emission) launch_features_emission(st, s->dscene, a, reinterpret_cast<float4*>(d_emission), k);
    else launch_features(st, s->dscene, a, k);
    HIPCHK(hipGetLastError());
  }
  return finish_traversal(s);
}

// the host variant of the feature pass, with the emission layer or without
static int features_host(pbrhip_scene* s, const pbrhip_render_desc* d, float* albedo_hits, float* normal_depth, uint32_t* count, bool with_emission,
                         float* emission) {
  if (!s || !d) return fail(PBRHIP_EINVAL, "render_features: NULL argument");
  if (int rc = check_render_desc(s, d)) return rc;
  HIPCHK(hipSetDevice(s->device));
  const size_t npx = (size_t)d->width * d->height;
  const bool keep = (d->flags & PBRHIP_RENDER_NO_CLEAR) != 0;
  Staging g(s->stream);
  float* const d_a = g.out(albedo_hits, npx * 4, keep);
  float* const d_n = g.out(normal_depth, npx * 4, keep);
  float* const d_e = g.out(emission, npx * 4, keep);
  uint32_t* const d_c = g.out(count, npx, keep);
  if (int rc = g.ready()) return rc;
  if (int rc = features_impl(s, d, d_a, d_n, d_c, nullptr, with_emission, d_e)) return rc;
  return g.finish();
}

extern "C" int pbrhip_render_features_device(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_albedo_hits, float* d_normal_depth,
                                             uint32_t* d_count) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_features: NULL argument");
    return features_impl(s, d, d_albedo_hits, d_normal_depth, d_count);
  });
}

extern "C" int pbrhip_render_features(pbrhip_scene* s, const pbrhip_render_desc* d, float* albedo_hits, float* normal_depth, uint32_t* count) {
  return guarded([&]() -> int { return features_host(s, d, albedo_hits, normal_depth, count, false, nullptr); });
}

// ------------------------------------------------------------------ the feature pass along caller-supplied rays, the projections
extern "C" int pbrhip_render_features_rays_device(pbrhip_scene* s, const pbrhip_render_desc* d, const void* d_rays, uint32_t ray_passes,
                                                  void* stream, float* d_albedo_hits, float* d_normal_depth, uint32_t* d_count) {
  return guarded([&]() -> int {
    if (int rc = check_ray_args("render_features_rays", s, d, d_rays, ray_passes, 0)) return rc;
    if (int rc = check_render_desc(s, d)) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    RaySource src{};
    src.rays = static_cast<const float4*>(d_rays), src.ray_passes = ray_passes;
    return features_impl(s, d, d_albedo_hits, d_normal_depth, d_count, &src);
  });
}

extern "C" int pbrhip_projection_rays_device(pbrhip_scene* s, uint32_t projection, float param, uint32_t width, uint32_t height,
                                             uint32_t first_pass, uint32_t num_pass, uint64_t seed_seq, void* d_rays, void* stream) {
  return guarded([&]() -> int {
    if (!s || !d_rays) return fail(PBRHIP_EINVAL, "projection_rays: NULL scene or rays");
    if (projection > PBRHIP_PROJECTION_ORTHO) return fail(PBRHIP_EINVAL, "projection_rays: unknown projection %u", projection);
    if (width == 0 || height == 0) return fail(PBRHIP_EINVAL, "projection_rays: zero image size");
    if ((uint64_t)width * height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "projection_rays: image too large");
    if ((uint64_t)first_pass + num_pass > (1ull << 32)) return fail(PBRHIP_EINVAL, "projection_rays: the passes do not fit 32 bits");
    if (!isfinite(param) || param < 0.0f) return fail(PBRHIP_EINVAL, "projection_rays: param %g is not a finite number >= 0", (double)param);
    if (projection == PBRHIP_PROJECTION_FISHEYE && param > 360.0f) return fail(PBRHIP_EINVAL, "projection_rays: a fisheye of %g degrees (at most 360)", (double)param);
    if (projection == PBRHIP_PROJECTION_ORTHO && !(param > 0.0f)) return fail(PBRHIP_EINVAL, "projection_rays: an orthographic view needs its half height > 0");
    if (!s->cam_set) return fail(PBRHIP_ESTATE, "projection_rays: the scene has no camera (pbrhip_scene_set_camera gives the frame)");
    if (num_pass == 0) return PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    ProjectArgs a{};
    a.cam = make_user_camera(s, width, height);
    a.projection = projection;
    // fisheye: the field of view in degrees, 0 = the camera's vertical one; the kernel takes half of it in radians, rounded once
    if (projection == PBRHIP_PROJECTION_FISHEYE) a.param = (float)((double)(param > 0.0f ? param : s->cam_vfov) * M_PI / 360.0);
    else a.param = param;
    a.width = width, a.height = height, a.first_pass = first_pass, a.npass = num_pass, a.seed_seq = seed_seq;
    a.rays = static_cast<float4*>(d_rays);
    launch_project_rays(static_cast<hipStream_t>(stream), a);
    HIPCHK(hipGetLastError());
    return PBRHIP_OK;
  });
}

// ------------------------------------------------------------------ the edge-avoiding filter
// the filter's arguments, host or device: the checks and both entry points pass them as one
struct DenoisePtrs {
  const float* rgba;
  const uint32_t* count;
  const float *albedo_hits, *normal_depth;
  const uint32_t* feature_count;
  float* out_rgba;
};
struct DenoiseParams {
  uint32_t iterations;
  float sigma_color, sigma_depth;
  uint32_t normal_squarings, flags;
};

// the checks both denoise entry points share; resolves the iteration default
static int check_denoise(int device, uint32_t width, uint32_t height, const DenoisePtrs& p, DenoiseParams& q) {
  if (!p.rgba || !p.count || !p.out_rgba) return fail(PBRHIP_EINVAL, "denoise: NULL rgba, count or out_rgba");
  if (int rc = check_image("denoise", width, height)) return rc;
  const int nfeat = (p.albedo_hits ? 1 : 0) + (p.normal_depth ? 1 : 0) + (p.feature_count ? 1 : 0);
  if (nfeat != 0 && nfeat != 3) return fail(PBRHIP_EINVAL, "denoise: albedo_hits, normal_depth and feature_count come together or not at all");
  if (q.sigma_color != q.sigma_color || q.sigma_depth != q.sigma_depth) return fail(PBRHIP_EINVAL, "denoise: a sigma is NaN");
  if (q.iterations > 8) return fail(PBRHIP_EINVAL, "denoise: %u iterations (at most 8)", q.iterations);
  if (q.normal_squarings > 16) return fail(PBRHIP_EINVAL, "denoise: %u normal squarings (at most 16)", q.normal_squarings);
  if (q.flags & ~PBRHIP_DENOISE_NO_ALBEDO) return fail(PBRHIP_EINVAL, "denoise: unknown flags 0x%x", q.flags);
  if (q.iterations == 0) q.iterations = PBRHIP_DENOISE_ITERATIONS;
  return check_device("denoise", device);
}

// prepare + one launch per iteration on the device's null stream; the three temporaries (two colour images, one guide image) live
// for the call
static int denoise_impl(int device, uint32_t width, uint32_t height, const DenoisePtrs& p, const DenoiseParams& q) {
  HIPCHK(hipSetDevice(device));
  const size_t npx = (size_t)width * height;
  DevBuf<float4> e0, e1, guide;
  HIPCHK(e0.reserve(npx));
  HIPCHK(e1.reserve(npx));
  HIPCHK(guide.reserve(npx));
  DenoiseArgs a;
  a.width = width, a.height = height;
  a.rgba = reinterpret_cast<const float4*>(p.rgba), a.count = p.count;
  a.albedo_hits = reinterpret_cast<const float4*>(p.albedo_hits), a.normal_depth = reinterpret_cast<const float4*>(p.normal_depth), a.feature_count = p.feature_count;
  a.no_albedo = (q.flags & PBRHIP_DENOISE_NO_ALBEDO) ? 1u : 0u;
  a.sigma_color = q.sigma_color, a.sigma_depth = q.sigma_depth, a.normal_squarings = q.normal_squarings;
  launch_denoise_prepare(nullptr, a, e0.p, guide.p);
  HIPCHK(hipGetLastError());
  for (uint32_t i = 0; i < q.iterations; i++) {
    const bool last = i + 1 == q.iterations;
    float4* const src = (i & 1u) ? e1.p : e0.p;
    float4* const dst = last ? reinterpret_cast<float4*>(p.out_rgba) : ((i & 1u) ? e0.p : e1.p);
    launch_denoise_iteration(nullptr, a, i, last, src, guide.p, dst);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_denoise_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                     const float* d_albedo_hits, const float* d_normal_depth, const uint32_t* d_feature_count, uint32_t iterations,
                                     float sigma_color, float sigma_depth, uint32_t normal_squarings, uint32_t flags, float* d_out_rgba) {
  return guarded([&]() -> int {
    const DenoisePtrs p{d_rgba, d_count, d_albedo_hits, d_normal_depth, d_feature_count, d_out_rgba};
    DenoiseParams q{iterations, sigma_color, sigma_depth, normal_squarings, flags};
    if (int rc = check_denoise(device, width, height, p, q)) return rc;
    return denoise_impl(device, width, height, p, q);
  });
}

extern "C" int pbrhip_denoise(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                              const float* normal_depth, const uint32_t* feature_count, uint32_t iterations, float sigma_color, float sigma_depth,
                              uint32_t normal_squarings, uint32_t flags, float* out_rgba) {
  return guarded([&]() -> int {
    const DenoisePtrs h{rgba, count, albedo_hits, normal_depth, feature_count, out_rgba};
    DenoiseParams q{iterations, sigma_color, sigma_depth, normal_squarings, flags};
    if (int rc = check_denoise(device, width, height, h, q)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const DenoisePtrs p{g.in(rgba, npx * 4), g.in(count, npx), g.in(albedo_hits, npx * 4), g.in(normal_depth, npx * 4), g.in(feature_count, npx),
                        g.out(out_rgba, npx * 4)};
    if (int rc = g.ready()) return rc;
    if (int rc = denoise_impl(device, width, height, p, q)) return rc;
    return g.finish();
  });
}

// ------------------------------------------------------------------ motion vectors and temporal accumulation
extern "C" int pbrhip_scene_snapshot_pose(pbrhip_scene* s) {
  return guarded([&]() -> int {
    if (!s) return fail(PBRHIP_EINVAL, "scene_snapshot_pose: scene is NULL");
    if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
    PB_NOT_STALE(s);
    HIPCHK(hipSetDevice(s->device));
    const size_t words = (size_t)s->tree.num_slots * 4;
    s->pose_set = false;
    HIPCHK(s->pose_slots.reserve(words));
    // on the scene's stream: behind the render that still reads the slots, in front of the refit that rewrites them
    if (words) HIPCHK(hipMemcpyAsync(s->pose_slots.p, s->dscene.slots, words * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    s->pose_cam = pose_camera(s);
    s->pose_set = true;
    return PBRHIP_OK;
  });
}

// the body of pbrhip_render_motion_device: device pointers on the scene's device, each may be null
static int motion_impl(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_motion, float* d_guide, uint32_t* d_ident) {
  if (int rc = check_render_desc(s, d)) return rc;
  if (!s->pose_set) return fail(PBRHIP_ESTATE, "render_motion: the scene has no pose snapshot (pbrhip_scene_snapshot_pose)");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const size_t npx_img = (size_t)d->width * d->height;
  if (d_motion) HIPCHK(hipMemsetAsync(d_motion, 0, npx_img * 4 * sizeof(float), st));
  if (d_guide) HIPCHK(hipMemsetAsync(d_guide, 0, npx_img * 4 * sizeof(float), st));
  if (d_ident) HIPCHK(hipMemsetAsync(d_ident, 0, npx_img * 4 * sizeof(uint32_t), st));
  if (int rc = ensure_pixels(s, k, d->width, d->height, d->tile_rank, d->tile_world ? d->tile_world : 1, d->shard_block)) return rc;
  const uint32_t npix = s->pk_npix;
  if (npix == 0 || (!d_motion && !d_guide && !d_ident)) {
    HIPCHK(hipStreamSynchronize(st));
    return PBRHIP_OK;
  }
  if (int rc = prepare_traversal(s)) return rc;
  MotionArgs a{};
  a.user = s->cam_set ? 1u : 0u, a.user_prev = s->pose_cam.set ? 1u : 0u;
  if (a.user) a.ucam = make_user_camera(s, d->width, d->height);
  else a.cam = make_camera(s, d->width, d->height);
  if (a.user_prev) a.ucam_prev = make_user_camera(s->pose_cam, d->width, d->height);
  else a.cam_prev = make_camera(s->pose_cam, d->width, d->height);
  a.width = d->width, a.height = d->height;
  a.pix = s->path_pix.p, a.npix = npix;
  a.prev_slots = s->pose_slots.p;
  a.motion = reinterpret_cast<float4*>(d_motion), a.guide = reinterpret_cast<float4*>(d_guide), a.ident = reinterpret_cast<uint4*>(d_ident);
  a.overflow = s->counts.p + kCntOverflow, a.spill = s->spill.p;
  launch_motion(st, s->dscene, a, k);
  return finish_traversal(s);
}

extern "C" int pbrhip_render_motion_device(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_motion, float* d_guide, uint32_t* d_ident) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_motion: NULL argument");
    return motion_impl(s, d, d_motion, d_guide, d_ident);
  });
}

extern "C" int pbrhip_render_motion(pbrhip_scene* s, const pbrhip_render_desc* d, float* motion, float* guide, uint32_t* ident) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_motion: NULL argument");
    if (int rc = check_render_desc(s, d)) return rc;
    if (!s->pose_set) return fail(PBRHIP_ESTATE, "render_motion: the scene has no pose snapshot (pbrhip_scene_snapshot_pose)");
    HIPCHK(hipSetDevice(s->device));
    const size_t npx = (size_t)d->width * d->height;
    Staging g(s->stream);
    float* const d_m = g.out(motion, npx * 4);
    float* const d_g = g.out(guide, npx * 4);
    uint32_t* const d_i = g.out(ident, npx * 4);
    if (int rc = g.ready()) return rc;
    if (int rc = motion_impl(s, d, d_m, d_g, d_i)) return rc;
    return g.finish();
  });
}

// the accumulation's arguments, host or device
struct TemporalPtrs {
  const float* rgba;
  const uint32_t* count;
  const float *motion, *guide, *hist_rgba, *hist_guide;
  float* out_rgba;
};
struct TemporalParams {
  float alpha_min, sigma_depth, normal_cos_min;
  uint32_t max_history;
};

// the checks both accumulation entry points share, before any device work
static int check_temporal(int device, uint32_t width, uint32_t height, const TemporalPtrs& p, const TemporalParams& q) {
  if (!p.rgba || !p.count || !p.motion || !p.guide || !p.out_rgba) return fail(PBRHIP_EINVAL, "temporal_accumulate: NULL rgba, count, motion, guide or out_rgba");
  if ((p.hist_rgba != nullptr) != (p.hist_guide != nullptr)) return fail(PBRHIP_EINVAL, "temporal_accumulate: hist_rgba and hist_guide come together or not at all");
  if (int rc = check_image("temporal_accumulate", width, height)) return rc;
  if (q.alpha_min != q.alpha_min || q.sigma_depth != q.sigma_depth || q.normal_cos_min != q.normal_cos_min) return fail(PBRHIP_EINVAL, "temporal_accumulate: a parameter is NaN");
  if (q.max_history == 0 || q.max_history > (1u << 24)) return fail(PBRHIP_EINVAL, "temporal_accumulate: max_history %u is not in [1, 2^24]", q.max_history);
  if (p.out_rgba == p.hist_rgba) return fail(PBRHIP_EINVAL, "temporal_accumulate: out_rgba is hist_rgba (the taps of one pixel read what another wrote)");
  return check_device("temporal_accumulate", device);
}

// one launch on the device's null stream
static int temporal_impl(int device, uint32_t width, uint32_t height, const TemporalPtrs& p, const TemporalParams& q) {
  HIPCHK(hipSetDevice(device));
  TemporalArgs a{};
  a.width = width, a.height = height;
  a.rgba = reinterpret_cast<const float4*>(p.rgba), a.count = p.count;
  a.motion = reinterpret_cast<const float4*>(p.motion), a.guide = reinterpret_cast<const float4*>(p.guide);
  a.hist_rgba = reinterpret_cast<const float4*>(p.hist_rgba), a.hist_guide = reinterpret_cast<const float4*>(p.hist_guide);
  a.alpha_min = q.alpha_min, a.sigma_depth = q.sigma_depth, a.normal_cos_min = q.normal_cos_min, a.max_history = (float)q.max_history;
  a.out = reinterpret_cast<float4*>(p.out_rgba);
  launch_temporal(nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_temporal_accumulate_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                                 const float* d_motion, const float* d_guide, const float* d_hist_rgba, const float* d_hist_guide,
                                                 float alpha_min, float sigma_depth, float normal_cos_min, uint32_t max_history, float* d_out_rgba) {
  return guarded([&]() -> int {
    const TemporalPtrs p{d_rgba, d_count, d_motion, d_guide, d_hist_rgba, d_hist_guide, d_out_rgba};
    const TemporalParams q{alpha_min, sigma_depth, normal_cos_min, max_history};
    if (int rc = check_temporal(device, width, height, p, q)) return rc;
    return temporal_impl(device, width, height, p, q);
  });
}

extern "C" int pbrhip_temporal_accumulate(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* motion,
                                          const float* guide, const float* hist_rgba, const float* hist_guide, float alpha_min, float sigma_depth,
                                          float normal_cos_min, uint32_t max_history, float* out_rgba) {
  return guarded([&]() -> int {
    const TemporalPtrs h{rgba, count, motion, guide, hist_rgba, hist_guide, out_rgba};
    const TemporalParams q{alpha_min, sigma_depth, normal_cos_min, max_history};
    if (int rc = check_temporal(device, width, height, h, q)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const TemporalPtrs p{g.in(rgba, npx * 4), g.in(count, npx), g.in(motion, npx * 4), g.in(guide, npx * 4),
                         g.in(hist_rgba, npx * 4), g.in(hist_guide, npx * 4), g.out(out_rgba, npx * 4)};
    if (int rc = g.ready()) return rc;
    if (int rc = temporal_impl(device, width, height, p, q)) return rc;
    return g.finish();
  });
}

// ------------------------------------------------------------------ variance-guided filtering
static int check_object_ids(pbrhip_scene* s, const void* ident, size_t num_pixels, uint32_t what, const void* ids) {
  if (!s) return fail(PBRHIP_EINVAL, "scene_object_ids: scene is NULL");
  if (what > PBRHIP_ID_GEOM) return fail(PBRHIP_EINVAL, "scene_object_ids: unknown id %u", what);
  if (num_pixels && (!ident || !ids)) return fail(PBRHIP_EINVAL, "scene_object_ids: NULL ident or ids");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  return PBRHIP_OK;
}

// one launch on the scene's stream; device pointers.  The caller copies out behind it, or synchronises.
static int object_ids_impl(pbrhip_scene* s, const uint32_t* d_ident, size_t num_pixels, uint32_t what, uint32_t* d_ids) {
  launch_object_ids(s->stream, s->dscene.shade, s->tree.num_slots, reinterpret_cast<const uint4*>(d_ident), num_pixels, what, d_ids);
  HIPCHK(hipGetLastError());
  return PBRHIP_OK;
}

extern "C" int pbrhip_scene_object_ids_device(pbrhip_scene* s, const void* d_ident, size_t num_pixels, uint32_t what, void* d_ids, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_object_ids(s, d_ident, num_pixels, what, d_ids)) return rc;
    if (!num_pixels) return PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = wait_for_caller_stream(s, stream)) return rc;
    if (int rc = object_ids_impl(s, static_cast<const uint32_t*>(d_ident), num_pixels, what, static_cast<uint32_t*>(d_ids))) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}

extern "C" int pbrhip_scene_object_ids(pbrhip_scene* s, const uint32_t* ident, size_t num_pixels, uint32_t what, uint32_t* ids) {
  return guarded([&]() -> int {
    if (int rc = check_object_ids(s, ident, num_pixels, what, ids)) return rc;
    if (!num_pixels) return PBRHIP_OK;
    HIPCHK(hipSetDevice(s->device));
    Staging g(s->stream);
    const uint32_t* const d_ident = g.in(ident, num_pixels * 4);
    uint32_t* const d_ids = g.out(ids, num_pixels);
    if (int rc = g.ready()) return rc;
    if (int rc = object_ids_impl(s, d_ident, num_pixels, what, d_ids)) return rc;
    return g.finish();
  });
}

// the accumulation's pointers, host or device: the checks and both entry points pass them as one
struct SvgfAccumPtrs {
  const float* rgba;
  const uint32_t* count;
  const float* albedo_hits;
  const uint32_t* feature_count;
  const float *motion, *guide;
  const uint32_t* ids;
  const float *hist_illum, *hist_var, *hist_guide;
  const uint32_t* hist_ids;
  float *out_illum, *out_var;
};

// the checks both accumulation entry points share, before any device work
static int check_svgf_accumulate(int device, uint32_t width, uint32_t height, const SvgfAccumPtrs& p, float alpha_min, float sigma_depth,
                                 float normal_cos_min, uint32_t max_history) {
  if (!p.rgba || !p.count || !p.motion || !p.guide || !p.out_illum || !p.out_var)
    return fail(PBRHIP_EINVAL, "svgf_accumulate: NULL rgba, count, motion, guide, out_illum or out_var");
  if ((p.albedo_hits != nullptr) != (p.feature_count != nullptr)) return fail(PBRHIP_EINVAL, "svgf_accumulate: albedo_hits and feature_count come together or not at all");
  const int nhist = (p.hist_illum ? 1 : 0) + (p.hist_var ? 1 : 0) + (p.hist_guide ? 1 : 0);
  if (nhist != 0 && nhist != 3) return fail(PBRHIP_EINVAL, "svgf_accumulate: hist_illum, hist_var and hist_guide come together or not at all");
  if ((p.hist_ids != nullptr) != (p.ids != nullptr && nhist == 3))
    return fail(PBRHIP_EINVAL, "svgf_accumulate: hist_ids is given exactly when ids is given and a history is present");
  if (int rc = check_image("svgf_accumulate", width, height)) return rc;
  if (alpha_min != alpha_min || sigma_depth != sigma_depth || normal_cos_min != normal_cos_min) return fail(PBRHIP_EINVAL, "svgf_accumulate: a parameter is NaN");
  if (alpha_min < 0.0f || alpha_min > 1.0f) return fail(PBRHIP_EINVAL, "svgf_accumulate: alpha_min %g is not in [0, 1]", (double)alpha_min);
  if (max_history == 0 || max_history > (1u << 24)) return fail(PBRHIP_EINVAL, "svgf_accumulate: max_history %u is not in [1, 2^24]", max_history);
  const void* outs[2] = {p.out_illum, p.out_var};
  const void* hists[4] = {p.hist_illum, p.hist_var, p.hist_guide, p.hist_ids};
  for (const void* o : outs)
    for (const void* h : hists)
      if (h && o == h) return fail(PBRHIP_EINVAL, "svgf_accumulate: an output is a history buffer (the taps of one pixel read what another wrote)");
  if ((const void*)p.out_illum == (const void*)p.out_var) return fail(PBRHIP_EINVAL, "svgf_accumulate: out_illum is out_var");
  return check_device("svgf_accumulate", device);
}

// one launch on the device's null stream; device pointers
static int svgf_accumulate_impl(int device, uint32_t width, uint32_t height, const SvgfAccumPtrs& p, float alpha_min, float sigma_depth,
                                float normal_cos_min, uint32_t max_history) {
  HIPCHK(hipSetDevice(device));
  SvgfAccumArgs a{};
  a.width = width, a.height = height;
  a.rgba = reinterpret_cast<const float4*>(p.rgba), a.count = p.count;
  a.albedo_hits = reinterpret_cast<const float4*>(p.albedo_hits), a.feature_count = p.feature_count;
  a.motion = reinterpret_cast<const float4*>(p.motion), a.guide = reinterpret_cast<const float4*>(p.guide), a.ids = p.ids;
  a.hist_illum = reinterpret_cast<const float4*>(p.hist_illum), a.hist_var = p.hist_var;
  a.hist_guide = reinterpret_cast<const float4*>(p.hist_guide), a.hist_ids = p.hist_ids;
  a.alpha_min = alpha_min, a.sigma_depth = sigma_depth, a.normal_cos_min = normal_cos_min, a.max_history = (float)max_history;
  a.out_illum = reinterpret_cast<float4*>(p.out_illum), a.out_var = p.out_var;
  launch_svgf_accumulate(nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_svgf_accumulate_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                             const float* d_albedo_hits, const uint32_t* d_feature_count, const float* d_motion,
                                             const float* d_guide, const uint32_t* d_ids, const float* d_hist_illum, const float* d_hist_var,
                                             const float* d_hist_guide, const uint32_t* d_hist_ids, float alpha_min, float sigma_depth,
                                             float normal_cos_min, uint32_t max_history, float* d_out_illum, float* d_out_var) {
  return guarded([&]() -> int {
    const SvgfAccumPtrs p{d_rgba, d_count, d_albedo_hits, d_feature_count, d_motion, d_guide, d_ids, d_hist_illum, d_hist_var, d_hist_guide,
                          d_hist_ids, d_out_illum, d_out_var};
    if (int rc = check_svgf_accumulate(device, width, height, p, alpha_min, sigma_depth, normal_cos_min, max_history)) return rc;
    return svgf_accumulate_impl(device, width, height, p, alpha_min, sigma_depth, normal_cos_min, max_history);
  });
}

extern "C" int pbrhip_svgf_accumulate(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* albedo_hits,
                                      const uint32_t* feature_count, const float* motion, const float* guide, const uint32_t* ids,
                                      const float* hist_illum, const float* hist_var, const float* hist_guide, const uint32_t* hist_ids,
                                      float alpha_min, float sigma_depth, float normal_cos_min, uint32_t max_history, float* out_illum,
                                      float* out_var) {
  return guarded([&]() -> int {
    const SvgfAccumPtrs h{rgba, count, albedo_hits, feature_count, motion, guide, ids, hist_illum, hist_var, hist_guide, hist_ids, out_illum, out_var};
    if (int rc = check_svgf_accumulate(device, width, height, h, alpha_min, sigma_depth, normal_cos_min, max_history)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const SvgfAccumPtrs p{g.in(rgba, npx * 4), g.in(count, npx), g.in(albedo_hits, npx * 4), g.in(feature_count, npx), g.in(motion, npx * 4),
                          g.in(guide, npx * 4), g.in(ids, npx), g.in(hist_illum, npx * 4), g.in(hist_var, npx), g.in(hist_guide, npx * 4),
                          g.in(hist_ids, npx), g.out(out_illum, npx * 4), g.out(out_var, npx)};
    if (int rc = g.ready()) return rc;
    if (int rc = svgf_accumulate_impl(device, width, height, p, alpha_min, sigma_depth, normal_cos_min, max_history)) return rc;
    return g.finish();
  });
}

// the filter's pointers, host or device
struct SvgfFilterPtrs {
  const float *illum, *var, *guide;
  const uint32_t* ids;
  const float* albedo_hits;
  const uint32_t* feature_count;
  float *out_rgba, *out_feedback;
};
struct SvgfFilterParams {
  uint32_t iterations;
  float sigma_lum, sigma_depth;
  uint32_t normal_squarings;
};

// the checks both filter entry points share; resolves the iteration default
static int check_svgf_filter(int device, uint32_t width, uint32_t height, const SvgfFilterPtrs& p, SvgfFilterParams& q) {
  if (!p.illum || !p.var || !p.guide || !p.out_rgba) return fail(PBRHIP_EINVAL, "svgf_filter: NULL illum, var, guide or out_rgba");
  if ((p.albedo_hits != nullptr) != (p.feature_count != nullptr)) return fail(PBRHIP_EINVAL, "svgf_filter: albedo_hits and feature_count come together or not at all");
  if (int rc = check_image("svgf_filter", width, height)) return rc;
  if (q.sigma_lum != q.sigma_lum || q.sigma_depth != q.sigma_depth) return fail(PBRHIP_EINVAL, "svgf_filter: a sigma is NaN");
  if (q.iterations > 8) return fail(PBRHIP_EINVAL, "svgf_filter: %u iterations (at most 8)", q.iterations);
  if (q.normal_squarings > 16) return fail(PBRHIP_EINVAL, "svgf_filter: %u normal squarings (at most 16)", q.normal_squarings);
  if (p.out_rgba == p.illum || p.out_rgba == p.guide || p.out_feedback == p.illum || p.out_feedback == p.guide || p.out_feedback == p.out_rgba)
    return fail(PBRHIP_EINVAL, "svgf_filter: an output is an input or the other output (the taps of one pixel read what another wrote)");
  if (q.iterations == 0) q.iterations = PBRHIP_SVGF_ITERATIONS;
  return check_device("svgf_filter", device);
}

// prepare + one launch per iteration on the device's null stream; the two temporaries (e | v, twice) live for the call
static int svgf_filter_impl(int device, uint32_t width, uint32_t height, const SvgfFilterPtrs& p, const SvgfFilterParams& q) {
  HIPCHK(hipSetDevice(device));
  const size_t npx = (size_t)width * height;
  DevBuf<float4> e0, e1;
  HIPCHK(e0.reserve(npx));
  if (q.iterations > 1) HIPCHK(e1.reserve(npx));
  SvgfFilterArgs a{};
  a.width = width, a.height = height;
  a.illum = reinterpret_cast<const float4*>(p.illum), a.var = p.var, a.guide = reinterpret_cast<const float4*>(p.guide), a.ids = p.ids;
  a.albedo_hits = reinterpret_cast<const float4*>(p.albedo_hits), a.feature_count = p.feature_count;
  a.sigma_lum = q.sigma_lum, a.sigma_depth = q.sigma_depth, a.normal_squarings = q.normal_squarings;
  launch_svgf_prepare(nullptr, a, e0.p);
  HIPCHK(hipGetLastError());
  for (uint32_t i = 0; i < q.iterations; i++) {
    const bool last = i + 1 == q.iterations;
    float4* const src = (i & 1u) ? e1.p : e0.p;
    float4* const dst = last ? reinterpret_cast<float4*>(p.out_rgba) : ((i & 1u) ? e0.p : e1.p);
    launch_svgf_iteration(nullptr, a, i, last, src, dst, i == 0 ? reinterpret_cast<float4*>(p.out_feedback) : nullptr);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_svgf_filter_device(int device, uint32_t width, uint32_t height, const float* d_illum, const float* d_var, const float* d_guide,
                                         const uint32_t* d_ids, const float* d_albedo_hits, const uint32_t* d_feature_count, uint32_t iterations,
                                         float sigma_lum, float sigma_depth, uint32_t normal_squarings, float* d_out_rgba, float* d_out_feedback) {
  return guarded([&]() -> int {
    const SvgfFilterPtrs p{d_illum, d_var, d_guide, d_ids, d_albedo_hits, d_feature_count, d_out_rgba, d_out_feedback};
    SvgfFilterParams q{iterations, sigma_lum, sigma_depth, normal_squarings};
    if (int rc = check_svgf_filter(device, width, height, p, q)) return rc;
    return svgf_filter_impl(device, width, height, p, q);
  });
}

extern "C" int pbrhip_svgf_filter(int device, uint32_t width, uint32_t height, const float* illum, const float* var, const float* guide,
                                  const uint32_t* ids, const float* albedo_hits, const uint32_t* feature_count, uint32_t iterations, float sigma_lum,
                                  float sigma_depth, uint32_t normal_squarings, float* out_rgba, float* out_feedback) {
  return guarded([&]() -> int {
    const SvgfFilterPtrs h{illum, var, guide, ids, albedo_hits, feature_count, out_rgba, out_feedback};
    SvgfFilterParams q{iterations, sigma_lum, sigma_depth, normal_squarings};
    if (int rc = check_svgf_filter(device, width, height, h, q)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const SvgfFilterPtrs p{g.in(illum, npx * 4), g.in(var, npx), g.in(guide, npx * 4), g.in(ids, npx),
                           g.in(albedo_hits, npx * 4), g.in(feature_count, npx), g.out(out_rgba, npx * 4), g.out(out_feedback, npx * 4)};
    if (int rc = g.ready()) return rc;
    if (int rc = svgf_filter_impl(device, width, height, p, q)) return rc;
    return g.finish();
  });
}

// ------------------------------------------------------------------ the first-hit emission layer
extern "C" int pbrhip_render_features_emission_device(pbrhip_scene* s, const pbrhip_render_desc* d, float* d_albedo_hits, float* d_normal_depth,
                                                      uint32_t* d_count, float* d_emission) {
  return guarded([&]() -> int {
    if (!s || !d) return fail(PBRHIP_EINVAL, "render_features: NULL argument");
    return features_impl(s, d, d_albedo_hits, d_normal_depth, d_count, nullptr, true, d_emission);
  });
}

extern "C" int pbrhip_render_features_emission(pbrhip_scene* s, const pbrhip_render_desc* d, float* albedo_hits, float* normal_depth,
                                               uint32_t* count, float* emission) {
  return guarded([&]() -> int { return features_host(s, d, albedo_hits, normal_depth, count, true, emission); });
}

// the pointers of pbrhip_emission_split, host or device
struct EmissionSplitPtrs {
  const float* rgba;
  const uint32_t* count;
  const float *emission, *albedo_hits;
  const uint32_t* feature_count;
  float *out_rgba, *out_albedo_hits;
};

// the checks both split entry points share, before any device work
static int check_emission_split(int device, uint32_t width, uint32_t height, const EmissionSplitPtrs& p) {
  if (int rc = check_image("emission_split", width, height)) return rc;
  if (!p.rgba || !p.count || !p.emission || !p.out_rgba) return fail(PBRHIP_EINVAL, "emission_split: NULL rgba, count, emission or out_rgba");
  const int nal = (p.albedo_hits ? 1 : 0) + (p.feature_count ? 1 : 0) + (p.out_albedo_hits ? 1 : 0);
  if (nal != 0 && nal != 3) return fail(PBRHIP_EINVAL, "emission_split: albedo_hits, feature_count and out_albedo_hits come together or not at all");
  const void* ins[4] = {p.rgba, p.count, p.emission, p.feature_count};
  for (const void* in : ins)
    if (p.out_albedo_hits && (const void*)p.out_albedo_hits == in)
      return fail(PBRHIP_EINVAL, "emission_split: out_albedo_hits is an input other than albedo_hits");
  if (p.out_albedo_hits && (const void*)p.out_albedo_hits == (const void*)p.out_rgba) return fail(PBRHIP_EINVAL, "emission_split: out_albedo_hits is out_rgba");
  const void* others[4] = {p.count, p.emission, p.albedo_hits, p.feature_count};
  for (const void* in : others)
    if (in && (const void*)p.out_rgba == in) return fail(PBRHIP_EINVAL, "emission_split: out_rgba is an input other than rgba");
  return check_device("emission_split", device);
}

// one launch on the device's null stream; device pointers
static int emission_split_impl(int device, uint32_t width, uint32_t height, const EmissionSplitPtrs& p) {
  HIPCHK(hipSetDevice(device));
  EmissionSplitArgs a{};
  a.npx = (size_t)width * height;
  a.rgba = reinterpret_cast<const float4*>(p.rgba), a.count = p.count, a.emission = reinterpret_cast<const float4*>(p.emission);
  a.albedo_hits = reinterpret_cast<const float4*>(p.albedo_hits), a.feature_count = p.feature_count;
  a.out_rgba = reinterpret_cast<float4*>(p.out_rgba), a.out_albedo_hits = reinterpret_cast<float4*>(p.out_albedo_hits);
  launch_emission_split(nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_emission_split_device(int device, uint32_t width, uint32_t height, const float* d_rgba, const uint32_t* d_count,
                                            const float* d_emission, const float* d_albedo_hits, const uint32_t* d_feature_count,
                                            float* d_out_rgba, float* d_out_albedo_hits) {
  return guarded([&]() -> int {
    const EmissionSplitPtrs p{d_rgba, d_count, d_emission, d_albedo_hits, d_feature_count, d_out_rgba, d_out_albedo_hits};
    if (int rc = check_emission_split(device, width, height, p)) return rc;
    return emission_split_impl(device, width, height, p);
  });
}

extern "C" int pbrhip_emission_split(int device, uint32_t width, uint32_t height, const float* rgba, const uint32_t* count, const float* emission,
                                     const float* albedo_hits, const uint32_t* feature_count, float* out_rgba, float* out_albedo_hits) {
  return guarded([&]() -> int {
    const EmissionSplitPtrs h{rgba, count, emission, albedo_hits, feature_count, out_rgba, out_albedo_hits};
    if (int rc = check_emission_split(device, width, height, h)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const EmissionSplitPtrs p{g.in(rgba, npx * 4), g.in(count, npx), g.in(emission, npx * 4), g.in(albedo_hits, npx * 4),
                              g.in(feature_count, npx), g.out(out_rgba, npx * 4), g.out(out_albedo_hits, npx * 4)};
    if (int rc = g.ready()) return rc;
    if (int rc = emission_split_impl(device, width, height, p)) return rc;
    return g.finish();
  });
}

static int check_emission_merge(int device, uint32_t width, uint32_t height, const void* filtered, const void* emission, const void* count,
                                const void* out_rgba) {
  if (int rc = check_image("emission_merge", width, height)) return rc;
  if (!filtered || !emission || !count || !out_rgba) return fail(PBRHIP_EINVAL, "emission_merge: NULL filtered_rgba, emission, count or out_rgba");
  if (out_rgba == emission || out_rgba == count) return fail(PBRHIP_EINVAL, "emission_merge: out_rgba is an input other than filtered_rgba");
  return check_device("emission_merge", device);
}

static int emission_merge_impl(int device, uint32_t width, uint32_t height, const float* filtered, const float* emission, const uint32_t* count,
                               float* out_rgba) {
  HIPCHK(hipSetDevice(device));
  EmissionMergeArgs a{};
  a.npx = (size_t)width * height;
  a.filtered = reinterpret_cast<const float4*>(filtered), a.emission = reinterpret_cast<const float4*>(emission), a.count = count;
  a.out = reinterpret_cast<float4*>(out_rgba);
  launch_emission_merge(nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  return PBRHIP_OK;
}

extern "C" int pbrhip_emission_merge_device(int device, uint32_t width, uint32_t height, const float* d_filtered_rgba, const float* d_emission,
                                            const uint32_t* d_count, float* d_out_rgba) {
  return guarded([&]() -> int {
    if (int rc = check_emission_merge(device, width, height, d_filtered_rgba, d_emission, d_count, d_out_rgba)) return rc;
    return emission_merge_impl(device, width, height, d_filtered_rgba, d_emission, d_count, d_out_rgba);
  });
}

extern "C" int pbrhip_emission_merge(int device, uint32_t width, uint32_t height, const float* filtered_rgba, const float* emission,
                                     const uint32_t* count, float* out_rgba) {
  return guarded([&]() -> int {
    if (int rc = check_emission_merge(device, width, height, filtered_rgba, emission, count, out_rgba)) return rc;
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    Staging g;
    const float* const d_f = g.in(filtered_rgba, npx * 4);
    const float* const d_e = g.in(emission, npx * 4);
    const uint32_t* const d_c = g.in(count, npx);
    float* const d_out = g.out(out_rgba, npx * 4);
    if (int rc = g.ready()) return rc;
    if (int rc = emission_merge_impl(device, width, height, d_f, d_e, d_c, d_out)) return rc;
    return g.finish();
  });
}
