// render_adaptive.cpp -- adaptive sampling (pbrhip_render_adaptive): rounds of render_impl over a pixel list that shrinks,
// with one decision step (adaptive.hip) between two rounds.  Host C++ only.
//
// Levels n_0 = first_level, n_k = min(2 n_{k-1}, num_sample).  Round 0 renders passes [first_pass, first_pass + n_0) of every pixel
// of the rank, round k >= 1 the passes [first_pass + n_{k-1}, first_pass + n_k) of the pixels of the tiles still active; after every
// round k >= 1 the tiles whose error estimate is at most the threshold leave the list for good.  Every round continues the layer
// (PBRHIP_RENDER_NO_CLEAR), so pixel p holds, bit for bit, what a plain render of count[p] passes holds at p.
#include <string.h>

#include "adaptive_kernels.h"
#include "scene_impl.h"

using namespace pb;

namespace {
struct Levels {
  uint32_t first, max;
  uint32_t next(uint32_t n) const { return n >= max - n ? max : 2u * n; }  // min(2 n, max) without overflow
};

int check_threshold(float threshold, const char* who) {
  if (!(threshold >= 0.0f)) return fail(PBRHIP_EINVAL, "%s: the threshold is negative or NaN", who);
  return PBRHIP_OK;
}

// The rank's tiles in the order their pixels first appear in ensure_pixels' list.  With the default knobs that list's patches ARE the
// tiles, so round 0 and (while no tile stops) every later round enqueue what a plain render enqueues, in the same scattered order;
// with other knobs this is merely some order of the same tiles, and no image depends on the order.
int ensure_tiles0(pbrhip_scene* s, uint32_t width, uint32_t height) {
  AdaptiveBufs& as = s->as;
  const uint32_t key[7] = {s->pk_w, s->pk_h, s->pk_rank, s->pk_world, s->pk_block, s->pk_tile, s->pk_npix};
  if (!memcmp(key, as.key, sizeof(key)) && (!as.tiles0.empty() || s->pk_npix == 0)) return PBRHIP_OK;
  std::vector<uint32_t> pix(s->pk_npix);
  if (!pix.empty()) HIPCHK(hipMemcpy(pix.data(), s->path_pix.p, pix.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const uint32_t across = as_tiles_across(width);
  std::vector<uint8_t> seen((size_t)across * as_tiles_across(height), 0);
  as.tiles0.clear();
  for (uint32_t p : pix) {
    const uint32_t id = (p / width / kAsTile) * across + (p % width) / kAsTile;
    if (!seen[id]) seen[id] = 1, as.tiles0.push_back(id);
  }
  memcpy(as.key, key, sizeof(key));
  return PBRHIP_OK;
}

// the body of pbrhip_render_adaptive_device: device pointers on the scene's device; d_tile_error may be null
int adaptive_impl(pbrhip_scene* s, const pbrhip_render_desc* d0, float threshold, uint32_t first_level, const volatile unsigned char* cancel,
                  float* d_rgba, uint32_t* d_count, float* d_tile_error, size_t* finish_pass, uint64_t* samples, uint32_t* rounds) {
  if (d0->flags & PBRHIP_RENDER_NO_CLEAR) return fail(PBRHIP_EINVAL, "render_adaptive: PBRHIP_RENDER_NO_CLEAR (an adaptive layer cannot be resumed)");
  if (int rc = check_threshold(threshold, "render_adaptive")) return rc;
  if (d0->num_sample == 0) return fail(PBRHIP_EINVAL, "render_adaptive: no samples");
  if (d0->shard_block % kAsTile != 0) return fail(PBRHIP_EINVAL, "render_adaptive: shard_block %u is not a multiple of %u", d0->shard_block, kAsTile);
  if ((uint64_t)d0->first_pass + d0->num_sample > (1ull << 32)) return fail(PBRHIP_EINVAL, "render_adaptive: the passes do not fit 32 bits");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  PB_NOT_STALE(s);
  if (d0->width == 0 || d0->height == 0) return fail(PBRHIP_EINVAL, "empty image");
  if ((uint64_t)d0->width * d0->height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "image too large");
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  AdaptiveBufs& as = s->as;
  const uint32_t W = d0->width, H = d0->height;
  const size_t npx_img = (size_t)W * H;
  const uint32_t all_tiles = as_tiles_across(W) * as_tiles_across(H);
  const Levels lv{std::min(first_level ? first_level : PBRHIP_ADAPTIVE_FIRST_LEVEL, d0->num_sample), d0->num_sample};

  HIPCHK(as.tile_error.reserve(all_tiles));
  float* const terr = d_tile_error ? d_tile_error : as.tile_error.p;
  HIPCHK(hipMemsetAsync(d_rgba, 0, npx_img * 4 * sizeof(float), st));
  HIPCHK(hipMemsetAsync(d_count, 0, npx_img * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(terr, 0, all_tiles * sizeof(float), st));
  if (finish_pass) __atomic_store_n(finish_pass, (size_t)0, __ATOMIC_RELEASE);
  if (samples) *samples = 0;
  if (rounds) *rounds = 0;

  pbrhip_render_desc d = *d0;
  d.flags = (d0->flags | PBRHIP_RENDER_NO_CLEAR) & ~(PBRHIP_RENDER_STATS | PBRHIP_RENDER_TIMING | PBRHIP_RENDER_TIMING_TRACE);
  uint64_t total = 0;
  uint32_t nrounds = 0, level = 0;                 // level: passes the active pixels hold
  const uint32_t* pixels = nullptr;                // null: ensure_pixels' list (every pixel of the rank)
  uint32_t npix = 0, ntiles = 0, cur = 0;          // of the active list; cur: which of as.tiles holds it
  bool every_tile_active = true;
  for (;;) {
    const uint32_t target = level == 0 ? lv.first : lv.next(level);
    d.first_pass = d0->first_pass + level, d.num_sample = target - level;
    pbrhip_render_stats S;
    if (int rc = render_impl(s, &d, cancel, d_rgba, d_count, nullptr, &S, pixels, npix)) return rc;
    if (level == 0) {  // round 0 (ensure_pixels has run: the rank's pixels and tiles are known)
      npix = s->pk_npix;
      if (npix == 0) break;  // a rank without tiles: the zeroed layer
      if (int rc = ensure_tiles0(s, W, H)) return rc;
      ntiles = (uint32_t)as.tiles0.size();
      HIPCHK(as.tiles[0].reserve(ntiles));
      HIPCHK(as.tiles[1].reserve(ntiles));
      HIPCHK(as.keep.reserve(ntiles));
      HIPCHK(as.tile_off.reserve(ntiles));
      HIPCHK(as.pix_off.reserve(ntiles));
      HIPCHK(as.totals.reserve(2));
      HIPCHK(as.pixels.reserve(npix));
      HIPCHK(as.snapshot.reserve(npx_img));
      HIPCHK(hipMemcpyAsync(as.tiles[0].p, as.tiles0.data(), ntiles * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    const uint32_t done = (uint32_t)S.passes_done;
    nrounds += done ? 1u : 0u, total += (uint64_t)done * npix;  // (a round cancelled before its first pass is none)
    const uint32_t prev = level;
    level += done;
    if (samples) *samples = total;
    if (rounds) *rounds = nrounds;
    if (finish_pass && every_tile_active) __atomic_store_n(finish_pass, (size_t)level, __ATOMIC_RELEASE);
    if (done < d.num_sample || (cancel && __atomic_load_n(cancel, __ATOMIC_RELAXED) != 0)) break;  // cancelled: no decision follows
    if (prev == 0) {  // round 0: A = the layer at level n_0 (from here on k_as_error keeps A up to date)
      if (level == lv.max) break;  // first_level >= num_sample: one plain round
      HIPCHK(hipMemcpyAsync(as.snapshot.p, d_rgba, npx_img * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
      continue;
    }
    AdaptiveArgs a;
    a.width = W, a.height = H, a.rgba = reinterpret_cast<const float4*>(d_rgba), a.snapshot = as.snapshot.p;
    a.n_prev = (float)prev, a.n_delta = (float)(level - prev), a.n_now = (float)level, a.threshold = (double)threshold;
    a.tiles_in = as.tiles[cur].p, a.num_tiles = ntiles, a.tile_error = terr;
    a.keep = as.keep.p, a.tile_off = as.tile_off.p, a.pix_off = as.pix_off.p, a.totals = as.totals.p;
    a.tiles_out = as.tiles[cur ^ 1u].p, a.pixels_out = as.pixels.p;
    launch_adaptive_step(st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_counts, as.totals.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (s->h_counts[0] > ntiles || s->h_counts[1] > npix) return fail(PBRHIP_EHIP, "render_adaptive: the active list grew");
    if (s->h_counts[0] != ntiles) every_tile_active = false;
    ntiles = s->h_counts[0], npix = s->h_counts[1], cur ^= 1u, pixels = as.pixels.p;
    if (level == lv.max || ntiles == 0) break;
  }
  HIPCHK(hipStreamSynchronize(st));
  return PBRHIP_OK;
}
}  // namespace

extern "C" int pbrhip_render_adaptive_device(pbrhip_scene* s, const pbrhip_render_desc* d, float threshold, uint32_t first_level,
                                             const volatile unsigned char* cancel, float* d_rgba, uint32_t* d_count, float* d_tile_error,
                                             size_t* finish_pass, uint64_t* samples, uint32_t* rounds) {
  return guarded([&]() -> int {
    if (!s || !d || !d_rgba || !d_count) return fail(PBRHIP_EINVAL, "render_adaptive: NULL argument");
    return adaptive_impl(s, d, threshold, first_level, cancel, d_rgba, d_count, d_tile_error, finish_pass, samples, rounds);
  });
}

extern "C" int pbrhip_render_adaptive(pbrhip_scene* s, const pbrhip_render_desc* d, float threshold, uint32_t first_level,
                                      const volatile unsigned char* cancel, float* rgba, uint32_t* count, float* tile_error,
                                      size_t* finish_pass, uint64_t* samples, uint32_t* rounds) {
  return guarded([&]() -> int {
    if (!s || !d || !rgba || !count) return fail(PBRHIP_EINVAL, "render_adaptive: NULL argument");
    if ((uint64_t)d->width * d->height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "image too large");
    HIPCHK(hipSetDevice(s->device));
    const size_t npx = (size_t)d->width * d->height;
    HIPCHK(s->own_rgba.reserve(npx * 4));
    HIPCHK(s->own_count.reserve(npx));
    if (int rc = adaptive_impl(s, d, threshold, first_level, cancel, s->own_rgba.p, s->own_count.p, nullptr, finish_pass, samples, rounds)) return rc;
    HIPCHK(hipMemcpyAsync(rgba, s->own_rgba.p, npx * 4 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipMemcpyAsync(count, s->own_count.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (tile_error)
      HIPCHK(hipMemcpyAsync(tile_error, s->as.tile_error.p, (size_t)as_tiles_across(d->width) * as_tiles_across(d->height) * sizeof(float),
                            hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PBRHIP_OK;
  });
}

// One decision step on caller-provided layers, without a scene: a test hook.
extern "C" int pbrhip_adaptive_step(int device, uint32_t width, uint32_t height, const float* rgba, float* snapshot_inout, uint32_t n_prev,
                                    uint32_t n_now, float threshold, const uint32_t* tiles_in, uint32_t num_tiles_in, uint32_t* tiles_out,
                                    uint32_t* num_tiles_out, uint32_t* pixels_out, uint32_t* num_pixels_out, float* tile_error_inout) {
  return guarded([&]() -> int {
    if (!rgba || !snapshot_inout || (!tiles_in && num_tiles_in) || !tiles_out || !num_tiles_out || !pixels_out || !num_pixels_out || !tile_error_inout)
      return fail(PBRHIP_EINVAL, "adaptive_step: NULL argument");
    if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 32)) return fail(PBRHIP_EINVAL, "adaptive_step: empty or too large an image");
    if (n_prev == 0 || n_now <= n_prev) return fail(PBRHIP_EINVAL, "adaptive_step: levels %u -> %u", n_prev, n_now);
    if (int rc = check_threshold(threshold, "adaptive_step")) return rc;
    const uint32_t all_tiles = as_tiles_across(width) * as_tiles_across(height);
    std::vector<uint8_t> seen(all_tiles, 0);  // (a tile listed twice would write its pixels twice: past the end of pixels_out)
    for (uint32_t i = 0; i < num_tiles_in; i++) {
      if (tiles_in[i] >= all_tiles || seen[tiles_in[i]]) return fail(PBRHIP_EINVAL, "adaptive_step: tile %u out of range or listed twice", tiles_in[i]);
      seen[tiles_in[i]] = 1;
    }
    int ndev = 0;
    if (int rc = pbrhip_device_count(&ndev)) return rc;
    if (ndev <= 0) return fail(PBRHIP_ENODEVICE, "no HIP device available: libpbrhip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(PBRHIP_EINVAL, "adaptive_step: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    const size_t npx = (size_t)width * height;
    DevBuf<float4> d_rgba, d_snap;
    DevBuf<float> d_err;
    DevBuf<uint32_t> d_in, d_out, d_pix, d_keep, d_toff, d_poff, d_tot;
    HIPCHK(d_rgba.reserve(npx));
    HIPCHK(d_snap.reserve(npx));
    HIPCHK(d_err.reserve(all_tiles));
    HIPCHK(d_in.reserve(num_tiles_in));
    HIPCHK(d_out.reserve(num_tiles_in));
    HIPCHK(d_pix.reserve(npx));
    HIPCHK(d_keep.reserve(num_tiles_in));
    HIPCHK(d_toff.reserve(num_tiles_in));
    HIPCHK(d_poff.reserve(num_tiles_in));
    HIPCHK(d_tot.reserve(2));
    HIPCHK(hipMemcpy(d_rgba.p, rgba, npx * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_snap.p, snapshot_inout, npx * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_err.p, tile_error_inout, all_tiles * sizeof(float), hipMemcpyHostToDevice));
    if (num_tiles_in) HIPCHK(hipMemcpy(d_in.p, tiles_in, num_tiles_in * sizeof(uint32_t), hipMemcpyHostToDevice));
    AdaptiveArgs a;
    a.width = width, a.height = height, a.rgba = d_rgba.p, a.snapshot = d_snap.p;
    a.n_prev = (float)n_prev, a.n_delta = (float)(n_now - n_prev), a.n_now = (float)n_now, a.threshold = (double)threshold;
    a.tiles_in = d_in.p, a.num_tiles = num_tiles_in, a.tile_error = d_err.p;
    a.keep = d_keep.p, a.tile_off = d_toff.p, a.pix_off = d_poff.p, a.totals = d_tot.p, a.tiles_out = d_out.p, a.pixels_out = d_pix.p;
    launch_adaptive_step(nullptr, a);
    HIPCHK(hipGetLastError());
    uint32_t tot[2] = {0, 0};
    HIPCHK(hipMemcpy(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost));  // (the null stream: the copy waits for the kernels)
    if (tot[0] > num_tiles_in || tot[1] > npx) return fail(PBRHIP_EHIP, "adaptive_step: the list grew");
    HIPCHK(hipMemcpy(snapshot_inout, d_snap.p, npx * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tile_error_inout, d_err.p, all_tiles * sizeof(float), hipMemcpyDeviceToHost));
    if (tot[0]) HIPCHK(hipMemcpy(tiles_out, d_out.p, tot[0] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tot[1]) HIPCHK(hipMemcpy(pixels_out, d_pix.p, (size_t)tot[1] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *num_tiles_out = tot[0], *num_pixels_out = tot[1];
    return PBRHIP_OK;
  });
}
