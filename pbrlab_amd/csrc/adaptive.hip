// adaptive.hip -- the decision kernels of adaptive sampling (pbrhip_render_adaptive).
//
//   k_as_error    one wave per active 8 x 8 tile, lane = pixel: the half-against-half error estimate e of every pixel in float32, the
//                 tile's mean E as a float64 butterfly over the wave, the snapshot A = I, and the tile's keep count
//   k_as_scan     exclusive prefix sums of the kept tiles and of their pixel counts, in list order (one block walks the list)
//   k_as_scatter  every kept tile writes its id and its row-major pixels at its offsets: the next round's lists, in a stable order
//
// The render kernels know nothing of this: they are handed the pixel list k_as_scatter wrote.  The lists are a subset of the rank's
// pixels in some order, and a pixel's value is a function of (pixel, pass) alone, so no image depends on anything here but the
// stop decisions.  All float32 arithmetic is rounded once per operation (no contraction); no LDS and no atomics in k_as_error.
// A translation unit of its own, linked after kernels.o: the render kernels' code object does not depend on it.
#include "adaptive_kernels.h"

namespace pb {

constexpr int kBlock = 256;                      // four tiles per block
constexpr int kTilesPerBlock = kBlock / 64;
constexpr int kScanBlock = 1024;                 // k_as_scan: one block, 16 waves
constexpr uint32_t kCanonicalNan = 0x7FC00000u;  // what a NaN E is stored as (the model's, too: NaN payloads are no part of the contract)

struct TileGeom {
  uint32_t x0, y0, cw, ch;  // origin, clipped width and height
};
__device__ __forceinline__ TileGeom tile_geom(uint32_t id, uint32_t width, uint32_t height) {
  const uint32_t across = (width + kAsTile - 1u) / kAsTile;
  TileGeom g;
  g.x0 = (id % across) * kAsTile, g.y0 = (id / across) * kAsTile;
  g.cw = min(kAsTile, width - g.x0), g.ch = min(kAsTile, height - g.y0);
  return g;
}

__global__ __launch_bounds__(kBlock) void k_as_error(AdaptiveArgs a) {
  const uint32_t t = blockIdx.x * kTilesPerBlock + threadIdx.x / 64u;  // wave-uniform
  if (t >= a.num_tiles) return;
  const uint32_t lane = threadIdx.x % 64u;
  const uint32_t id = a.tiles_in[t];
  const TileGeom g = tile_geom(id, a.width, a.height);
  const uint32_t lx = lane % kAsTile, ly = lane / kAsTile;
  double v = 0.0;  // an absent lane of a clipped tile contributes 0
  if (lx < g.cw && ly < g.ch) {
    const uint32_t p = (g.y0 + ly) * a.width + g.x0 + lx;
    const float4 I = a.rgba[p], A = a.snapshot[p];
    a.snapshot[p] = I;
    const float ar = A.x / a.n_prev, ag = A.y / a.n_prev, ab = A.z / a.n_prev;
    const float br = (I.x - A.x) / a.n_delta, bg = (I.y - A.y) / a.n_delta, bb = (I.z - A.z) / a.n_delta;
    const float mr = I.x / a.n_now, mg = I.y / a.n_now, mb = I.z / a.n_now;
    const float d = fabsf(ar - br) + fabsf(ag - bg) + fabsf(ab - bb);
    const float s = mr + mg + mb;
    v = (double)(d / sqrtf(s + 1e-3f));
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o);
  if (lane == 0u) {
    const uint32_t n = g.cw * g.ch;
    const double E = v / (double)n;
    a.tile_error[id] = E != E ? __uint_as_float(kCanonicalNan) : (float)E;
    a.keep[t] = E <= a.threshold ? 0u : n;  // (a NaN compares false: the tile stays active)
  }
}

// inclusive sum over the wave's lanes below and including this one
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)v, o);
    if (lane >= (uint32_t)o) v += up;
  }
  return v;
}

// One block walks the list kScanBlock entries at a time and carries the sums on: per entry the number of kept tiles before it (a
// ballot and mbcnt inside the wave) and the pixels of those tiles (a shuffle scan inside the wave), the waves' totals handed over
// through LDS once per turn.  A few hundred thousand tiles are a few hundred turns.
__global__ __launch_bounds__(kScanBlock) void k_as_scan(AdaptiveArgs a) {
  __shared__ uint32_t w_tiles[kScanBlock / 64], w_pix[kScanBlock / 64];
  const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
  uint32_t carry_tiles = 0u, carry_pix = 0u;
  for (uint32_t base = 0u; base < a.num_tiles; base += kScanBlock) {  // (block-uniform: every thread takes every turn)
    const uint32_t t = base + threadIdx.x;
    const uint32_t n = t < a.num_tiles ? a.keep[t] : 0u;
    const unsigned long long kept = __ballot(n != 0u);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
    const uint32_t incl = wave_inclusive_sum(n, lane);
    if (lane == 63u) w_tiles[wave] = (uint32_t)__popcll(kept), w_pix[wave] = incl;
    __syncthreads();
    uint32_t off_tiles = carry_tiles, off_pix = carry_pix, all_tiles = 0u, all_pix = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kScanBlock / 64; w++) {
      const uint32_t wt = w_tiles[w], wp = w_pix[w];
      if (w < wave) off_tiles += wt, off_pix += wp;
      all_tiles += wt, all_pix += wp;
    }
    if (t < a.num_tiles) a.tile_off[t] = off_tiles + before, a.pix_off[t] = off_pix + incl - n;
    carry_tiles += all_tiles, carry_pix += all_pix;
    __syncthreads();  // w_tiles / w_pix are rewritten in the next turn
  }
  if (threadIdx.x == 0u) a.totals[0] = carry_tiles, a.totals[1] = carry_pix;
}

__global__ __launch_bounds__(kBlock) void k_as_scatter(AdaptiveArgs a) {
  const uint32_t t = blockIdx.x * kTilesPerBlock + threadIdx.x / 64u;
  if (t >= a.num_tiles) return;
  const uint32_t n = a.keep[t];
  if (n == 0u) return;
  const uint32_t lane = threadIdx.x % 64u;
  const uint32_t id = a.tiles_in[t];
  const TileGeom g = tile_geom(id, a.width, a.height);  // (n == g.cw * g.ch)
  if (lane == 0u) a.tiles_out[a.tile_off[t]] = id;
  if (lane < n) a.pixels_out[a.pix_off[t] + lane] = (g.y0 + lane / g.cw) * a.width + g.x0 + lane % g.cw;
}

void launch_adaptive_step(hipStream_t s, const AdaptiveArgs& a) {
  if (a.num_tiles) {
    const dim3 grid((a.num_tiles + kTilesPerBlock - 1) / kTilesPerBlock);
    hipLaunchKernelGGL(k_as_error, grid, dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_as_scan, dim3(1), dim3(kScanBlock), 0, s, a);
    hipLaunchKernelGGL(k_as_scatter, grid, dim3(kBlock), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_as_scan, dim3(1), dim3(kScanBlock), 0, s, a);  // writes the two zero totals
  }
}

}  // namespace pb
