// adaptive_kernels.h -- launch interface of the decision kernels of adaptive sampling (adaptive.hip).  DESIGN.md §13.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pb {

constexpr uint32_t kAsTile = 8;  // edge of a tile: a wave is a tile, lane = (y & 7) * 8 + (x & 7)
inline uint32_t as_tiles_across(uint32_t extent) { return (extent + kAsTile - 1) / kAsTile; }

// One decision step over the `num_tiles` tiles of `tiles_in` (ids ty * ceil(W / 8) + tx, distinct and in range: the caller checks).
struct AdaptiveArgs {
  uint32_t width, height;
  const float4* rgba;      // the layer I at level n_now (W x H sums)
  float4* snapshot;        // A: the layer at level n_prev on entry, I on return (the tiles of tiles_in only)
  float n_prev, n_delta, n_now;  // (float)n_prev, (float)(n_now - n_prev), (float)n_now
  double threshold;        // a tile stops when E <= threshold
  const uint32_t* tiles_in;
  uint32_t num_tiles;
  float* tile_error;       // ceil(W / 8) x ceil(H / 8): entry `id` receives (float)E
  uint32_t* keep;          // num_tiles: the tile's pixel count when it stays active, else 0
  uint32_t* tile_off;      // num_tiles: kept tiles before this one
  uint32_t* pix_off;       // num_tiles: pixels of the kept tiles before this one
  uint32_t* totals;        // [0] kept tiles, [1] their pixels
  uint32_t* tiles_out;     // the kept tiles, in the order they had in tiles_in
  uint32_t* pixels_out;    // their pixels (y * W + x): tile after tile, row-major inside a tile
};
// k_as_error, k_as_scan, k_as_scatter on `s`, in this order; nothing returns to the host in between
void launch_adaptive_step(hipStream_t s, const AdaptiveArgs& a);

}  // namespace pb
