// knobs.h -- every PBRHIP_* environment variable the library reads: tuning knobs for A/B runs and debugging switches.
// read_knobs() (pbrhip.cpp) is the library's only reader of the environment.  Each public call that uses a knob reads the record once at
// its entry and passes it down; it is never cached across calls (a test may change a knob between two renders).
#pragma once

#include <stdint.h>
#include <optional>

#ifndef PB_QUAD_RAYS
#define PB_QUAD_RAYS 0u  // k_trace launches of at most this many rays run on k_trace_quad (PBRHIP_QUAD_RAYS overrides)
#endif

namespace pb {

struct Knobs {
  // scene commit
  int bvh = -1;                 // PBRHIP_BVH: -1 (unset) = the scene's builder; "gpu" = the LBVH built on the GPU, any other value = the host's SAH tree
  bool wide = true;             // PBRHIP_WIDE: a value that atoi reads as 0 (any non-number too) = no Q tree: none is built at commit, none is walked at render
  bool bvh_reinsert = true;     // PBRHIP_BVH_REINSERT (1): 0 = the host builder's tree as its top-down splits leave it, no subtree re-insertion (host_scene.h::BvhBuildOptions; triangle-only scenes, the others never get it)
  uint32_t bvh_reinsert_top = 20000;  // PBRHIP_BVH_REINSERT_TOP (kReinsertTop): the largest nodes by box area that a re-insertion pass takes out and puts back; 0 = none
  bool bvh_cost = true;         // PBRHIP_BVH_COST (1): 0 = the host builder and its Q collapse price a leaf per primitive and place re-insertion passes by area growth alone, as before the traversal's turns were priced (host_scene.h::BvhBuildOptions::cost; for A/Bs)
  bool sss_entry = true;        // PBRHIP_SSS_ENTRY (1): 0 = random walks start at the root, not at the cut of the Q tree around their instance
  uint32_t sss_foreign = 3;     // PBRHIP_SSS_FOREIGN (3): foreign references allowed in a walk's entry cut (at most kSssMaxForeign)
  uint32_t shadow_grid = 64;    // PBRHIP_SHADOW_GRID (64): cells per axis of the per-light shaft grid (shaft_grid.h; at most kShaftMaxRes); 0 = no grid, every shadow ray is traced
  uint32_t shadow_grid_list = 7;  // PBRHIP_SHADOW_GRID_LIST (7): triangle leaves a CLEAR cell may list (at most kShaftMaxList); for sweeps
  bool debug = false;           // PBRHIP_DEBUG: set = commit and render print sizes and free memory on stderr
  // path layout (ensure_pixels; part of its cache key)
  uint32_t pixel_tile = 8;      // PBRHIP_PIXEL_TILE (8): paths laid out in patches of this many pixels squared; 0 or 1 = rows
  bool patch_shuffle = true;    // PBRHIP_PATCH_SHUFFLE (1): 0 = the patches in image order instead of scattered
  // the group schedule (render_impl, ChunkRun)
  uint32_t pass_run = 0;        // PBRHIP_PASS_RUN: 0 (unset) = 64 for scenes with curves, else 1; R >= 1 = runs of up to R passes of a pixel
  const char* groups = nullptr; // PBRHIP_GROUPS: passes per path group, e.g. "56,8" (plan_groups parses it); unset = the default plan
  std::optional<uint32_t> tail_paths;  // PBRHIP_TAIL_PATHS: overrides pbrhip_render_desc.tail_paths: hand a group to k_tail at this many live paths, 0 = never
  std::optional<uint32_t> streams;     // PBRHIP_STREAMS: overrides pbrhip_render_desc.num_streams (that many equal groups; 0 = the default plan)
  uint32_t window = 8;          // PBRHIP_WINDOW (kMaxGroups; 1 when PBRHIP_GROUPS is set; at least 1): groups in their bulk phase at once
  uint32_t bulk_div = 0;        // PBRHIP_BULK_DIV (0): k = a group leaves its bulk phase below 1/k of its paths, not only at the hand-over to k_tail
  uint32_t pipe_depth = 2;      // PBRHIP_PIPE_DEPTH (2; 1 .. kRingSlots - 1): iterations of a group enqueued ahead of what the host has heard of
  uint32_t pipe_depth_small = 8;// PBRHIP_PIPE_DEPTH_SMALL (8; 1 .. kRingSlots - 1): the same below 256 Ki live paths
  double pipe_stop = 2.0;       // PBRHIP_PIPE_STOP (2.0, atof): nothing is enqueued ahead at or below this many times tail_paths live paths
  bool trace_sched = false;     // PBRHIP_TRACE_SCHED: set = one stderr line per iteration the host hears of
  const char* wave_log = nullptr;  // PBRHIP_WAVE_LOG: file for start / end / turns of every k_trace wave (with PBRHIP_RENDER_STATS; scripts/wave_log.py)
  bool pv_stats = false;        // PBRHIP_PV_STATS: set = the traversal statistics of a PBRHIP_RENDER_STATS render printed on stderr
  // what one iteration runs (ChunkRun::enqueue_iteration)
  uint32_t susp_turns = 24;     // PBRHIP_SUSP_TURNS (24): loop turns a k_trace wave drains an empty queue for before it suspends its rays; 0 = never
  uint32_t shadow_first = 1;    // PBRHIP_SHADOW_FIRST (1): k_trace takes the previous bounce's shadow rays before this bounce's closest-hit rays
  bool first_direct = true;     // PBRHIP_FIRST_DIRECT (1): 0 = a first bounce runs k_classify too
  bool direct = true;           // PBRHIP_DIRECT (1): 0 = every bounce of a scene without hair and media runs k_classify
  bool sss_walk = true;         // PBRHIP_SSS_WALK (1): 0 = one wavefront iteration per step of a random walk, no k_sss_walk
  bool wide_walk = true;        // PBRHIP_WIDE_WALK: a value that atoi reads as 0 = k_sss_walk walks the binary tree
  // launch shapes (kernels.hip)
  uint32_t rays_per_wave = 4;   // PBRHIP_RAYS_PER_WAVE (4): k_trace gets one wave per this many rays, up to the resident set
  uint32_t trace_blocks = 0;    // PBRHIP_TRACE_BLOCKS: k >= 1 = at most k resident blocks of k_trace per CU (never more than the kernel's); 0 = the kernel's
  bool small_caps = true;       // PBRHIP_TRACE_BLOCKS_SMALL unset: the built-in block caps of small k_trace launches (Q tree, no curves) apply
  uint32_t small_blocks = 0, small_rays = 0;  // PBRHIP_TRACE_BLOCKS_SMALL="k,n": k blocks per CU for launches of at most n rays instead ("0,0": none)
  uint32_t quad_rays = PB_QUAD_RAYS;  // PBRHIP_QUAD_RAYS (PB_QUAD_RAYS): k_trace launches of at most this many rays run one ray per quad of lanes
  // test hooks (pbrhip_trace_closest / _any)
  bool quad = false;            // PBRHIP_QUAD: a leading '1' = one ray per quad of lanes (Q tree, no curves)
  bool simple_traversal = false;// PBRHIP_SIMPLE_TRAVERSAL: set = the one-ray-per-lane traversal kernels
};

Knobs read_knobs();

}  // namespace pb
