// shaft_grid.h -- the per-light shaft grid: which shadow rays need no traversal.
//
// A regular grid over the scene's bounds, one set of cells per area light.  Cell C of light l records the triangle leaves of the Q tree
// (TriPair records, dscene.h) that hold a triangle whose own box, widened by the margin m, meets the SHAFT conv(C+ u B+): C+ the cell's
// box, B+ the box of the light's primitives, both widened by m.  By the intersection contract (dtrace.h: a hit is accepted only inside
// the ray's interval through the primitive's own box) no other primitive can occlude a shadow ray that starts in C and ends on the
// light.  A cell with at most kShaftMaxList such leaves is CLEAR and lists them; the shading kernel tests exactly those leaves, with
// the traversal's own test on the traversal's own words, and a ray none of them accepts is unoccluded.  Every other cell is UNKNOWN
// and its rays are traced.
//
// Everything here is host + device: the production build runs it one thread per (light, cell) (kernels.hip::k_shaft_grid), the CPU checker
// (tests/cpp/shaft_grid_check.cc) runs the same functions.
#pragma once

#include "dscene.h"

namespace pb {

constexpr uint32_t kShaftMaxLights = 8;   // scenes with more lights (or none) get no grid
constexpr uint32_t kShaftMaxList = 7;     // leaves a CLEAR cell can list
constexpr uint32_t kShaftUnknown = 0xFFFFFFFFu;
constexpr uint32_t kShaftCellWords = 8;   // a cell: state / count, then kShaftMaxList leaf indices (32 bytes: two 16-byte loads)
constexpr uint32_t kShaftMaxRes = 128;    // cells per axis at most
constexpr int kShaftStack = kStackDepth + 4;

// The margin: 2^-10 of the largest extent, plus 2^-18 of the largest coordinate so that it stays above the coordinates' own rounding
// in a scene far from the origin.  What it has to cover is orders of magnitude smaller.
PB_HD float shaft_margin(const float bmin[3], const float bmax[3]) {
  float ext = 0.0f, mag = 0.0f;
  for (int a = 0; a < 3; a++) {
    ext = fmaxf(ext, bmax[a] - bmin[a]);
    mag = fmaxf(mag, fmaxf(fabsf(bmin[a]), fabsf(bmax[a])));
  }
  return ext * 0.0009765625f + mag * 3.814697265625e-06f;
}

// Where the grid lies: the scene's bounds widened by the margin (a point ON a wall of the scene's box falls into a border cell)
struct ShaftFrame {
  float org[3], inv[3], cell[3];  // cell index = floor((p - org) * inv); a cell's edge
  uint32_t n;
};
PB_HD ShaftFrame shaft_frame(const float bmin[3], const float bmax[3], uint32_t n) {
  ShaftFrame f;
  const float m = shaft_margin(bmin, bmax);
  f.n = n;
  for (int a = 0; a < 3; a++) {
    const float lo = bmin[a] - m, size = fmaxf((bmax[a] + m) - lo, 1e-30f);
    f.org[a] = lo, f.cell[a] = size / (float)n, f.inv[a] = (float)n / size;
  }
  return f;
}
// The cell of a point; false outside the grid or for a NaN.
PB_HD bool shaft_cell_of(float px, float py, float pz, const float org[3], const float inv[3], uint32_t n, uint32_t* cell) {
  const float fn = (float)n;
  const float fx = (px - org[0]) * inv[0], fy = (py - org[1]) * inv[1], fz = (pz - org[2]) * inv[2];
  if (!(fx >= 0.0f && fx < fn && fy >= 0.0f && fy < fn && fz >= 0.0f && fz < fn)) return false;
  *cell = ((uint32_t)fz * n + (uint32_t)fy) * n + (uint32_t)fx;
  return true;
}
PB_HD void shaft_cell_box(const ShaftFrame& f, uint32_t ix, uint32_t iy, uint32_t iz, float lo[3], float hi[3]) {
  const uint32_t i[3] = {ix, iy, iz};
  for (int a = 0; a < 3; a++) lo[a] = f.org[a] + (float)i[a] * f.cell[a], hi[a] = f.org[a] + (float)(i[a] + 1u) * f.cell[a];
}

// Does the box [plo, phi] meet conv([clo, chi] u [blo, bhi])?  It does exactly when it meets the interpolated box
// (1 - s) [clo, chi] + s [blo, bhi] for some s in [0, 1]: per axis  plo <= chi + s (bhi - chi)  and  phi >= clo + s (blo - clo), six
// inequalities linear in s, i.e. an interval of s.  In double: the rounding is far below the margin whatever the coordinates.
PB_HD bool shaft_meets_box(const float clo[3], const float chi[3], const float blo[3], const float bhi[3], const float plo[3], const float phi[3]) {
  double s0 = 0.0, s1 = 1.0;
  for (int a = 0; a < 3; a++) {
    // s * k >= b, twice
    const double k[2] = {(double)bhi[a] - (double)chi[a], (double)clo[a] - (double)blo[a]};
    const double b[2] = {(double)plo[a] - (double)chi[a], (double)clo[a] - (double)phi[a]};
    for (int j = 0; j < 2; j++) {
      if (k[j] > 0.0) {
        const double s = b[j] / k[j];
        s0 = s > s0 ? s : s0;
      } else if (k[j] < 0.0) {
        const double s = b[j] / k[j];
        s1 = s < s1 ? s : s1;
      } else if (b[j] > 0.0) {
        return false;
      }
    }
  }
  return s0 <= s1;
}

// The Q tree of a triangle-only scene as the query reads it: DScene::wide's nodes and its TriPair records
struct ShaftTree {
  const QNode* nodes;
  const float4* tri;
  uint32_t num_nodes;
};

// The query of one cell.  [clo, chi] and [blo, bhi]: the cell's and the light's box, each ALREADY widened by 2 m -- a box widened by m
// meets the shaft of the boxes widened by m exactly when the box itself meets the shaft of the boxes widened by 2 m (Minkowski sums of
// boxes), so the tree's boxes and the triangles' own boxes are tested as they are; a node's box contains the boxes below it, hence a
// subtree whose box misses the shaft holds nothing that meets it.  Returns the number of leaves listed (<= max_list <= kShaftMaxList),
// or kShaftUnknown: more than max_list, a curve leaf, or a tree this walk cannot hold.
PB_HD uint32_t shaft_cell_query(const ShaftTree& t, const float clo[3], const float chi[3], const float blo[3], const float bhi[3], uint32_t max_list,
                                uint32_t list[kShaftMaxList]) {
  if (t.num_nodes == 0) return 0u;
  uint32_t stack[kShaftStack];
  int sp = 0;
  uint32_t count = 0;
  stack[sp++] = 0u;
  while (sp > 0) {
    const uint32_t ref = stack[--sp];
    if (ref & kLeafBit) {
      if (ref & kCurveBit) return kShaftUnknown;
      const uint32_t first = (ref & 0x3FFFFFFFu) >> 3;
      const float4* g = t.tri + (size_t)first * kTriPairWords;
      const float4 w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3], w4 = g[4];
      bool meets = false;
      for (int h = 0; h < 2; h++) {  // (a leaf of one triangle stores it twice)
        const float x[3] = {h ? w0.y : w0.x, h ? w1.w : w1.z, h ? w3.y : w3.x};
        const float y[3] = {h ? w0.w : w0.z, h ? w2.y : w2.x, h ? w3.w : w3.z};
        const float z[3] = {h ? w1.y : w1.x, h ? w2.w : w2.z, h ? w4.y : w4.x};
        const float plo[3] = {fminf(fminf(x[0], x[1]), x[2]), fminf(fminf(y[0], y[1]), y[2]), fminf(fminf(z[0], z[1]), z[2])};
        const float phi[3] = {fmaxf(fmaxf(x[0], x[1]), x[2]), fmaxf(fmaxf(y[0], y[1]), y[2]), fmaxf(fmaxf(z[0], z[1]), z[2])};
        // (a corner that is not a number fails every comparison of the triangle test: such a triangle occludes nothing)
        meets = meets || shaft_meets_box(clo, chi, blo, bhi, plo, phi);
      }
      if (meets) {
        if (count >= max_list || count >= kShaftMaxList) return kShaftUnknown;
        list[count++] = first;
      }
      continue;
    }
    if (ref >= t.num_nodes || sp + 4 > kShaftStack) return kShaftUnknown;
    const QNode& nd = t.nodes[ref];
    const float sc[3] = {nd.sx, nd.sy, nd.sz};
    const uint32_t ql[3] = {nd.qlo_x, nd.qlo_y, nd.qlo_z}, qh[3] = {nd.qhi_x, nd.qhi_y, nd.qhi_z};
    for (int c = 0; c < 4; c++) {
      if (nd.c[c] == kEmptyChild) continue;
      float lo[3], hi[3];  // the child's box as the traversal rebuilds it (dtrace.h::box_test4q)
      for (int a = 0; a < 3; a++)
        lo[a] = fmaf((float)((ql[a] >> (8 * c)) & 255u), sc[a], nd.org[a]), hi[a] = fmaf((float)((qh[a] >> (8 * c)) & 255u), sc[a], nd.org[a]);
      if (shaft_meets_box(clo, chi, blo, bhi, lo, hi)) stack[sp++] = nd.c[c];
    }
  }
  return count;
}

// One cell of one light, start to end: its box, both boxes widened, the query, the record.
struct ShaftBuild {
  ShaftTree tree;
  ShaftFrame frame;
  float margin;
  uint32_t num_lights, max_list;
  float light_lo[kShaftMaxLights][3], light_hi[kShaftMaxLights][3];  // the box of each light's primitives
};
PB_HD void shaft_build_cell(const ShaftBuild& b, uint32_t light, uint32_t cell, uint32_t rec[kShaftCellWords]) {
  const uint32_t n = b.frame.n;
  const uint32_t ix = cell % n, iy = (cell / n) % n, iz = cell / (n * n);
  float clo[3], chi[3], blo[3], bhi[3];
  shaft_cell_box(b.frame, ix, iy, iz, clo, chi);
  const float w = 2.0f * b.margin;
  for (int a = 0; a < 3; a++) clo[a] -= w, chi[a] += w, blo[a] = b.light_lo[light][a] - w, bhi[a] = b.light_hi[light][a] + w;
  uint32_t list[kShaftMaxList];
  for (uint32_t i = 0; i < kShaftMaxList; i++) list[i] = 0u;
  rec[0] = shaft_cell_query(b.tree, clo, chi, blo, bhi, b.max_list, list);
  for (uint32_t i = 0; i < kShaftMaxList; i++) rec[1 + i] = rec[0] == kShaftUnknown ? 0u : list[i];
}

// kernels.hip: every cell of every light, on the device.  cells: num_lights x n^3 records of kShaftCellWords words.
hipError_t build_shaft_grid_gpu(hipStream_t st, const ShaftBuild& b, uint32_t* cells);

}  // namespace pb
