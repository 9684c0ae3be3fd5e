// The soundness of the per-light shaft grid (pbrlab_amd/csrc/shaft_grid.h), on the CPU with the code the device runs.
//
// A scene is a set of triangles and a set of light boxes; a light box is the box of some of the triangles (an emissive mesh) or, once per
// scene, a box in free air that holds no geometry -- the only way a list can be EMPTY, since a light's own triangles always lie in its
// shaft.  The tree is built as a commit builds it (build_bvh with the turn cost and the passes, build_qlayout: QNodes and TriPair records),
// the grid by shaft_build_cell, the function the device's build kernel calls per cell.  Then seeded rays: an origin -- uniform in a cell,
// or exactly on its faces, edges and corners --, the cell shaft_cell_of finds for it (what the shading kernel does), and if that cell is
// CLEAR, targets in the light's box, among them the point straight above or below the origin (a direction with two zero components: 1 / d
// infinite).  Each ray is the renderer's shadow ray: d = (q - o) / |q - o| in float, [1e-3, max(1e-3, |q - o| - 1e-3)].  Required: the
// any-hit over ALL triangles with the contract's test (tri_test + hit_inside of dtrace.h, restated here operation for operation; this
// file is compiled with -ffp-contract=off) equals the any-hit over the triangles of the cell's listed leaves.
// Also: shaft_meets_box against a brute-force sampling of s, and shaft_cell_of at the grid's edges.
// Per scene at least 100 CLEAR cells with an empty list and 100 with a non-empty one must have been exercised.
//   shaft_grid_check --synthetic            the built-in scenes
//   shaft_grid_check triangles.bin R        a file: uint32 n, uint32 nb, 9 n floats, nb boxes of 6 floats (lo, hi)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_scene.h"
#include "shaft_grid.h"
using namespace pb;

static uint64_t rng_state;
static double rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((rng_state >> 11) & ((1ull << 53) - 1)) / 9007199254740992.0;
}

// ---- the contract's triangle test (dtrace.h::tri_test, hit_inside), float, operation for operation
static float vbox_lo(float v) { return fmaf(-fabsf(v), 7.62939453125e-06f, v) - 1e-31f; }
static float vbox_hi(float v) { return fmaf(fabsf(v), 7.62939453125e-06f, v) + 1e-31f; }
static bool hit_inside(const float lo[3], const float hi[3], const float o[3], const float inv[3], float t) {
  float a = 0.f, b = 0.f;
  for (int k = 0; k < 3; k++) {
    const float t0 = (vbox_lo(lo[k]) - o[k]) * inv[k], t1 = (vbox_hi(hi[k]) - o[k]) * inv[k];
    const float mn = fminf(t0, t1), mx = fmaxf(t0, t1);
    a = k ? fmaxf(a, mn) : mn, b = k ? fminf(b, mx) : mx;
  }
  const float e = 1.52587890625e-05f;
  a = fmaf(-fabsf(a), e, a), b = fmaf(fabsf(b), e, b);
  return a <= t && t <= b;
}
static void sub3(const float* a, const float* b, float* o) { o[0] = a[0] - b[0], o[1] = a[1] - b[1], o[2] = a[2] - b[2]; }
static void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
static float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static bool tri_test(const float* tri, const float o[3], const float d[3], const float inv3[3], float tmin, float* t) {
  const float *v0 = tri, *v1 = tri + 3, *v2 = tri + 6;
  float e1[3], e2[3], p[3], s[3], q[3];
  sub3(v1, v0, e1), sub3(v2, v0, e2);
  cross3(d, e2, p);
  const float det = dot3(e1, p);
  if (!(det != 0.0f)) return false;
  const float inv = 1.0f / det;
  sub3(o, v0, s);
  const float uu = dot3(s, p) * inv;
  if (!(uu >= 0.0f && uu <= 1.0f)) return false;
  cross3(s, e1, q);
  const float vv = dot3(d, q) * inv;
  if (!(vv >= 0.0f && uu + vv <= 1.0f)) return false;
  const float tt = dot3(e2, q) * inv;
  if (!(tt > tmin)) return false;
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) lo[a] = fminf(fminf(v0[a], v1[a]), v2[a]), hi[a] = fmaxf(fmaxf(v0[a], v1[a]), v2[a]);
  if (!hit_inside(lo, hi, o, inv3, tt)) return false;
  *t = tt;
  return true;
}

struct Scene {
  std::string name;
  std::vector<float> tri;     // 9 per triangle
  std::vector<float> lights;  // 6 per light box
  uint32_t res = 16;
  uint32_t rays_per_cell = 6;
};
static void add_tri(Scene& s, const float a[3], const float b[3], const float c[3]) {
  s.tri.insert(s.tri.end(), a, a + 3), s.tri.insert(s.tri.end(), b, b + 3), s.tri.insert(s.tri.end(), c, c + 3);
}
// an axis-aligned rectangle: `axis` fixed at `at`, the other two over [u0, u1] x [v0, v1]
static void add_quad(Scene& s, int axis, float at, float u0, float u1, float v0, float v1) {
  const int ua = (axis + 1) % 3, va = (axis + 2) % 3;
  float p[4][3];
  const float us[4] = {u0, u1, u1, u0}, vs[4] = {v0, v0, v1, v1};
  for (int i = 0; i < 4; i++) p[i][axis] = at, p[i][ua] = us[i], p[i][va] = vs[i];
  add_tri(s, p[0], p[1], p[2]), add_tri(s, p[0], p[2], p[3]);
}
static void add_box(Scene& s, const float lo[3], const float hi[3]) {
  for (int a = 0; a < 3; a++) {
    const int ua = (a + 1) % 3, va = (a + 2) % 3;
    add_quad(s, a, lo[a], lo[ua], hi[ua], lo[va], hi[va]), add_quad(s, a, hi[a], lo[ua], hi[ua], lo[va], hi[va]);
  }
}
static void add_light_box_of(Scene& s, size_t first_tri, size_t ntri) {
  float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 9 * first_tri; i < 9 * (first_tri + ntri); i++) b[i % 3] = std::min(b[i % 3], s.tri[i]), b[3 + i % 3] = std::max(b[3 + i % 3], s.tri[i]);
  s.lights.insert(s.lights.end(), b, b + 6);
}
// the room every built-in scene starts from: the unit cube's floor, ceiling, back and side walls (open towards +z), a light of 0.3 x 0.3
// just below the ceiling (or IN the ceiling's plane: a light coplanar with a wall), and the box in free air
static Scene room(const char* name, bool coplanar_light = false) {
  Scene s;
  s.name = name;
  add_quad(s, 1, 0.0f, 0.f, 1.f, 0.f, 1.f), add_quad(s, 1, 1.0f, 0.f, 1.f, 0.f, 1.f);
  add_quad(s, 0, 0.0f, 0.f, 1.f, 0.f, 1.f), add_quad(s, 0, 1.0f, 0.f, 1.f, 0.f, 1.f);
  add_quad(s, 2, 0.0f, 0.f, 1.f, 0.f, 1.f);
  const size_t first = s.tri.size() / 9;
  add_quad(s, 1, coplanar_light ? 1.0f : 0.98f, 0.35f, 0.65f, 0.35f, 0.65f);  // (axis 1: u = z, v = x)
  add_light_box_of(s, first, 2);
  const float air[6] = {0.15f, 0.55f, 0.70f, 0.25f, 0.60f, 0.80f};
  s.lights.insert(s.lights.end(), air, air + 6);
  return s;
}

struct Tally {
  uint64_t cells_empty = 0, cells_listed = 0, rays = 0, occluded = 0, unknown = 0;
};

static bool check_scene(const Scene& s, Tally* tally) {
  const uint32_t n = (uint32_t)(s.tri.size() / 9), nl = (uint32_t)(s.lights.size() / 6), R = s.res;
  if (!n || !nl || nl > kShaftMaxLights) return printf("FAIL %s: %u triangles, %u lights\n", s.name.c_str(), n, nl), false;
  std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
  std::vector<uint8_t> kinds(n, 0);
  float bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t g = 0; g < n; g++)
    for (int a = 0; a < 3; a++) {
      const float* t = &s.tri[9 * (size_t)g];
      lo[3 * g + a] = std::min(t[a], std::min(t[3 + a], t[6 + a])), hi[3 * g + a] = std::max(t[a], std::max(t[3 + a], t[6 + a]));
      bmin[a] = std::min(bmin[a], lo[3 * g + a]), bmax[a] = std::max(bmax[a], hi[3 * g + a]);
    }
  BvhBuildOptions opt;
  opt.reinsert_passes = kReinsertPasses, opt.cost = kBvhCostTurns;
  FlatBvh bvh;
  build_bvh(lo, hi, kinds, &bvh, opt);
  const uint32_t ns = (uint32_t)bvh.slot_gid.size();
  std::vector<float4> slots(4 * (size_t)ns, make_float4(0.f, 0.f, 0.f, 0.f));
  for (uint32_t k = 0; k < ns; k++) {
    const float* t = &s.tri[9 * (size_t)bvh.slot_gid[k]];
    for (int c = 0; c < 3; c++) slots[4 * (size_t)k + c] = make_float4(t[3 * c], t[3 * c + 1], t[3 * c + 2], 0.f);
  }
  QLayout q;
  build_qlayout(bvh, slots, kinds, &q, opt);
  if (q.nodes.empty()) return printf("FAIL %s: no Q tree\n", s.name.c_str()), false;
  // a listed leaf index -> its triangles, read from the TriPair words themselves
  auto leaf_tris = [&](uint32_t first, float out[2][9]) {
    const float4* g = q.tri.data() + (size_t)first * kTriPairWords;
    const float w[20] = {g[0].x, g[0].y, g[0].z, g[0].w, g[1].x, g[1].y, g[1].z, g[1].w, g[2].x, g[2].y, g[2].z, g[2].w, g[3].x, g[3].y, g[3].z, g[3].w, g[4].x, g[4].y, g[4].z, g[4].w};
    for (int h = 0; h < 2; h++)
      for (int c = 0; c < 9; c++) out[h][c] = w[2 * c + h];
  };
  ShaftBuild b;
  b.tree.nodes = q.nodes.data(), b.tree.tri = q.tri.data(), b.tree.num_nodes = (uint32_t)q.nodes.size();
  b.frame = shaft_frame(bmin, bmax, R), b.margin = shaft_margin(bmin, bmax);
  b.num_lights = nl, b.max_list = kShaftMaxList;
  for (uint32_t l = 0; l < nl; l++)
    for (int a = 0; a < 3; a++) b.light_lo[l][a] = s.lights[6 * l + a], b.light_hi[l][a] = s.lights[6 * l + 3 + a];
  const uint32_t n3 = R * R * R;
  std::vector<uint32_t> cells((size_t)n3 * nl * kShaftCellWords);
  for (uint32_t l = 0; l < nl; l++)
    for (uint32_t c = 0; c < n3; c++) shaft_build_cell(b, l, c, &cells[((size_t)l * n3 + c) * kShaftCellWords]);
  // every leaf a list names must exist
  for (size_t c = 0; c < cells.size(); c += kShaftCellWords)
    if (cells[c] != kShaftUnknown) {
      if (cells[c] > kShaftMaxList) return printf("FAIL %s: a cell's count is %u\n", s.name.c_str(), cells[c]), false;
      for (uint32_t i = 0; i < cells[c]; i++)
        if ((size_t)(cells[c + 1 + i] + 1) * kTriPairWords > q.tri.size()) return printf("FAIL %s: a listed leaf is out of range\n", s.name.c_str()), false;
    }
  Tally t;
  rng_state = 977 + n;
  std::vector<uint8_t> seen((size_t)n3 * nl, 0);
  for (uint32_t l = 0; l < nl; l++)
    for (uint32_t c0 = 0; c0 < n3; c0++) {
      float clo[3], chi[3];
      shaft_cell_box(b.frame, c0 % R, (c0 / R) % R, c0 / (R * R), clo, chi);
      for (uint32_t r = 0; r < s.rays_per_cell; r++) {
        // the origin: uniform in the cell; every third one snapped onto the cell's faces (one, two or three coordinates: face, edge, corner)
        float o[3];
        for (int a = 0; a < 3; a++) o[a] = clo[a] + (float)rnd() * (chi[a] - clo[a]);
        if (r % 3 == 2)
          for (int a = 0; a < 3; a++)
            if (rnd() < 0.6) o[a] = rnd() < 0.5 ? clo[a] : chi[a];
        uint32_t cell;
        if (!shaft_cell_of(o[0], o[1], o[2], b.frame.org, b.frame.inv, R, &cell)) continue;  // (outside: the kernel traces)
        const uint32_t* rec = &cells[((size_t)l * n3 + cell) * kShaftCellWords];
        if (rec[0] == kShaftUnknown) {
          t.unknown++;
          continue;
        }
        // the target: uniform in the light's box; every fourth one straight above / below the origin where the box allows it
        float qp[3];
        for (int a = 0; a < 3; a++) qp[a] = b.light_lo[l][a] + (float)rnd() * (b.light_hi[l][a] - b.light_lo[l][a]);
        if (r % 4 == 1) {
          int keep = 1;  // the axis the ray runs along: the one in which the origin is farthest outside the box
          float far = -1.f;
          for (int a = 0; a < 3; a++) {
            const float dist = std::max(b.light_lo[l][a] - o[a], o[a] - b.light_hi[l][a]);
            if (dist > far) far = dist, keep = a;
          }
          bool inside = true;
          for (int a = 0; a < 3; a++)
            if (a != keep) inside = inside && o[a] >= b.light_lo[l][a] && o[a] <= b.light_hi[l][a];
          if (inside)
            for (int a = 0; a < 3; a++)
              if (a != keep) qp[a] = o[a];
        }
        float d[3], inv[3];
        sub3(qp, o, d);
        const float dist = sqrtf(dot3(d, d));
        if (!(dist > 0.f)) continue;
        for (int a = 0; a < 3; a++) d[a] = d[a] / dist, inv[a] = 1.0f / d[a];
        const float tmin = 1e-3f, tmax = std::max(1e-3f, dist - 1e-3f);
        bool any_all = false, any_list = false;
        float tt;
        for (uint32_t g = 0; g < n && !any_all; g++) any_all = tri_test(&s.tri[9 * (size_t)g], o, d, inv, tmin, &tt) && tt <= tmax;
        for (uint32_t i = 0; i < rec[0] && !any_list; i++) {
          float two[2][9];
          leaf_tris(rec[1 + i], two);
          for (int h = 0; h < 2; h++) any_list = any_list || (tri_test(two[h], o, d, inv, tmin, &tt) && tt <= tmax);
        }
        t.rays++, t.occluded += any_all;
        if (any_all != any_list)
          return printf("FAIL %s: light %u cell %u (list of %u): all triangles say %d, the list says %d; o %.9g %.9g %.9g q %.9g %.9g %.9g\n", s.name.c_str(), l, cell, rec[0],
                        (int)any_all, (int)any_list, o[0], o[1], o[2], qp[0], qp[1], qp[2]),
                 false;
        uint8_t& sn = seen[(size_t)l * n3 + cell];
        if (!sn) sn = 1, (rec[0] ? t.cells_listed : t.cells_empty)++;
      }
    }
  printf("scene %s triangles %u lights %u res %u clear_empty %llu clear_listed %llu rays %llu occluded %llu unknown_rays %llu\n", s.name.c_str(), n, nl, R,
         (unsigned long long)t.cells_empty, (unsigned long long)t.cells_listed, (unsigned long long)t.rays, (unsigned long long)t.occluded, (unsigned long long)t.unknown);
  if (t.cells_empty < 100 || t.cells_listed < 100) return printf("FAIL %s: too few CLEAR cells exercised\n", s.name.c_str()), false;
  *tally = t;
  return true;
}

// shaft_meets_box against the definition: the box meets (1 - s) C + s B for one of 4097 values of s.  The sampling can only miss a meeting
// (then the predicate says yes and the sampling no: allowed when the boxes come within 1e-3 of each other, counted); a sampled meeting
// the predicate denies is an error.
static bool check_predicate() {
  rng_state = 4242;
  uint32_t yes = 0, no = 0, near = 0;
  for (int it = 0; it < 20000; it++) {
    float c[2][3], b[2][3], p[2][3];
    const float along = (float)rnd();  // the box lies near the shaft's axis: about as many meetings as misses
    for (int a = 0; a < 3; a++) {
      const float c0 = (float)rnd(), b0 = (float)rnd(), p0 = c0 + along * (b0 - c0) + 0.5f * ((float)rnd() - 0.5f);
      c[0][a] = c0, c[1][a] = c0 + 0.05f, b[0][a] = b0, b[1][a] = b0 + (it % 5 == 0 ? 0.f : 0.2f * (float)rnd());
      p[0][a] = p0, p[1][a] = p0 + (it % 7 == 0 ? 0.f : 0.3f * (float)rnd());
    }
    const bool pred = shaft_meets_box(c[0], c[1], b[0], b[1], p[0], p[1]);
    bool sampled = false;
    double closest = INFINITY;
    for (int k = 0; k <= 4096 && !sampled; k++) {
      const double s = k / 4096.0;
      double gap = 0.0;
      for (int a = 0; a < 3; a++) {
        const double lo = (1 - s) * c[0][a] + s * b[0][a], hi = (1 - s) * c[1][a] + s * b[1][a];
        gap = std::max(gap, std::max((double)p[0][a] - hi, lo - (double)p[1][a]));
      }
      sampled = gap <= 0.0, closest = std::min(closest, gap);
    }
    if (sampled && !pred) return printf("FAIL predicate: a sampled s meets the box, the predicate says no (case %d)\n", it), false;
    if (pred && !sampled && closest > 1e-3) return printf("FAIL predicate: yes, but no sampled s comes within 1e-3 (case %d: %.3g)\n", it, closest), false;
    yes += pred, no += !pred, near += pred && !sampled;
  }
  printf("predicate yes %u no %u yes_between_samples %u\n", yes, no, near);
  return yes > 2000 && no > 2000;
}

// shaft_cell_of at the grid's edges: the bounds' own corners and faces lie inside (the frame is widened), the frame's far faces and
// anything beyond, a NaN and an infinity outside; inside, the index is the cell whose box (shaft_cell_box) holds the point up to an ulp
static bool check_cell_index() {
  const float bmin[3] = {-1.5f, 0.0f, 2.0f}, bmax[3] = {2.5f, 1.0f, 2.75f};
  for (uint32_t R : {1u, 7u, 64u, 128u}) {
    const ShaftFrame f = shaft_frame(bmin, bmax, R);
    uint32_t cell = 0;
    for (int k = 0; k < 8; k++) {
      const float p[3] = {k & 1 ? bmax[0] : bmin[0], k & 2 ? bmax[1] : bmin[1], k & 4 ? bmax[2] : bmin[2]};
      if (!shaft_cell_of(p[0], p[1], p[2], f.org, f.inv, R, &cell) || cell >= R * R * R) return printf("FAIL cell index: a corner of the bounds is outside (R %u)\n", R), false;
    }
    const float nan = NAN, inf = INFINITY;
    const float far[3] = {f.org[0] + (float)R * f.cell[0] * 1.001f, f.org[1], f.org[2]};
    if (shaft_cell_of(nan, 0.5f, 2.1f, f.org, f.inv, R, &cell) || shaft_cell_of(0.f, inf, 2.1f, f.org, f.inv, R, &cell) || shaft_cell_of(0.f, 0.5f, -inf, f.org, f.inv, R, &cell) ||
        shaft_cell_of(far[0], 0.5f, 2.1f, f.org, f.inv, R, &cell) || shaft_cell_of(bmin[0] - 1.f, 0.5f, 2.1f, f.org, f.inv, R, &cell))
      return printf("FAIL cell index: a point outside the grid got a cell (R %u)\n", R), false;
    rng_state = 7 + R;
    const float tol = 4.0f * 1.1920929e-07f * 4.0f;  // a few ulps of the largest coordinate
    for (int it = 0; it < 20000; it++) {
      float p[3];
      for (int a = 0; a < 3; a++) p[a] = bmin[a] + (float)rnd() * (bmax[a] - bmin[a]);
      if (it % 3 == 0) {  // on a cell border
        float lo[3], hi[3];
        shaft_cell_box(f, (uint32_t)(rnd() * R), (uint32_t)(rnd() * R), (uint32_t)(rnd() * R), lo, hi);
        for (int a = 0; a < 3; a++)
          if (lo[a] >= bmin[a] && lo[a] <= bmax[a]) p[a] = lo[a];
      }
      if (!shaft_cell_of(p[0], p[1], p[2], f.org, f.inv, R, &cell)) return printf("FAIL cell index: a point inside the bounds is outside (R %u)\n", R), false;
      float lo[3], hi[3];
      shaft_cell_box(f, cell % R, (cell / R) % R, cell / (R * R), lo, hi);
      for (int a = 0; a < 3; a++)
        if (!(p[a] >= lo[a] - tol && p[a] <= hi[a] + tol)) return printf("FAIL cell index: the point is %.3g outside its cell (R %u)\n", std::max(lo[a] - p[a], p[a] - hi[a]), R), false;
    }
  }
  printf("cell index ok\n");
  return true;
}

static bool run_synthetic() {
  if (!check_predicate() || !check_cell_index()) return false;
  std::vector<Scene> scenes;
  {  // an occluder whose box only touches a shaft's boundary: its top corner lies exactly on the segment from a floor cell's corner to a
     // corner of the light's box, half way; a second one a hair outside the same shaft
    Scene s = room("touching_occluder");
    const ShaftFrame f = shaft_frame((const float[3]){0.f, 0.f, 0.f}, (const float[3]){1.f, 1.f, 1.f}, s.res);
    float clo[3], chi[3];
    shaft_cell_box(f, 2, 0, 3, clo, chi);
    float mid[3];
    for (int a = 0; a < 3; a++) mid[a] = 0.5f * (clo[a] + s.lights[a]);
    const float lo1[3] = {mid[0] - 0.2f, mid[1] - 0.1f, mid[2] - 0.2f};
    add_box(s, lo1, mid);
    const float hi2[3] = {mid[0] - 0.21f, mid[1] + 0.2f, mid[2] + 0.3f}, lo2[3] = {mid[0] - 0.3f, mid[1] - 0.3f, mid[2] - 0.1f};
    add_box(s, lo2, hi2);
    scenes.push_back(s);
  }
  {  // sliver triangles: long, thin, some degenerate, across the middle of the room
    Scene s = room("slivers");
    rng_state = 31;
    for (int i = 0; i < 60; i++) {
      float a[3], b[3], c[3];
      for (int k = 0; k < 3; k++) a[k] = 0.1f + 0.8f * (float)rnd(), b[k] = 0.1f + 0.8f * (float)rnd();
      a[1] = 0.2f + 0.3f * (float)rnd(), b[1] = 0.2f + 0.3f * (float)rnd();
      for (int k = 0; k < 3; k++) c[k] = 0.5f * (a[k] + b[k]) + (i % 4 == 0 ? 0.f : 1e-5f * (float)rnd());
      add_tri(s, a, b, c);
    }
    scenes.push_back(s);
  }
  {  // a light in the ceiling's own plane, and a pillar
    Scene s = room("coplanar_light", true);
    const float lo[3] = {0.7f, 0.0f, 0.2f}, hi[3] = {0.8f, 0.6f, 0.3f};
    add_box(s, lo, hi);
    scenes.push_back(s);
  }
  {  // two lights (and the box in the air): the second one low on the left wall, behind a screen
    Scene s = room("two_lights");
    const size_t first = s.tri.size() / 9;
    add_quad(s, 0, 0.02f, 0.2f, 0.4f, 0.3f, 0.5f);
    const float air[6] = {s.lights[6], s.lights[7], s.lights[8], s.lights[9], s.lights[10], s.lights[11]};
    s.lights.resize(6);
    add_light_box_of(s, first, 2);
    s.lights.insert(s.lights.end(), air, air + 6);
    const float lo[3] = {0.3f, 0.0f, 0.1f}, hi[3] = {0.32f, 0.5f, 0.6f};
    add_box(s, lo, hi);
    scenes.push_back(s);
  }
  {  // a light with a degenerate triangle (three collinear corners, and one of zero extent) beside its two ordinary ones
    Scene s = room("degenerate_light");
    const size_t first = s.tri.size() / 9 - 2;
    const float a[3] = {0.35f, 0.98f, 0.35f}, b[3] = {0.5f, 0.98f, 0.5f}, c[3] = {0.65f, 0.98f, 0.65f};
    add_tri(s, a, b, c), add_tri(s, b, b, b);
    const float air[6] = {s.lights[6], s.lights[7], s.lights[8], s.lights[9], s.lights[10], s.lights[11]};
    s.lights.clear();
    add_light_box_of(s, first, 4);
    s.lights.insert(s.lights.end(), air, air + 6);
    const float lo[3] = {0.4f, 0.0f, 0.4f}, hi[3] = {0.6f, 0.3f, 0.6f};
    add_box(s, lo, hi);
    scenes.push_back(s);
  }
  for (const Scene& s : scenes) {
    Tally t;
    if (!check_scene(s, &t)) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return printf("usage: shaft_grid_check --synthetic | triangles.bin resolution\n"), 2;
  if (strcmp(argv[1], "--synthetic") == 0) return run_synthetic() ? (printf("synthetic ok\n"), 0) : 1;
  Scene s;
  s.name = "file";
  s.res = argc > 2 ? (uint32_t)atoi(argv[2]) : 24u;
  s.rays_per_cell = argc > 3 ? (uint32_t)atoi(argv[3]) : 3u;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return printf("FAIL: cannot open %s\n", argv[1]), 1;
  uint32_t n = 0, nb = 0;
  bool ok = fread(&n, 4, 1, f) == 1 && fread(&nb, 4, 1, f) == 1 && n > 0 && n < (1u << 27) && nb > 0 && nb <= kShaftMaxLights && s.res >= 1 && s.res <= kShaftMaxRes;
  if (ok) s.tri.resize(9 * (size_t)n), s.lights.resize(6 * (size_t)nb);
  ok = ok && fread(s.tri.data(), 36, n, f) == n && fread(s.lights.data(), 24, nb, f) == nb;
  fclose(f);
  if (!ok) return printf("FAIL: %s is not a file of triangles and light boxes\n", argv[1]), 1;
  Tally t;
  return check_scene(s, &t) ? (printf("file ok\n"), 0) : 1;
}
