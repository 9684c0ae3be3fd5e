// commit.cpp -- from the host model to the device scene: the staging helpers (light tables, primitive boxes, slots and
// ShadeRecs, materials), pbrhip_scene_commit, pbrhip_scene_refit with its two ways of staging (on the host, or -- device geometry mode,
// geom_gpu.h -- on the device), the host side of that mode and the device write of a material edit.  Host C++ only.
#include <math.h>
#include <string.h>

#include <chrono>
#include <limits>
#include <numeric>

#include "geom_math.h"
#include "scene_impl.h"

using namespace pb;

static_assert(sizeof(LightRec) == 80, "light record layout");

// ------------------------------------------------------------------ commit
static V3 mesh_vertex(const HostMesh& m, uint32_t prim, int k) {
  const float* p = m.vertices.data() + (size_t)m.vid[prim * 3 + k] * 4;
  return V3(p[0], p[1], p[2]);
}
static V3 world_vertex(const HostInstance& in, const HostMesh& m, uint32_t prim, int k) {
  const V3 v = mesh_vertex(m, prim, k);
  return in.identity ? v : xf_point(in.xf, v);
}
// control points xyzr of curve `prim` as the raytracer sees them (the radius is not scaled)
static void world_curve(const HostInstance& in, const HostMesh& m, uint32_t prim, float out[16]) {
  const float* cps = m.cverts.data() + (size_t)m.cidx[prim] * 4;
  for (int c = 0; c < 4; c++) {
    V3 v(cps[4 * c], cps[4 * c + 1], cps[4 * c + 2]);
    if (!in.identity) v = xf_point(in.xf, v);
    out[4 * c] = v.x, out[4 * c + 1] = v.y, out[4 * c + 2] = v.z, out[4 * c + 3] = cps[4 * c + 3];
  }
}
// TriangleMesh::FetchFaceArea (mesh/triangle-mesh.cc:113-124)
static float face_area(const HostMesh& m, uint32_t prim) {
  V3 p0 = mesh_vertex(m, prim, 0), p1 = mesh_vertex(m, prim, 1), p2 = mesh_vertex(m, prim, 2);
  return length(cross(p1 - p0, p2 - p0)) * 0.5f;
}

// LightManager::RegisterInstanceMesh (light-manager.cc:79-184)
static void register_lights(pbrhip_scene* s, uint32_t instance_id) {
  HostInstance& in = s->instances[instance_id];
  size_t ng = in.light_ids.size();
  in.has_area_light.assign(ng, 0);
  in.area_lights.assign(ng, HostAreaLight());
  for (size_t g = 0; g < ng; g++) {
    const std::vector<uint32_t>& ids = in.light_ids[g];
    if (ids.empty()) continue;
    const HostMesh& m = *inst_mesh(s, instance_id, (uint32_t)g);
    if (m.kind != 0) continue;
    uint32_t nf = m.nfaces;
    bool have = false;
    for (uint32_t f = 0; f < nf; f++) have = have || ids[f] != kNone;
    if (!have) continue;
    HostAreaLight& a = in.area_lights[g];
    in.has_area_light[g] = 1;
    a.light_param_ids = ids;
    a.choose_prob.assign(nf, 0.f);
    for (uint32_t f = 0; f < nf; f++) {
      float intensity = 0.0f;
      if (ids[f] != kNone) intensity = spectrum_norm(s->light_params[ids[f]]);
      a.choose_prob[f] = intensity * face_area(m, f);
    }
    a.intensity_sum = std::accumulate(a.choose_prob.begin(), a.choose_prob.end(), 0.0f);
    const float sum = a.intensity_sum;
    for (float& v : a.choose_prob) v = v / sum;
    a.cdf = a.choose_prob;
    for (uint32_t f = 0; nf > 0 && f < nf - 1u; f++) a.cdf[f + 1u] += a.cdf[f];
    a.area_pdf.assign(nf, 0.f);
    for (uint32_t f = 0; f < nf; f++)
      if (ids[f] != kNone) a.area_pdf[f] = 1.0f / face_area(m, f);
  }
}
// LightManager::Commit (light-manager.cc:29-77)
static void commit_lights(pbrhip_scene* s) {
  s->lights.clear();
  double intensity_sum = 0.0;
  for (uint32_t i = 0; i < s->instances.size(); i++) {
    HostInstance& in = s->instances[i];
    for (uint32_t g = 0; g < in.area_lights.size(); g++) {
      if (!in.has_area_light[g]) continue;
      in.area_lights[g].global_id = (uint32_t)s->lights.size();
      HostLight L;
      L.choose_prob = in.area_lights[g].intensity_sum;
      L.instance_id = i, L.geom_id = g;
      intensity_sum += (double)L.choose_prob;
      s->lights.push_back(L);
    }
  }
  for (HostLight& L : s->lights) L.choose_prob = (float)((double)L.choose_prob / intensity_sum);
  s->light_cdf.resize(s->lights.size());
  for (size_t l = 0; l < s->lights.size(); l++) s->light_cdf[l] = s->lights[l].choose_prob;
  for (size_t l = 0; !s->light_cdf.empty() && l < s->light_cdf.size() - 1u; l++) s->light_cdf[l + 1u] += s->light_cdf[l];
}

static Material make_material(const HostMaterial& hm) {
  Material m;
  memset(&m, 0, sizeof(m));
  m.kind = hm.kind;
  m.bsdf = default_bsdf();
  if (hm.kind == kMatPrincipled) {
    m.bsdf = param_to_bsdf(hm.pr);
    m.param = hm.pr;
    medium_coefficients(m.bsdf, m.sss_sigt, m.sss_sigs, m.sss_wthr);  // (only read when the subsurface closure is picked)
    m.textured = (hm.pr.base_color_tex_id != kNone || hm.pr.subsurface_color_tex_id != kNone) ? 1u : 0u;
  } else {
    m.hair = hair_param_to_bsdf(hm.hr);
  }
  return m;
}

// Flattens the primitives in canonical (instance, geom, prim, sub) order: the index is the gid.  A gid thus names a UNIT -- a triangle,
// or one piece of a cubic --, and the pieces of one cubic have ascending gids: dknearest.h::knearest_offer orders equal distances by
// the gid alone and relies on both.  Whoever renumbers here gives that comparison its third key, sub, back.
static int flatten_prims(const pbrhip_scene* s, std::vector<PrimRef>* prims) {
  for (uint32_t i = 0; i < s->instances.size(); i++)
    for (uint32_t g = 0; g < s->instances[i].material_ids.size(); g++) {
      const HostMesh& m = *inst_mesh(s, i, g);
      if (s->instances[i].material_ids[g].size() != m.num_prims())
        return fail(PBRHIP_ESIZE, "material param error (instance %u geom %u)", i, g);
      for (uint32_t p = 0; p < m.num_prims(); p++)
        for (uint32_t sub = 0; sub < (m.kind == 1 ? 4u : 1u); sub++) prims->push_back({i, g, p, (uint32_t)m.kind, sub});
    }
  return PBRHIP_OK;
}

// Scene bounds (rtcGetSceneBounds, raytracer_impl.cc:199-202; they place the camera): the union of the instances'
// bounds.  An RTC_GEOMETRY_TYPE_INSTANCE (raytracer_impl.cc:61-81) reports the box of the transformed CORNERS of its local
// scene's box -- larger than the box of the transformed geometry under rotation or shear; an instance whose matrix is
// bit for bit the identity reports the local box.  Local box: triangles by their corners, curves by the hull of their
// control points widened by the largest control radius.  (The tree is built over the transformed primitives.)
// (the LOCAL box of instance i into ll / lh; false: it has no primitive)
static bool instance_local_box(const pbrhip_scene* s, uint32_t i, float ll[3], float lh[3]) {
  const float inf = std::numeric_limits<float>::infinity();
  const HostInstance& inst = s->instances[i];
  for (int k = 0; k < 3; k++) ll[k] = inf, lh[k] = -inf;
  bool any = false;
  for (uint32_t g = 0; g < inst.material_ids.size(); g++) {
    const HostMesh& m = *inst_mesh(s, i, g);
    for (uint32_t p = 0; p < m.num_prims(); p++) {
      any = true;
      if (m.kind == 0) {
        for (int c = 0; c < 3; c++) {
          const V3 v = mesh_vertex(m, p, c);
          const float a[3] = {v.x, v.y, v.z};
          for (int k = 0; k < 3; k++) ll[k] = fminf(ll[k], a[k]), lh[k] = fmaxf(lh[k], a[k]);
        }
      } else {
        float r = 0.f, cl[3] = {inf, inf, inf}, ch[3] = {-inf, -inf, -inf};
        for (int c = 0; c < 4; c++) {
          const float* cp = m.cverts.data() + ((size_t)m.cidx[p] + c) * 4;
          r = fmaxf(r, fabsf(cp[3]));
          for (int k = 0; k < 3; k++) cl[k] = fminf(cl[k], cp[k]), ch[k] = fmaxf(ch[k], cp[k]);
        }
        for (int k = 0; k < 3; k++) ll[k] = fminf(ll[k], cl[k] - r), lh[k] = fmaxf(lh[k], ch[k] + r);
      }
    }
  }
  return any;
}
// (what an instance with local box ll / lh adds to the scene's box)
static void unite_instance_box(const HostInstance& inst, const float ll[3], const float lh[3], float bmin[3], float bmax[3]) {
  if (inst.identity) {
    for (int k = 0; k < 3; k++) bmin[k] = fminf(bmin[k], ll[k]), bmax[k] = fmaxf(bmax[k], lh[k]);
  } else {
    for (int c = 0; c < 8; c++) {
      const V3 v = xf_point(inst.xf, V3((c & 1) ? lh[0] : ll[0], (c & 2) ? lh[1] : ll[1], (c & 4) ? lh[2] : ll[2]));
      const float a[3] = {v.x, v.y, v.z};
      for (int k = 0; k < 3; k++) bmin[k] = fminf(bmin[k], a[k]), bmax[k] = fmaxf(bmax[k], a[k]);
    }
  }
}
static void scene_bounds(pbrhip_scene* s) {
  const float inf = std::numeric_limits<float>::infinity();
  float bmin[3] = {inf, inf, inf}, bmax[3] = {-inf, -inf, -inf};
  for (uint32_t i = 0; i < s->instances.size(); i++) {
    float ll[3], lh[3];
    if (instance_local_box(s, i, ll, lh)) unite_instance_box(s->instances[i], ll, lh, bmin, bmax);
  }
  memcpy(s->bmin, bmin, sizeof(bmin));
  memcpy(s->bmax, bmax, sizeof(bmax));
}

// The tight box of a slot's first three words: a triangle's corners, or the two end points (xyz, radius) of a curve piece widened by
// the larger end radius (the ribbon between them never leaves that box, and a hit is reported at the depth of the axis point).
static void slot_tight_box(const float4* sl, bool curve, float lo[3], float hi[3]) {
  const float a[3] = {sl[0].x, sl[0].y, sl[0].z}, b[3] = {sl[1].x, sl[1].y, sl[1].z}, c[3] = {sl[2].x, sl[2].y, sl[2].z};
  const float r = std::max(fabsf(sl[0].w), fabsf(sl[1].w));
  for (int k = 0; k < 3; k++) {
    if (curve) lo[k] = std::min(a[k], b[k]) - r, hi[k] = std::max(a[k], b[k]) + r;
    else lo[k] = std::min(std::min(a[k], b[k]), c[k]), hi[k] = std::max(std::max(a[k], b[k]), c[k]);
  }
}
// The box (world space) and kind of every primitive: what the tree is built over, from the numbers its slot will hold.
static void prim_boxes(const pbrhip_scene* s, const std::vector<PrimRef>& prims, std::vector<float>* lo, std::vector<float>* hi,
                       std::vector<uint8_t>* kinds) {
  const uint32_t np = (uint32_t)prims.size();
  lo->assign(3 * (size_t)np, 0.f), hi->assign(3 * (size_t)np, 0.f), kinds->assign(np, 0);
  for (uint32_t g = 0; g < np; g++) {
    const PrimRef& pr = prims[g];
    const HostMesh& m = *inst_mesh(s, pr.instance_id, pr.geom_id);
    const HostInstance& inst = s->instances[pr.instance_id];
    float4 sl[3] = {};
    float cps[16], a[4], b[4];
    (*kinds)[g] = (uint8_t)pr.kind;
    if (pr.kind == 0) {
      for (int c = 0; c < 3; c++) {
        const V3 v = world_vertex(inst, m, pr.prim_id, c);
        sl[c] = make_float4(v.x, v.y, v.z, 0.f);
      }
    } else {
      world_curve(inst, m, pr.prim_id, cps);
      curve_piece(cps, pr.sub, a, b);
      sl[0] = make_float4(a[0], a[1], a[2], a[3]), sl[1] = make_float4(b[0], b[1], b[2], b[3]);
    }
    slot_tight_box(sl, pr.kind != 0, &(*lo)[3 * (size_t)g], &(*hi)[3 * (size_t)g]);
  }
}

// Light records: one per (light, prim), concatenated; heads[l] is light l's stretch of them.
static void light_records(const pbrhip_scene* s, std::vector<LightHead>* heads, std::vector<LightRec>* lrecs,
                          std::vector<float>* lprim_cdf) {
  heads->resize(s->lights.size());
  for (size_t l = 0; l < s->lights.size(); l++) {
    const HostLight& L = s->lights[l];
    const HostAreaLight& a = s->instances[L.instance_id].area_lights[L.geom_id];
    const HostMesh& m = *inst_mesh(s, L.instance_id, L.geom_id);
    (*heads)[l].first = (uint32_t)lrecs->size();
    (*heads)[l].count = m.nfaces;
    for (uint32_t f = 0; f < m.nfaces; f++) {
      LightRec r;
      memset(&r, 0, sizeof(r));
      V3 p0 = mesh_vertex(m, f, 0), p1 = mesh_vertex(m, f, 1), p2 = mesh_vertex(m, f, 2);
      V3 n = vnormalize(cross(p1 - p0, p2 - p1));  // CalcGeometryNormal (triangle-mesh.cc:181-184)
      r.p0[0] = p0.x, r.p0[1] = p0.y, r.p0[2] = p0.z;
      r.p1[0] = p1.x, r.p1[1] = p1.y, r.p1[2] = p1.z;
      r.p2[0] = p2.x, r.p2[1] = p2.y, r.p2[2] = p2.z;
      r.normal[0] = n.x, r.normal[1] = n.y, r.normal[2] = n.z;
      // light-manager.h:68-70,149-150: choose_light * choose_prim * prim_area_pdf, in that order
      r.pdf = L.choose_prob * a.choose_prob[f] * a.area_pdf[f];
      if (a.light_param_ids[f] != kNone) {
        V3 e = s->light_params[a.light_param_ids[f]];
        r.emission[0] = e.x, r.emission[1] = e.y, r.emission[2] = e.z;
      }
      lrecs->push_back(r);
      lprim_cdf->push_back(a.cdf[f]);
    }
  }
}

// One slot: the four 16-byte words `sl` and the ShadeRec `sr` of primitive `pr` with canonical id g (what pbrhip_scene_commit stages
// for every slot and pbrhip_scene_refit for the dirty ones).
static int slot_and_shade(const pbrhip_scene* s, const PrimRef& pr, uint32_t g, const std::vector<LightHead>& heads, float4* sl, ShadeRec& sr) {
  const HostInstance& in = s->instances[pr.instance_id];
  const HostMesh& m = *inst_mesh(s, pr.instance_id, pr.geom_id);
  uint32_t mat = in.material_ids[pr.geom_id][pr.prim_id];
  if (mat != kNone && (mat >= s->materials.size() || mat >= 0x00FFFFFFu)) return fail(PBRHIP_EINVAL, "material id %u out of range", mat);
  memset(&sr, 0, sizeof(sr));
  uint32_t flags = 0, lightrec = kNone;
  if (mat == kNone) flags |= kSlotMatNone;
  else if (s->materials[mat].kind == kMatHair) flags |= kSlotMatHair;
  for (int c = 0; c < 4; c++) sl[c] = make_float4(0, 0, 0, 0);
  if (pr.kind == 0) {
    for (int c = 0; c < 3; c++) {
      // traversal: what Embree sees (the transformed triangle); shading: the mesh's own corners -- the geometric normal
      // Embree reports for an instance is in the instance's local space and pbrlab uses it as it is
      const V3 w = world_vertex(in, m, pr.prim_id, c);
      sl[c] = make_float4(w.x, w.y, w.z, 0.f);
    }
    {
      // the two normals every hit on this triangle would otherwise compute from its corners (ShadeRec, dscene.h): the kernels'
      // own functions, evaluated here
      const V3 v0 = mesh_vertex(m, pr.prim_id, 0), v1 = mesh_vertex(m, pr.prim_id, 1), v2 = mesh_vertex(m, pr.prim_id, 2);
      const V3 ng = normalize_raw(cross(v1 - v0, v2 - v0));
      const V3 nf = vnormalize(cross(v1 - v0, v2 - v1));  // CalcGeometryNormal, triangle-mesh.cc:181-184
      sr.ng[0] = ng.x, sr.ng[1] = ng.y, sr.ng[2] = ng.z;
      sr.ns_flat[0] = nf.x, sr.ns_flat[1] = nf.y, sr.ns_flat[2] = nf.z;
    }
    uint32_t a = m.nid[pr.prim_id * 3 + 0], b = m.nid[pr.prim_id * 3 + 1], c = m.nid[pr.prim_id * 3 + 2];
    if (a != kNone && b != kNone && c != kNone) {  // triangle-mesh.cc:81-84
      flags |= kSlotHasNormals;
      const uint32_t idx[3] = {a, b, c};
      for (int q = 0; q < 3; q++) {
        const float* n = m.normals.data() + (size_t)idx[q] * 4;
        sr.n[3 * q + 0] = n[0], sr.n[3 * q + 1] = n[1], sr.n[3 * q + 2] = n[2];
      }
    }
    if (in.has_area_light[pr.geom_id]) {
      const HostAreaLight& al = in.area_lights[pr.geom_id];
      if (al.light_param_ids[pr.prim_id] != kNone) lightrec = heads[al.global_id].first + pr.prim_id;
    }
    uint32_t ta = m.tid[pr.prim_id * 3 + 0], tb = m.tid[pr.prim_id * 3 + 1], tc = m.tid[pr.prim_id * 3 + 2];
    if (ta != kNone && tb != kNone && tc != kNone) {  // triangle-mesh.cc:130-133
      flags |= kSlotHasUV;
      const uint32_t idx[3] = {ta, tb, tc};
      for (int q = 0; q < 3; q++) {
        sr.uv[2 * q + 0] = m.texcoords[(size_t)idx[q] * 2 + 0];
        sr.uv[2 * q + 1] = m.texcoords[(size_t)idx[q] * 2 + 1];
      }
    }
  } else {
    flags |= kSlotIsCurve;
    const float* cps = m.cverts.data() + (size_t)m.cidx[pr.prim_id] * 4;  // local: the tangent (= Ng) shading uses
    float wcps[16];
    world_curve(in, m, pr.prim_id, wcps);
    float a[4], b[4];
    curve_piece(wcps, pr.sub, a, b);
    sl[0] = make_float4(a[0], a[1], a[2], a[3]);
    sl[1] = make_float4(b[0], b[1], b[2], b[3]);
    sl[2] = make_float4(__builtin_bit_cast(float, pr.sub), 0.f, 0.f, 0.f);
    // shading needs the cubic itself (tangent = dP/du at the hit): control points xyzr in words 8..23 of the record
    float* w = reinterpret_cast<float*>(&sr);
    for (int c = 0; c < 16; c++) w[8 + c] = cps[c];
  }
  sr.gid = g, sr.lightrec = lightrec;
  sr.matflags = (mat == kNone ? 0x00FFFFFFu : mat) | (flags << 24);
  const uint32_t route = ((flags & kSlotMatHair) ? kHitHair : 0u) | ((flags & kSlotMatNone) ? kHitNoMaterial : 0u) |
                         (lightrec != kNone ? kHitLight : 0u) |
                         ((flags & (kSlotHasNormals | kSlotHasUV | kSlotIsCurve)) ? kHitMore : 0u);
  sl[2].w = __builtin_bit_cast(float, route);  // travels with the hit record (Hit::slot)
  sr.instance_id = pr.instance_id, sr.geom_id = pr.geom_id, sr.prim_id = pr.prim_id;
  return PBRHIP_OK;
}
// One box per light over all primitives of its mesh, packed two per node (an odd last one is stored twice).
static std::vector<BvhNode> light_boxes(const std::vector<LightHead>& heads, const std::vector<LightRec>& lrecs) {
  std::vector<BvhNode> boxes((heads.size() + 1) / 2);
  for (size_t l = 0; l < heads.size(); l++) {
    float lo3[3] = {INFINITY, INFINITY, INFINITY}, hi3[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t f = heads[l].first; f < heads[l].first + heads[l].count; f++)
      for (const float* p : {lrecs[f].p0, lrecs[f].p1, lrecs[f].p2})
        for (int a = 0; a < 3; a++) lo3[a] = std::min(lo3[a], p[a]), hi3[a] = std::max(hi3[a], p[a]);
    BvhNode& nd = boxes[l / 2];
    if (l % 2 == 0) memset(&nd, 0, sizeof(nd)), nd.set_box(1, lo3, hi3);
    nd.set_box(int(l % 2), lo3, hi3);
  }
  return boxes;
}

// ------------------------------------------------------------------ the steps of commit and refit
static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// Every host array a step stages.  Most are handed to hipMemcpyAsync from pageable memory: commit and refit own one of these until
// their final hipStreamSynchronize, so that no staged array dies before the copy has read it.
struct CommitStage {
  std::vector<PrimRef> prims;  // canonical order: the index is the gid
  std::vector<float> lo, hi, lprim_cdf;  // (lo, hi, kinds: what the tree is built over)
  std::vector<uint8_t> kinds;
  FlatBvh bvh;  // (built on the GPU: no nodes here, they are on the device)
  BvhBuildOptions bvh_opt;  // what the host tree was built with: its collapse prices the same cost
  std::vector<float4> slots;
  std::vector<ShadeRec> shade;
  std::vector<Material> mats;
  QLayout q;  // built on the host: all of it; collapsed on the device, or refitted there: the nodes as they came back
  std::vector<LightRec> lrecs;
  std::vector<BvhNode> lboxes;
  std::vector<SssEntry> walk_entries;
};

static void stage_lights(pbrhip_scene* s, CommitStage* cs) {  // the light tables of the whole model: they are small
  for (uint32_t i = 0; i < s->instances.size(); i++) register_lights(s, i);
  commit_lights(s);
  light_records(s, &s->light_heads, &cs->lrecs, &cs->lprim_cdf);
  cs->lboxes = light_boxes(s->light_heads, cs->lrecs);
  s->num_lrecs = (uint32_t)cs->lrecs.size();
  s->light_box.assign(6 * s->light_heads.size(), 0.0f);  // (what the shaft grid is cut around: shaft_grid.h)
  for (size_t l = 0; l < s->light_heads.size(); l++) {
    float* b = &s->light_box[6 * l];
    for (int a = 0; a < 3; a++) b[a] = INFINITY, b[3 + a] = -INFINITY;
    for (uint32_t r = s->light_heads[l].first; r < s->light_heads[l].first + s->light_heads[l].count; r++)
      for (const float* p : {cs->lrecs[r].p0, cs->lrecs[r].p1, cs->lrecs[r].p2})
        for (int a = 0; a < 3; a++) b[a] = std::min(b[a], p[a]), b[3 + a] = std::max(b[3 + a], p[a]);
  }
  // light sampling works on the meshes' local positions (light-manager.h:128-136 "TODO transform"), the raytracer on the
  // transformed ones: the doomed-path pretest against the light primitives (kernels.hip::misses_all_lights) is only the
  // traversal's own test when the two coincide
  s->lights_transformed = std::any_of(s->lights.begin(), s->lights.end(), [&](const HostLight& L) { return !s->instances[L.instance_id].identity; });
}
static int upload_lights(pbrhip_scene* s, const CommitStage& cs) {
  HIPCHK(s->d_light_cdf.upload(s->light_cdf, s->stream));
  HIPCHK(s->d_heads.upload(s->light_heads, s->stream));
  HIPCHK(s->d_lprim_cdf.upload(cs.lprim_cdf, s->stream));
  HIPCHK(s->d_lrecs.upload(cs.lrecs, s->stream));
  HIPCHK(s->d_light_boxes.upload(cs.lboxes, s->stream));
  return PBRHIP_OK;
}

static int build_binary_tree(pbrhip_scene* s, const Knobs& k, int builder, CommitStage* cs) {  // on the GPU into the scene's nodes, or on the host and uploaded
  FlatBvh& bvh = cs->bvh;
  const uint32_t np = (uint32_t)cs->prims.size();
  s->bvh_built_on_gpu = false;
  if ((builder == PBRHIP_BVH_GPU_LBVH || builder == PBRHIP_BVH_GPU_LBVH_WIDE) && np > 0) {
    HIPCHK(s->tree.reserve_nodes(TreeBufs::lbvh_nodes(np), np));  // (one slot per primitive)
    HIPCHK(build_bvh_gpu(s->stream, cs->lo, cs->hi, cs->kinds, s->tree.d_nodes.p, &bvh.slot_gid, &bvh.depth));
    s->bvh_built_on_gpu = bvh.depth <= (uint32_t)kStackDepth;
    if (!s->bvh_built_on_gpu) {
      // a Morton-order tree over badly distributed primitives can be deeper than the traversal stack: use the SAH tree
      fprintf(stderr, "pbrhip: GPU-built BVH is %u deep (stack %d): building on the host instead\n", bvh.depth, kStackDepth);
      bvh = FlatBvh();
    }
  }
  if (!s->bvh_built_on_gpu) {
    BvhBuildOptions& opt = cs->bvh_opt;
    opt.reinsert_passes = k.bvh_reinsert ? kReinsertPasses : 0u, opt.reinsert_top = k.bvh_reinsert_top;
    opt.for_qtree = k.wide;  // (no Q tree at this commit: the binary tree is what the rays walk)
    opt.cost = k.bvh_cost ? kBvhCostTurns : kBvhCostPrims;
    build_bvh(cs->lo, cs->hi, cs->kinds, &bvh, opt);
    if (k.debug)
      fprintf(stderr, "pbrhip: commit: host BVH: top-down build %.2f ms; re-insertion %.2f ms: %u passes kept, %u subtrees moved, %s %.6g -> %.6g\n", bvh.build_ms,
              bvh.reinsert_ms, bvh.reinsert_passes, bvh.reinsert_moves, k.wide ? "collapse cost" : "inner area", bvh.reinsert_cost0, bvh.reinsert_cost);
  }
  if (bvh.depth > (uint32_t)kStackDepth)
    return fail(PBRHIP_EOVERFLOW, "BVH depth %u exceeds the traversal stack (%d)", bvh.depth, kStackDepth);
  s->bvh_depth = bvh.depth;
  if (!s->bvh_built_on_gpu) {
    HIPCHK(s->tree.reserve_nodes((uint32_t)bvh.nodes.size(), (uint32_t)bvh.slot_gid.size()));
    if (!bvh.nodes.empty()) HIPCHK(hipMemcpyAsync(s->tree.d_nodes.p, bvh.nodes.data(), bvh.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice, s->stream));
  }
  return PBRHIP_OK;
}

static int stage_slots_and_materials(pbrhip_scene* s, CommitStage* cs) {
  const uint32_t ns = (uint32_t)cs->bvh.slot_gid.size();
  if (ns > kHitSlotMask) return fail(PBRHIP_EINVAL, "%u traversal primitives: at most %u are supported", ns, kHitSlotMask);
  // leaf-ordered slots (traversal geometry, 64 B each) + one 128-byte ShadeRec per slot (everything shading needs)
  cs->slots.resize(4 * (size_t)ns), cs->shade.resize(ns);
  for (uint32_t k = 0; k < ns; k++)
    if (int rc = slot_and_shade(s, cs->prims[cs->bvh.slot_gid[k]], cs->bvh.slot_gid[k], s->light_heads, &cs->slots[4 * (size_t)k], cs->shade[k])) return rc;
  std::vector<Material>& mats = cs->mats;
  mats.resize(s->materials.size());
  s->has_hair = s->has_sss = s->has_textured = false;
  for (size_t i = 0; i < mats.size(); i++) {
    const HostMaterial& hm = s->materials[i];
    if (hm.kind == kMatPrincipled)
      for (uint32_t t : {hm.pr.base_color_tex_id, hm.pr.subsurface_color_tex_id})
        if (t != kNone && t >= s->tex_descs.size()) return fail(PBRHIP_EINVAL, "material %zu: texture id %u out of range", i, t);
    mats[i] = make_material(s->materials[i]);
    if (mats[i].textured) s->has_sss = s->has_textured = true;  // a subsurface_color / base_color map can switch the SSS closure on per hit
    s->has_hair = s->has_hair || mats[i].kind == kMatHair;
    s->has_sss = s->has_sss || (mats[i].kind == kMatPrincipled && mats[i].bsdf.enable_subsurface);
  }
  return PBRHIP_OK;
}

// The Q tree of the traversal kernels (dscene.h::QNode; PBRHIP_WIDE=0 at commit: none).  A host-built tree is collapsed on the host
// (bvh_build.cpp::build_qlayout) and uploaded.  PBRHIP_BVH_GPU_LBVH_WIDE: the GPU-built tree is collapsed on the device (qtree_gpu.hip)
// straight into the scene's buffers, and the nodes come back for the stack need and the walk entries.  A tree that cannot be kept is dropped.
static int build_wide_tree(pbrhip_scene* s, const Knobs& k, int builder, CommitStage* cs) {
  TreeBufs& t = s->tree;
  QLayout& q = cs->q;
  s->wide_built_on_gpu = false;
  if (!s->bvh_built_on_gpu && t.num_nodes && k.wide) {
    build_qlayout(cs->bvh, cs->slots, cs->kinds, &q, cs->bvh_opt);
    if (k.debug) fprintf(stderr, "pbrhip: commit: curve leaves of the Q tree (counted over the collapse's visits): %zu of one piece, %zu of two pieces\n", q.leaves_one, q.leaves_pair);
  }
  if (s->bvh_built_on_gpu && builder == PBRHIP_BVH_GPU_LBVH_WIDE && k.wide) {
    const bool tri_pairs = all_triangles(cs->kinds);
    QCollapse qc;
    HIPCHK(hipStreamSynchronize(s->stream));  // (the slots are on the device: what follows is the collapse's own time)
    const auto t_start = std::chrono::steady_clock::now();
    HIPCHK(collapse_qtree_gpu(s->stream, t.d_nodes.p, t.num_slots, t.slots(), tri_pairs, [&](auto... a) { return t.alloc_wide(a...); }, &qc));
    const double ms_collapse = ms_since(t_start);
    const char* why = !qc.fits ? "a record index overflows its reference" : (!qc.quantised ? "a node cannot be quantised" : nullptr);
    if (!why) {
      q.nodes.resize(qc.nodes);
      HIPCHK(hipMemcpyAsync(q.nodes.data(), t.d_wide.p, (size_t)qc.nodes * sizeof(QNode), hipMemcpyDeviceToHost, s->stream));
      HIPCHK(hipStreamSynchronize(s->stream));
      q.stack_need = qtree_stack_need(q.nodes);
      if (q.stack_need > (uint32_t)kStackDepth) why = "its traversal needs more than the stack";
    }
    if (k.debug)
      fprintf(stderr, "pbrhip: commit: Q tree on the device: %u nodes in %u levels, collapse %.2f ms (of which allocation %.2f ms), download + stack need %.2f ms\n",
              qc.nodes, qc.levels, ms_collapse, qc.alloc_ms, ms_since(t_start) - ms_collapse);
    if (why) {
      fprintf(stderr, "pbrhip: the Q tree of the GPU-built BVH is dropped (%s): rendering the binary tree\n", why);
      q = QLayout();
    } else {
      s->wide_built_on_gpu = true;
      t.set_wide(qc.nodes, qc.tri_words, qc.pts);
    }
  }
  if (!s->wide_built_on_gpu) HIPCHK(t.upload(q.nodes.data(), (uint32_t)q.nodes.size(), q.tri.data(), q.tri.size(), q.pts.data(), q.hit.data(), q.pts.size(), s->stream));
  s->wide_stack_need = q.nodes.empty() ? 0u : q.stack_need;
  return PBRHIP_OK;
}

// (the bounds of an instance's primitive boxes: what the random walks' entries are cut around)
static void accumulate_instance_bounds(std::vector<float>& ilo, std::vector<float>& ihi, size_t inst, const float* lo, const float* hi) {
  for (size_t a = 0; a < 3; a++) ilo[3 * inst + a] = std::min(ilo[3 * inst + a], lo[a]), ihi[3 * inst + a] = std::max(ihi[3 * inst + a], hi[a]);
}

// Where the random walks' rays start (dscene.h::SssEntry): per instance, the cut of the Q tree (cs->q.nodes: its nodes on the host) around
// the instance's bounds; none without a Q tree or with !want.  *ms (optional): what building them took, untouched if none were built.
static int update_walk_entries(pbrhip_scene* s, const Knobs& k, bool want, const std::vector<float>& ilo, const std::vector<float>& ihi, CommitStage* cs, double* ms) {
  cs->walk_entries.clear();
  if (want && !cs->q.nodes.empty()) {
    const auto t_entries = std::chrono::steady_clock::now();
    // (every foreign reference costs each walk ray a slab test: a deeper entry is only worth so many)
    cs->walk_entries = build_sss_entries(cs->q.nodes, ilo, ihi, std::min(k.sss_foreign, kSssMaxForeign));
    if (ms) *ms = ms_since(t_entries);
  }
  s->num_walk_entries = (uint32_t)cs->walk_entries.size();
  if (cs->walk_entries.empty()) s->d_sss_entries.release();
  else HIPCHK(s->d_sss_entries.upload(cs->walk_entries, s->stream));
  return PBRHIP_OK;
}

int pb::ensure_shadow_grid(pbrhip_scene* s, const Knobs& k) {
  ShaftState& g = s->shaft;
  DScene& d = s->dscene;
  const TreeBufs& t = s->tree;
  const uint32_t nl = (uint32_t)s->lights.size();
  // who gets one: a triangle-only scene with a Q tree (the cells list its TriPair leaves) and 1 .. kShaftMaxLights lights whose records
  // are what the raytracer sees
  bool want = k.shadow_grid > 0 && k.shadow_grid_list > 0 && nl >= 1 && nl <= kShaftMaxLights && !s->lights_transformed && t.wide_nodes > 0 && s->num_curves == 0 &&
              s->light_box.size() == 6 * (size_t)nl;
  for (size_t i = 0; want && i < s->light_box.size(); i++) want = std::isfinite(s->light_box[i]);
  for (int a = 0; a < 3; a++) want = want && std::isfinite(s->bmin[a]) && std::isfinite(s->bmax[a]);
  const uint32_t n = want ? k.shadow_grid : 0u;
  if (!(g.valid && g.n == n && (n == 0 || (g.max_list == k.shadow_grid_list && g.num_lights == nl)))) {
    g.valid = false;
    if (n == 0) {
      g.drop();
    } else {
      const size_t words = (size_t)n * n * n * nl * kShaftCellWords;
      HIPCHK(hipSetDevice(s->device));
      HIPCHK(g.cells.reserve(words));
      ShaftBuild b;
      b.tree.nodes = reinterpret_cast<const QNode*>(t.d_wide.p), b.tree.tri = t.tri(), b.tree.num_nodes = t.wide_nodes;
      b.frame = shaft_frame(s->bmin, s->bmax, n);
      b.margin = shaft_margin(s->bmin, s->bmax);
      b.num_lights = nl, b.max_list = k.shadow_grid_list;
      for (uint32_t l = 0; l < nl; l++)
        for (int a = 0; a < 3; a++) b.light_lo[l][a] = s->light_box[6 * l + a], b.light_hi[l][a] = s->light_box[6 * l + 3 + a];
      HIPCHK(hipStreamSynchronize(s->stream));  // (what follows is the build's own time)
      const auto t0 = std::chrono::steady_clock::now();
      HIPCHK(build_shaft_grid_gpu(s->stream, b, g.cells.p));
      HIPCHK(hipStreamSynchronize(s->stream));
      g.build_ms = ms_since(t0);
      g.n = n, g.max_list = k.shadow_grid_list, g.num_lights = nl;
      if (k.debug) fprintf(stderr, "pbrhip: shaft grid: %u^3 cells x %u lights, lists of at most %u leaves, %.1f MB, built in %.2f ms\n", n, nl, g.max_list, words * 4 / 1048576.0, g.build_ms);
    }
    g.valid = true;
  }
  d.shaft_cells = g.n ? reinterpret_cast<const uint4*>(g.cells.p) : nullptr, d.shaft_n = g.n;
  if (g.n) {
    const ShaftFrame f = shaft_frame(s->bmin, s->bmax, g.n);
    for (int a = 0; a < 3; a++) d.shaft_org[a] = f.org[a], d.shaft_inv[a] = f.inv[a];
  }
  return PBRHIP_OK;
}

void pb::bind_dscene(pbrhip_scene* s) {
  DScene& d = s->dscene;
  const TreeBufs& t = s->tree;
  d.nodes = t.d_nodes.p, d.slots = t.slots(), d.num_nodes = t.num_nodes, d.num_slots = t.num_slots;
  d.top_nodes = s->bvh_built_on_gpu ? 0u : std::min<uint32_t>(t.num_nodes, (uint32_t)kTopNodes);
  d.wide = t.wide_nodes ? t.d_wide.p : nullptr, d.q_hitcode = t.wide_nodes ? t.d_qhit.p : nullptr, d.wide_nodes = t.wide_nodes;
  d.q_tri0 = (uint32_t)t.tri0(), d.q_pt0 = (uint32_t)t.pt0();
  d.shade = s->d_shade.p, d.num_curves = s->num_curves;
  d.materials = s->d_materials.p, d.num_materials = (uint32_t)s->materials.size();
  d.light_cdf = s->d_light_cdf.p, d.light_heads = s->d_heads.p, d.num_lights = (uint32_t)s->lights.size();
  d.lprim_cdf = s->d_lprim_cdf.p, d.lrecs = s->d_lrecs.p, d.num_lrecs = s->num_lrecs;
  d.light_boxes = s->d_light_boxes.p, d.lights_transformed = s->lights_transformed ? 1u : 0u;
  d.tex_pixels = s->d_tex_pixels.p, d.textures = s->d_tex_descs.p, d.num_textures = (uint32_t)s->tex_descs.size();
  d.sss_entries = s->num_walk_entries ? s->d_sss_entries.p : nullptr, d.num_sss_entries = s->num_walk_entries;
}

extern "C" int pbrhip_scene_commit(pbrhip_scene* s) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  const int builder = k.bvh >= 0 ? k.bvh : s->bvh_builder;
  CommitStage cs;  // (outlives the synchronise below)
  // the steps rewrite what the scene records and reallocate its device buffers: one that fails leaves the scene uncommitted, not
  // bound to tables that were never uploaded or to freed memory
  s->committed = false;
  s->dg.drop();  // (device geometry mode ends with the commit it belonged to)
  s->pose_set = false, s->pose_slots.release();  // (a pose snapshot is in the old tree's slot order: DESIGN.md §16)
  stage_lights(s, &cs);
  if (int rc = flatten_prims(s, &cs.prims)) return rc;
  const uint32_t np = (uint32_t)cs.prims.size();
  if (np >= (1u << 27)) return fail(PBRHIP_EUNSUPPORTED, "too many primitives (%u)", np);
  prim_boxes(s, cs.prims, &cs.lo, &cs.hi, &cs.kinds);
  scene_bounds(s);
  s->num_curves = (uint32_t)(cs.kinds.size() - std::count(cs.kinds.begin(), cs.kinds.end(), 0));
  if (int rc = build_binary_tree(s, k, builder, &cs)) return rc;
  if (int rc = stage_slots_and_materials(s, &cs)) return rc;
  const TreeBufs& t = s->tree;
  if (t.num_slots) HIPCHK(hipMemcpyAsync(t.slots(), cs.slots.data(), (size_t)t.num_slots * 64, hipMemcpyHostToDevice, s->stream));
  if (int rc = build_wide_tree(s, k, builder, &cs)) return rc;
  s->inst_lo.assign(3 * s->instances.size(), INFINITY), s->inst_hi.assign(3 * s->instances.size(), -INFINITY);  // (kept for pbrhip_scene_refit)
  for (size_t g = 0; g < cs.prims.size(); g++) accumulate_instance_bounds(s->inst_lo, s->inst_hi, cs.prims[g].instance_id, &cs.lo[3 * g], &cs.hi[3 * g]);
  double ms_entries = -1.0;  // (whatever the materials are now: pbrhip_scene_update_* can switch subsurface on later)
  if (int rc = update_walk_entries(s, k, k.sss_entry, s->inst_lo, s->inst_hi, &cs, &ms_entries)) return rc;
  if (k.debug) {
    if (ms_entries >= 0.0) fprintf(stderr, "pbrhip: commit: random walks' entries over %zu wide nodes: %.2f ms\n", cs.q.nodes.size(), ms_entries);
    for (size_t i = 0; i < cs.walk_entries.size(); i++)
      if (cs.walk_entries[i].entry) fprintf(stderr, "pbrhip: commit: instance %zu: random walks start at Q node %u with %u foreign references\n", i, cs.walk_entries[i].entry, cs.walk_entries[i].nforeign);
    fprintf(stderr, "pbrhip: commit: %u binary nodes, %zu wide nodes, %zu slots, %zu triangle leaves + %zu points in the Q tree\n", t.num_nodes, (size_t)t.wide_nodes, (size_t)t.num_slots, t.tri_words / kTriPairWords, t.points);
  }
  HIPCHK(s->d_shade.upload(cs.shade, s->stream));
  HIPCHK(s->d_materials.upload(cs.mats, s->stream));
  if (int rc = upload_lights(s, cs)) return rc;
  HIPCHK(s->d_tex_pixels.upload(s->tex_pixels, s->stream));
  HIPCHK(s->d_tex_descs.upload(s->tex_descs, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  bind_dscene(s);
  // what pbrhip_scene_refit needs of this commit; the device scene is the model's again
  s->slot_gid = std::move(cs.bvh.slot_gid);
  s->rf_plan.release();
  s->sdf.drop();  // (slot order and topology may have changed)
  s->shaft.valid = false;  // (the trees, the lights or the bounds may have changed)
  if (int rc = ensure_shadow_grid(s, k)) return rc;
  s->dirty_inst.assign(s->instances.size(), 0), s->stale = false;
  s->committed = true;
  return PBRHIP_OK;
  });
}

int pb::update_material(pbrhip_scene* s, uint32_t id, const HostMaterial& hm) {
  // validate everything first: a rejected call leaves the host material, has_sss and the device copy as they were
  if (id >= s->materials.size()) return fail(PBRHIP_EINVAL, "material id %u out of range", id);
  if (s->materials[id].kind != hm.kind) return fail(PBRHIP_EINVAL, "material %u is of the other kind", id);
  if (s->committed && hm.kind == kMatPrincipled)
    for (uint32_t t : {hm.pr.base_color_tex_id, hm.pr.subsurface_color_tex_id})
      if (t != kNone && t >= s->tex_descs.size()) return fail(PBRHIP_EINVAL, "texture id %u out of range", t);
  if (s->committed) {
    HIPCHK(hipSetDevice(s->device));
    const Material m = make_material(hm);
    HIPCHK(hipMemcpyAsync(s->d_materials.p + id, &m, sizeof(m), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->has_sss = s->has_sss || (m.kind == kMatPrincipled && (m.bsdf.enable_subsurface || m.textured));
    s->has_textured = s->has_textured || (m.kind == kMatPrincipled && m.textured);
  }
  s->materials[id] = hm;
  return PBRHIP_OK;
}

// ------------------------------------------------------------------ device geometry mode (geom_gpu.h; DESIGN.md section 8, "Staging on the device")
static const std::vector<float>& mesh_positions(const HostMesh& m) { return m.kind == 0 ? m.vertices : m.cverts; }
static const std::vector<uint32_t>& mesh_indices(const HostMesh& m) { return m.kind == 0 ? m.vid : m.cidx; }

// The one-off cost of the mode: every mesh's arrays, the (instance, geom) -> mesh table and the instances' slot lists go to the device;
// the instances' local boxes are cached for scene_bounds' last step.  The model is read as it stands.
static int switch_on_device_geometry(pbrhip_scene* s) {
  DevGeom& g = s->dg;
  hipStream_t st = s->stream;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t ninst = s->instances.size();
  const uint32_t ns = s->tree.num_slots;
  std::vector<PrimRef> prims;
  if (int rc = flatten_prims(s, &prims)) return rc;
  if (s->slot_gid.size() != ns || prims.size() != ns) return fail(PBRHIP_ESTATE, "the model no longer has the committed topology");
  std::vector<float> verts, normals;
  std::vector<uint32_t> vidx, nidx, geom_mesh, ig_off(ninst), slot_list(ns);
  g.h_recs.clear();
  for (const HostMesh& m : s->meshes) {
    const std::vector<float>& pos = mesh_positions(m);
    const std::vector<uint32_t>& idx = mesh_indices(m);
    DgMeshRec r = {};
    r.vert_off = (uint32_t)(verts.size() / 4), r.nverts = (uint32_t)(pos.size() / 4);
    r.idx_off = (uint32_t)vidx.size(), r.nidx = (uint32_t)idx.size();
    verts.insert(verts.end(), pos.begin(), pos.end());
    vidx.insert(vidx.end(), idx.begin(), idx.end());
    if (m.kind == 0) {
      r.norm_off = (uint32_t)(normals.size() / 4), r.nnorm = (uint32_t)(m.normals.size() / 4), r.nid_off = (uint32_t)nidx.size();
      normals.insert(normals.end(), m.normals.begin(), m.normals.end());
      nidx.insert(nidx.end(), m.nid.begin(), m.nid.end());
    }
    g.h_recs.push_back(r);
  }
  if (std::max({verts.size() / 4, normals.size() / 4, vidx.size(), nidx.size()}) >= (size_t(1) << 31))
    return fail(PBRHIP_EUNSUPPORTED, "device geometry: the meshes' arrays are too large for 32-bit offsets");
  for (size_t i = 0; i < ninst; i++) {
    ig_off[i] = (uint32_t)geom_mesh.size();
    for (uint32_t m : s->locals[s->instances[i].local_scene]) geom_mesh.push_back(m);
  }
  // the slots grouped by instance, in slot order within one
  g.inst_first.assign(ninst + 1, 0);
  for (uint32_t k = 0; k < ns; k++) g.inst_first[prims[s->slot_gid[k]].instance_id + 1]++;
  for (size_t i = 0; i < ninst; i++) g.inst_first[i + 1] += g.inst_first[i];
  std::vector<uint32_t> at(g.inst_first.begin(), g.inst_first.end() - 1);
  for (uint32_t k = 0; k < ns; k++) slot_list[at[prims[s->slot_gid[k]].instance_id]++] = k;
  g.local_lo.assign(3 * ninst, INFINITY), g.local_hi.assign(3 * ninst, -INFINITY);
  for (size_t i = 0; i < ninst; i++) instance_local_box(s, (uint32_t)i, &g.local_lo[3 * i], &g.local_hi[3 * i]);
  g.ngeoms = (uint32_t)geom_mesh.size();
  auto upload4 = [&](DevBuf<float4>& b, const std::vector<float>& h) {  // (xyzw per element)
    hipError_t e4 = b.reserve(h.size() / 4);
    if (e4 == hipSuccess && !h.empty()) e4 = hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, st);
    return e4;
  };
  hipError_t e = upload4(g.verts, verts);
  if (e == hipSuccess) e = upload4(g.normals, normals);
  if (e == hipSuccess) e = g.vidx.upload(vidx, st);
  if (e == hipSuccess) e = g.nidx.upload(nidx, st);
  if (e == hipSuccess) e = g.recs.upload(g.h_recs, st);
  if (e == hipSuccess) e = g.geom_mesh.upload(geom_mesh, st);
  if (e == hipSuccess) e = g.ig_off.upload(ig_off, st);
  if (e == hipSuccess) e = g.slot_list.upload(slot_list, st);
  if (e == hipSuccess) e = g.xf.reserve(ninst);
  if (e == hipSuccess) e = g.bounds.reserve(ninst * kDgBoundWords);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the staged arrays die here)
  if (e != hipSuccess) {
    const double keep = g.download_ms;
    g.drop();
    g.download_ms = keep;
    return fail(PBRHIP_EHIP, "device geometry: the upload of the meshes failed: %s", hipGetErrorString(e));
  }
  g.on = true;
  g.switch_ms += ms_since(t0);
  return PBRHIP_OK;
}

int pb::update_mesh_device(pbrhip_scene* s, uint32_t mesh_id, const void* d_verts, const void* d_normals, void* stream, const char* who) {
  DevGeom& g = s->dg;
  HostMesh& m = s->meshes[mesh_id];
  std::vector<float>& pos = m.kind == 0 ? m.vertices : m.cverts;
  const size_t nv = pos.size() / 4, nn = d_normals ? m.normals.size() / 4 : 0;
  if (g.on && mesh_id >= g.h_recs.size()) return fail(PBRHIP_ESTATE, "%s: mesh %u was added after the commit (pbrhip_scene_commit takes it in)", who, mesh_id);
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const auto t0 = std::chrono::steady_clock::now();
  {  // the arrays are read only after what the caller's stream already holds: an event there, and this scene's stream waits for it
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    (void)hipEventDestroy(ev);
    HIPCHK(e);
  }
  // checked on the device; on a committed scene copied beside the device copy meanwhile, so that a refused array never reaches it and an
  // accepted one needs no second read of the caller's buffer
  float4* inc = nullptr;
  if (s->committed) {
    HIPCHK(g.incoming.reserve(nv + nn));
    inc = g.incoming.p;
  }
  HIPCHK(g.flag.reserve(1));
  HIPCHK(hipMemsetAsync(g.flag.p, 0, sizeof(uint32_t), st));
  HIPCHK(dg_check_gpu(st, d_verts, nv, inc, g.flag.p));
  if (nn) HIPCHK(dg_check_gpu(st, d_normals, nn, inc ? inc + nv : nullptr, g.flag.p));
  std::vector<float> hv(4 * nv), hn(4 * nn);
  uint32_t flag = 0;
  if (nv) HIPCHK(hipMemcpyAsync(hv.data(), inc ? (const void*)inc : d_verts, nv * 16, hipMemcpyDeviceToHost, st));
  if (nn) HIPCHK(hipMemcpyAsync(hn.data(), inc ? (const void*)(inc + nv) : d_normals, nn * 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&flag, g.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // (the one synchronise of the call: the caller may overwrite its buffer from here on)
  if (flag) return fail(PBRHIP_EINVAL, "%s: a value is not finite", who);
  g.download_ms += ms_since(t0);
  if (s->committed && !g.on)
    if (int rc = switch_on_device_geometry(s)) return rc;  // (before the model changes: a failure leaves everything as it was)
  pos.swap(hv);
  if (nn) m.normals.swap(hn);
  if (g.on) {
    const DgMeshRec& r = g.h_recs[mesh_id];
    if (nv) HIPCHK(hipMemcpyAsync(g.verts.p + r.vert_off, inc, nv * 16, hipMemcpyDeviceToDevice, st));
    if (nn) HIPCHK(hipMemcpyAsync(g.normals.p + r.norm_off, inc + nv, nn * 16, hipMemcpyDeviceToDevice, st));
  }
  return PBRHIP_OK;
}

int pb::refresh_mesh_device(pbrhip_scene* s, uint32_t mesh_id) {
  DevGeom& g = s->dg;
  if (!g.on || mesh_id >= g.h_recs.size()) return PBRHIP_OK;  // (a mesh added after the commit is in no committed instance)
  const HostMesh& m = s->meshes[mesh_id];
  const DgMeshRec& r = g.h_recs[mesh_id];
  const std::vector<float>& pos = mesh_positions(m);
  HIPCHK(hipSetDevice(s->device));
  if (r.nverts) HIPCHK(hipMemcpyAsync(g.verts.p + r.vert_off, pos.data(), (size_t)r.nverts * 16, hipMemcpyHostToDevice, s->stream));
  if (r.nnorm) HIPCHK(hipMemcpyAsync(g.normals.p + r.norm_off, m.normals.data(), (size_t)r.nnorm * 16, hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return PBRHIP_OK;
}

// What refit stages for the dirty instances, one of two ways.  Both leave the new slots and ShadeRecs on the device, the dirty instances'
// world bounds in ilo / ihi, the scene's box in s->bmin / bmax and the number of dirty slots in *m.
// On the host: flatten_prims, slot_and_shade per dirty slot, scene_bounds over the whole model, one packed upload and k_rf_scatter.
// (`packed` is handed to hipMemcpyAsync from pageable memory: the caller owns it until its final synchronise)
static int stage_refit_host(pbrhip_scene* s, std::chrono::steady_clock::time_point t_host, std::vector<float>& ilo, std::vector<float>& ihi, std::vector<float4>& packed,
                            uint32_t* m_out, double* ms_host, double* ms_upload) {
  hipStream_t st = s->stream;
  const TreeBufs& t = s->tree;
  std::vector<PrimRef> prims;
  if (int rc = flatten_prims(s, &prims)) return rc;
  const uint32_t ns = t.num_slots;
  if (s->slot_gid.size() != ns || prims.size() != ns) return fail(PBRHIP_ESTATE, "scene_refit: the model no longer has the committed topology");
  std::vector<uint32_t> dirty;
  for (uint32_t slot = 0; slot < ns; slot++)
    if (s->dirty_inst[prims[s->slot_gid[slot]].instance_id]) dirty.push_back(slot);
  const uint32_t m = (uint32_t)dirty.size();
  const size_t idx_words = ((size_t)m + 3) / 4;
  packed.assign(idx_words + 12 * (size_t)m, make_float4(0, 0, 0, 0));
  for (uint32_t e = 0; e < m; e++) {
    const uint32_t g = s->slot_gid[dirty[e]];
    float4* sl = &packed[idx_words + 4 * (size_t)e];
    ShadeRec sr;
    if (int rc = slot_and_shade(s, prims[g], g, s->light_heads, sl, sr)) return rc;
    reinterpret_cast<uint32_t*>(packed.data())[e] = dirty[e];
    memcpy(&packed[idx_words + 4 * (size_t)m + 8 * (size_t)e], &sr, sizeof(sr));
    float lo[3], hi[3];
    slot_tight_box(sl, prims[g].kind != 0, lo, hi);
    accumulate_instance_bounds(ilo, ihi, prims[g].instance_id, lo, hi);
  }
  scene_bounds(s);
  *ms_host = ms_since(t_host);
  const auto t_up = std::chrono::steady_clock::now();
  HIPCHK(s->rf_packed.upload(packed, st));
  HIPCHK(scatter_slots_gpu(st, s->rf_packed.p, m, ns, t.slots(), reinterpret_cast<float4*>(s->d_shade.p)));
  *ms_upload = ms_since(t_up);
  *m_out = m;
  return PBRHIP_OK;
}
// On the device (device geometry mode): the instances' transforms as a small table, k_dg_stage per dirty instance, the bounds back.  The
// scene's box is finished here as scene_bounds finishes it -- instances in ascending order -- from the dirty instances' new local boxes
// (llo / lhi: every instance's, the clean ones' as cached) .
static int stage_refit_device(pbrhip_scene* s, std::vector<float>& ilo, std::vector<float>& ihi, std::vector<float>& llo, std::vector<float>& lhi, uint32_t* m_out) {
  DevGeom& g = s->dg;
  hipStream_t st = s->stream;
  const TreeBufs& t = s->tree;
  const size_t ninst = s->instances.size();
  if (g.inst_first.size() != ninst + 1 || g.inst_first[ninst] != t.num_slots) return fail(PBRHIP_ESTATE, "scene_refit: the model no longer has the committed topology");
  g.h_xf.resize(ninst);
  for (size_t i = 0; i < ninst; i++) {
    memcpy(g.h_xf[i].m, s->instances[i].xf, sizeof(g.h_xf[i].m));
    g.h_xf[i].identity = s->instances[i].identity ? 1u : 0u;
  }
  HIPCHK(g.xf.upload(g.h_xf, st));
  HIPCHK(hipMemsetAsync(g.flag.p, 0, sizeof(uint32_t), st));
  HIPCHK(dg_init_bounds_gpu(st, g.bounds.p, (uint32_t)ninst));
  DgScene d;
  d.slots = t.slots(), d.shade = reinterpret_cast<float4*>(s->d_shade.p), d.ns = t.num_slots;
  d.verts = g.verts.p, d.normals = g.normals.p, d.vidx = g.vidx.p, d.nidx = g.nidx.p, d.recs = g.recs.p;
  d.geom_mesh = g.geom_mesh.p, d.ig_off = g.ig_off.p, d.ngeoms = g.ngeoms, d.slot_list = g.slot_list.p, d.xf = g.xf.p;
  d.bounds = g.bounds.p, d.flag = g.flag.p;
  uint32_t m = 0;
  for (size_t i = 0; i < ninst; i++)
    if (s->dirty_inst[i]) {
      const uint32_t count = g.inst_first[i + 1] - g.inst_first[i];
      HIPCHK(dg_stage_gpu(st, d, (uint32_t)i, g.inst_first[i], count));
      m += count;
    }
  g.h_bounds.assign(ninst * kDgBoundWords, 0u);
  uint32_t flag = 0;
  if (ninst) HIPCHK(hipMemcpyAsync(g.h_bounds.data(), g.bounds.p, g.h_bounds.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&flag, g.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (flag) return fail(PBRHIP_ESTATE, "scene_refit: the device geometry tables hold an index out of range; the scene stays stale (pbrhip_scene_commit rebuilds it)");
  const float inf = std::numeric_limits<float>::infinity();
  float bmin[3] = {inf, inf, inf}, bmax[3] = {-inf, -inf, -inf};
  for (size_t i = 0; i < ninst; i++) {
    if (g.inst_first[i + 1] == g.inst_first[i]) continue;  // (no primitive: no box)
    if (s->dirty_inst[i]) {
      const uint32_t* b = &g.h_bounds[i * kDgBoundWords];
      for (int a = 0; a < 3; a++) {
        llo[3 * i + a] = dg_decode(b[a]), lhi[3 * i + a] = dg_decode(b[3 + a]);
        ilo[3 * i + a] = dg_decode(b[6 + a]), ihi[3 * i + a] = dg_decode(b[9 + a]);
      }
    }
    unite_instance_box(s->instances[i], &llo[3 * i], &lhi[3 * i], bmin, bmax);
  }
  memcpy(s->bmin, bmin, sizeof(bmin)), memcpy(s->bmax, bmax, sizeof(bmax));
  *m_out = m;
  return PBRHIP_OK;
}

extern "C" int pbrhip_scene_refit(pbrhip_scene* s) {
  return guarded([&]() -> int {
  if (!s) return fail(PBRHIP_EINVAL, "scene is NULL");
  if (s->replica) return fail(PBRHIP_ESTATE, "scene_refit: a replica holds no geometry (refit the source scene and replicate it again)");
  if (!s->committed) return fail(PBRHIP_ESTATE, "scene not committed");
  if (!s->stale) return PBRHIP_OK;
  s->shaft.valid = false, s->dscene.shaft_cells = nullptr;  // ... and so is what the shaft grid was cut from: it is made again before the next render
  s->sdf.table_valid = false;  // the slots are about to change: the pseudonormal table is made again when it is next asked for
  const Knobs k = read_knobs();
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const TreeBufs& t = s->tree;
  const auto t_stage = std::chrono::steady_clock::now();
  const size_t ninst = s->instances.size();
  s->dirty_inst.resize(ninst, 0);
  CommitStage cs;  // (outlives the last synchronise)
  // light tables: positions, areas and with them every probability
  bool lights_dirty = false;
  for (size_t i = 0; i < ninst; i++)
    if (s->dirty_inst[i])
      for (int has : s->instances[i].has_area_light) lights_dirty = lights_dirty || has != 0;
  if (lights_dirty) stage_lights(s, &cs);
  // the dirty slots and their ShadeRecs; the dirty instances' bounds from their new boxes
  const uint32_t ns = t.num_slots;
  std::vector<float> ilo = s->inst_lo, ihi = s->inst_hi;
  for (size_t i = 0; i < ninst; i++)
    if (s->dirty_inst[i])
      for (int a = 0; a < 3; a++) ilo[3 * i + a] = INFINITY, ihi[3 * i + a] = -INFINITY;
  float keep_min[3], keep_max[3];  // (a failed refit leaves the scene as stale as it was)
  memcpy(keep_min, s->bmin, 12), memcpy(keep_max, s->bmax, 12);
  const bool on_device = s->dg.on;
  std::vector<float> llo, lhi;
  std::vector<float4> packed;
  uint32_t m = 0;
  double ms_host = 0.0, ms_upload = 0.0;
  int rc;
  if (on_device) {
    llo = s->dg.local_lo, lhi = s->dg.local_hi;
    rc = stage_refit_device(s, ilo, ihi, llo, lhi, &m);
  } else {
    rc = stage_refit_host(s, t_stage, ilo, ihi, packed, &m, &ms_host, &ms_upload);
  }
  if (rc) {
    memcpy(s->bmin, keep_min, 12), memcpy(s->bmax, keep_max, 12);
    return rc;
  }
  const double ms_stage = ms_since(t_stage);
  const auto t_lights = std::chrono::steady_clock::now();
  if (lights_dirty)
    if (int rc2 = upload_lights(s, cs)) return rc2;
  if (k.debug) HIPCHK(hipStreamSynchronize(st));
  ms_upload += ms_since(t_lights);

  RefitTimes rt;
  HIPCHK(refit_tree_gpu(st, t.refit_tree(s->num_curves == 0), k.debug, &s->rf_plan, &rt));
  if (rt.failed) {
    memcpy(s->bmin, keep_min, 12), memcpy(s->bmax, keep_max, 12);
    return fail(PBRHIP_EHIP, "scene_refit: %s; the scene stays stale (pbrhip_scene_commit rebuilds it)",
                (rt.failed & 1u) ? "a node of the Q tree cannot be quantised" : "the committed tree holds an index out of range");
  }
  const auto t_entries = std::chrono::steady_clock::now();
  if (t.wide_nodes && s->num_walk_entries) {  // (the scene has them: made again for the new bounds, over the refitted nodes)
    cs.q.nodes.resize(t.wide_nodes);
    HIPCHK(hipMemcpyAsync(cs.q.nodes.data(), t.d_wide.p, cs.q.nodes.size() * sizeof(QNode), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc2 = update_walk_entries(s, k, true, ilo, ihi, &cs, nullptr)) return rc2;
  }
  HIPCHK(hipStreamSynchronize(st));
  if (k.debug && !on_device)
    fprintf(stderr, "pbrhip: refit: %u of %u slots dirty: host staging %.2f ms, upload + scatter %.2f ms, plan %.2f ms, pack + trees %.2f ms (%u + %u levels), Q-node download + walk entries %.2f ms\n",
            m, ns, ms_host, ms_upload, rt.plan_ms, rt.trees_ms, rt.bin_levels, rt.q_levels, ms_since(t_entries));
  if (k.debug && on_device)
    fprintf(stderr, "pbrhip: refit (device geometry): %u of %u slots dirty: switch-on %.2f ms, updates' check + download to the model %.2f ms, staging + bounds kernels %.2f ms, light tables %.2f ms, plan %.2f ms, pack + trees %.2f ms (%u + %u levels), Q-node download + walk entries %.2f ms\n",
            m, ns, s->dg.switch_ms, s->dg.download_ms, ms_stage, ms_upload, rt.plan_ms, rt.trees_ms, rt.bin_levels, rt.q_levels, ms_since(t_entries));
  bind_dscene(s);
  s->inst_lo = std::move(ilo), s->inst_hi = std::move(ihi);
  if (on_device) s->dg.local_lo = std::move(llo), s->dg.local_hi = std::move(lhi), s->dg.switch_ms = s->dg.download_ms = 0.0;
  s->dirty_inst.assign(ninst, 0), s->stale = false;
  return PBRHIP_OK;
  });
}
