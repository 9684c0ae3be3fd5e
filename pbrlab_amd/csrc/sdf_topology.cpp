// sdf_topology.cpp -- the incidence lists of the pseudonormal table and the topology report (sdf_topology.h).  Plain C++.
#include "sdf_topology.h"

#include <algorithm>

namespace pb {
namespace {

struct Incidence {
  uint32_t object, v0, v1;  // the feature's key: an edge (v0 <= v1), or a vertex (v1 = kSdfNone)
  uint32_t gid, slot;
  uint8_t corner;           // 0..2: the face's corner at a vertex; 3: an edge
  uint8_t forward;          // an edge: the face runs along it from v0 to v1
  bool same_feature(const Incidence& o) const { return object == o.object && v0 == o.v0 && v1 == o.v1; }
  bool operator<(const Incidence& o) const {
    if (object != o.object) return object < o.object;
    if (v0 != o.v0) return v0 < o.v0;
    if (v1 != o.v1) return v1 < o.v1;
    if (gid != o.gid) return gid < o.gid;
    return corner < o.corner;
  }
};

}  // namespace

bool build_sdf_topology(uint32_t num_slots, const uint32_t* slot_gid, const uint32_t* object, const uint32_t* vid, SdfTopology* out) {
  *out = SdfTopology();
  if (num_slots >= (1u << 30)) return false;
  std::vector<uint8_t> seen(num_slots, 0);
  for (uint32_t s = 0; s < num_slots; s++) {
    if (slot_gid[s] >= num_slots || seen[slot_gid[s]]) return false;
    seen[slot_gid[s]] = 1;
  }
  out->slot_feat.assign(6 * (size_t)num_slots, kSdfNone);
  // six incidences per triangle slot, in the table's row order (ab, bc, ca, a, b, c): an incidence's index modulo 6 is its row
  std::vector<Incidence> inc;
  for (uint32_t s = 0; s < num_slots; s++) {
    const uint32_t g = slot_gid[s];
    if (object[g] == kSdfNone) continue;
    out->report.triangles++;
    const uint32_t v[3] = {vid[3 * (size_t)g], vid[3 * (size_t)g + 1], vid[3 * (size_t)g + 2]};
    for (uint32_t k = 0; k < 3; k++) {  // edges ab, bc, ca
      const uint32_t from = v[k], to = v[(k + 1) % 3];
      inc.push_back({object[g], std::min(from, to), std::max(from, to), g, s, 3, (uint8_t)(from < to)});
    }
    for (uint32_t k = 0; k < 3; k++) inc.push_back({object[g], v[k], kSdfNone, g, s, (uint8_t)k, 0});
  }
  std::vector<uint32_t> order(inc.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  auto is_edge = [&](uint32_t i) { return inc[i].corner == 3; };
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (is_edge(a) != is_edge(b)) return is_edge(a);  // all edges, then all vertices
    return inc[a] < inc[b];
  });
  out->feat_off.push_back(0);
  for (size_t at = 0; at < order.size();) {
    size_t end = at + 1;
    while (end < order.size() && is_edge(order[end]) == is_edge(order[at]) && inc[order[end]].same_feature(inc[order[at]])) end++;
    const uint32_t f = (uint32_t)out->feat_off.size() - 1;
    uint32_t forward = 0;
    for (size_t i = at; i < end; i++) {
      const Incidence& r = inc[order[i]];
      out->feat_items.push_back((r.slot << 2) | r.corner);
      forward += r.forward;
      out->slot_feat[(size_t)r.slot * 6 + order[i] % 6] = f;
    }
    out->feat_off.push_back((uint32_t)out->feat_items.size());
    const size_t faces = end - at;
    if (!is_edge(order[at])) {
      out->report.vertices++;
    } else if (faces == 1) {
      out->report.edges_boundary++;
    } else if (faces >= 3) {
      out->report.edges_nonmanifold++;
    } else if (forward == 1) {
      out->report.edges_manifold++;
    } else {
      out->report.edges_inconsistent++;
    }
    at = end;
  }
  return true;
}

}  // namespace pb
