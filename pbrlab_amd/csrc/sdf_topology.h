// sdf_topology.h -- the adjacency the pseudonormal table of the signed-distance queries is gathered from.  Plain C++
// with no HIP in it: scripts/fuzz/sdf_topology_fuzz.cc builds sdf_topology.cpp on the CPU under a sanitizer.
//
// A FEATURE is an edge or a vertex of one object -- one (instance, geometry) pair --: two corners are the same vertex when they belong
// to the same object and carry the same position index (the mesh's vertex_ids entry); an edge is an unordered pair of such vertices.
// Equal positions under different indices are not welded.
#pragma once

#include <stdint.h>

#include <vector>

namespace pb {

constexpr uint32_t kSdfNone = 0xFFFFFFFFu;

struct SdfReport {
  uint32_t triangles = 0;          // triangle slots
  uint32_t vertices = 0;           // distinct vertices the triangles use
  uint32_t edges_manifold = 0;     // exactly two faces that run along it in opposite directions
  uint32_t edges_boundary = 0;     // one face
  uint32_t edges_nonmanifold = 0;  // three or more faces
  uint32_t edges_inconsistent = 0; // two faces that run along it in the same direction
};

struct SdfTopology {
  // per slot six feature ids, in the table's row order ab, bc, ca, a, b, c (kSdfNone six times: a curve piece)
  std::vector<uint32_t> slot_feat;
  // feature f gathers from items[off[f] .. off[f + 1]): (slot << 2) | corner, in ascending canonical id of the face.  corner 0, 1, 2 =
  // a, b, c names the corner of that face at a vertex feature (its angle is the weight); an edge feature's items carry 3.
  std::vector<uint32_t> feat_off, feat_items;
  SdfReport report;
};

// num_slots slots in leaf order.  slot_gid: slot -> canonical id (a permutation of 0 .. num_slots - 1).  Per canonical id g: object[g]
// = the index of its (instance, geometry) pair, or kSdfNone for a curve piece; vid[3 g ..] = its three position indices (not read for
// a curve piece).  Returns false -- and leaves *out empty -- when slot_gid is no such permutation or num_slots is 2^30 or more.
bool build_sdf_topology(uint32_t num_slots, const uint32_t* slot_gid, const uint32_t* object, const uint32_t* vid, SdfTopology* out);

}  // namespace pb
