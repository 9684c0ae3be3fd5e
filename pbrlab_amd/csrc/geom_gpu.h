// geom_gpu.h -- device geometry mode ("Staging on the device"): what geom_gpu.hip offers the host code.  After the
// first pbrhip_scene_update_*_mesh_device call on a committed scene the library keeps every mesh's position, normal and index arrays
// on the device, and pbrhip_scene_refit re-derives the dirty instances' slots, ShadeRecs and bounds there (k_dg_stage) instead of
// staging them on the host.  The next commit drops all of it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pb {

// One mesh in the concatenated device arrays: `verts` holds its vertices xyzw (triangles) or control points xyzr (curves), `vidx` its
// vid (three per face) or cidx (one per curve); normals / nid likewise (triangle meshes only).  Counts are what the kernel checks an
// index against before it reads.
struct DgMeshRec {
  uint32_t vert_off, nverts, norm_off, nnorm, idx_off, nidx, nid_off, pad;
};
// An instance's transform as a refit sees it: 16 floats + "the matrix is the identity as bits" (such an instance shows its meshes as they are)
struct DgXf {
  float m[16];
  uint32_t identity, pad[3];
};
// Per instance twelve bounds in an order-preserving integer encoding of the float (dg_decode): local lo, local hi, world lo, world hi
constexpr uint32_t kDgBoundWords = 12;

struct DgScene {  // device pointers: the scene's buffers and the mode's tables
  float4* slots = nullptr;
  float4* shade = nullptr;
  uint32_t ns = 0;
  const float4* verts = nullptr;
  const float4* normals = nullptr;
  const uint32_t* vidx = nullptr;
  const uint32_t* nidx = nullptr;
  const DgMeshRec* recs = nullptr;
  const uint32_t* geom_mesh = nullptr;  // [ig_off[instance] + geom] -> mesh
  const uint32_t* ig_off = nullptr;
  uint32_t ngeoms = 0;                  // entries of geom_mesh
  const uint32_t* slot_list = nullptr;  // the slots grouped by instance
  const DgXf* xf = nullptr;
  uint32_t* bounds = nullptr;           // ninst x kDgBoundWords
  uint32_t* flag = nullptr;             // set when an index of the tables is out of range (nothing is read or written through it)
};

inline float dg_decode(uint32_t e) {  // the inverse of geom_gpu.hip::dg_encode
  const uint32_t u = (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// n 16-byte words of the caller's array: *flag |= 1 if a value is not finite; with dst, copied there as well
hipError_t dg_check_gpu(hipStream_t st, const void* src, size_t n, float4* dst, uint32_t* flag);
// every bound of ninst instances to the neutral element of its minimum / maximum
hipError_t dg_init_bounds_gpu(hipStream_t st, uint32_t* bounds, uint32_t ninst);
// the `count` slots slot_list[first ..] of instance `inst`, rewritten in place from the device arrays; its bounds accumulated
hipError_t dg_stage_gpu(hipStream_t st, const DgScene& d, uint32_t inst, uint32_t first, uint32_t count);

}  // namespace pb
