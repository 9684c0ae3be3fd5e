// A C++ caller of pbrlab::Scene::TraceClosestDevice, TraceAnyDevice, NearestPoint and NearestPointDevice (include/pbrlab_hip.hpp): a unit
// quad at z = 0 in front of a wall at z = -2.  Rays and points go to device memory through the HIP runtime the library links (three of
// its functions, declared here: the caller needs no HIP headers), the answers come back and are printed as hexadecimal words, one query
// per line, for tests/test_query_shim.py to compare with the Python binding's answers on the same scene.
// Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = a result that breaks the contract.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "pbrlab_hip.hpp"

extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);  // kind 1: host to device, 2: device to host
}

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  try {
    pbrlab::Scene scene;
    pbrlab::CyclesPrincipledBsdfParameter grey;
    grey.base_color = pbrlab::float3(0.25f);
    const uint32_t mat = scene.AddMaterialParam(grey);
    const float I[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int k = 0; k < 2; k++) {
      auto attr = std::make_shared<pbrlab::Attribute>();
      const float r = k ? 8.0f : 1.0f, z = k ? -2.0f : 0.0f;
      attr->vertices = {-r, -r, z, 1, r, -r, z, 1, r, r, z, 1, -r, r, z, 1};
      const pbrlab::MeshPtr quad = scene.AddTriangleMesh(k ? "wall" : "quad", attr, std::vector<uint32_t>{0, 1, 2, 0, 2, 3}, std::vector<uint32_t>{},
                                                         std::vector<uint32_t>{}, std::vector<uint32_t>{mat, mat});
      const uint32_t ls = scene.CreateLocalScene();
      scene.AddMeshToLocalScene(ls, quad);
      scene.CreateInstance(ls, I);
    }
    scene.CommitScene();
    const float inf = std::numeric_limits<float>::infinity();
    // rays: at the quad, past it at the wall, away from both, one that stops short, an inactive one (zero direction)
    const std::vector<pbrhip_ray> rays = {{{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, inf},  {{3.0f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, inf},
                                          {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, 1}, inf},   {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, 2.5f},
                                          {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, 0}, inf},   {{0.1f, -0.7f, 1.0f}, 0.0f, {0.3f, 0.2f, -1.0f}, 100.0f}};
    // points: above the quad, beside it, behind the wall, one with a bound nothing meets, an inactive one (NaN)
    const std::vector<pbrhip_point> pts = {{{0.25f, 0.5f, 1.0f}, inf},  {{1.5f, 0.25f, 0.25f}, inf}, {{4.0f, -3.0f, -2.5f}, inf},
                                           {{0.25f, 0.5f, 1.0f}, 0.5f}, {{std::nanf(""), 0, 0}, inf}, {{-0.3f, 0.9f, -0.7f}, 1.25f}};
    const size_t nr = rays.size(), np = pts.size();
    void *d_rays = nullptr, *d_pts = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_rays, nr * sizeof(pbrhip_ray)) || hipMalloc(&d_pts, np * sizeof(pbrhip_point)) || hipMalloc(&d_out, 4096)) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(d_rays, rays.data(), nr * sizeof(pbrhip_ray), 1) || hipMemcpy(d_pts, pts.data(), np * sizeof(pbrhip_point), 1)) throw std::runtime_error("hipMemcpy failed");
    uint32_t* d_ident = static_cast<uint32_t*>(d_out);                                   // 16 bytes per query
    pbrhip_hit* d_hits = reinterpret_cast<pbrhip_hit*>(static_cast<char*>(d_out) + 1024);  // 36
    uint8_t* d_occ = static_cast<uint8_t*>(d_out) + 2048;
    float* d_closest = reinterpret_cast<float*>(static_cast<char*>(d_out) + 3072);       // 16
    std::vector<uint32_t> ident(4 * nr), nident(4 * np), hident;
    std::vector<pbrhip_hit> hits(nr);
    std::vector<uint8_t> occ(nr);
    std::vector<float> closest(4 * np), hclosest;
    scene.TraceClosestDevice(d_rays, nr, d_ident, d_hits);
    scene.TraceAnyDevice(d_rays, nr, d_occ);
    if (hipMemcpy(ident.data(), d_ident, 16 * nr, 2) || hipMemcpy(hits.data(), d_hits, sizeof(pbrhip_hit) * nr, 2) || hipMemcpy(occ.data(), d_occ, nr, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.NearestPointDevice(d_pts, np, d_ident, d_closest);
    if (hipMemcpy(nident.data(), d_ident, 16 * np, 2) || hipMemcpy(closest.data(), d_closest, 16 * np, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.NearestPoint(pts, &hident, &hclosest);
    hipFree(d_rays), hipFree(d_pts), hipFree(d_out);
    if (hident != nident || memcmp(hclosest.data(), closest.data(), 16 * np) != 0) return 2;  // host and device variants agree
    // what the geometry says: ray 0 hits the quad at t = 3, ray 1 the wall at t = 5, rays 2 .. 4 nothing; point 0 is 1 above the quad
    if (ident[3] != bits(3.0f) || ident[7] != bits(5.0f) || ident[8] != PBRHIP_NONE || ident[12] != PBRHIP_NONE || ident[16] != PBRHIP_NONE) return 2;
    if (hits[0].instance_id != 0 || hits[1].instance_id != 1 || hits[2].instance_id != PBRHIP_NONE || hits[0].t != 3.0f) return 2;
    if (occ[0] != 1 || occ[1] != 1 || occ[2] != 0 || occ[3] != 0 || occ[4] != 0) return 2;
    if (closest[3] != 1.0f || closest[0] != 0.25f || closest[1] != 0.5f || closest[2] != 0.0f || nident[3] != bits(1.0f)) return 2;
    if (nident[12] != PBRHIP_NONE || nident[16] != PBRHIP_NONE || closest[12] != 0.0f) return 2;
    for (size_t i = 0; i < nr; i++) {
      const pbrhip_hit& h = hits[i];
      printf("R %zu %08x %08x %08x %08x | %08x %08x %08x %08x %08x %08x %08x %08x %08x | %u\n", i, ident[4 * i], ident[4 * i + 1], ident[4 * i + 2], ident[4 * i + 3],
             bits(h.normal_g[0]), bits(h.normal_g[1]), bits(h.normal_g[2]), bits(h.t), bits(h.u), bits(h.v), h.instance_id, h.geom_id, h.prim_id, unsigned(occ[i]));
    }
    for (size_t i = 0; i < np; i++)
      printf("N %zu %08x %08x %08x %08x | %08x %08x %08x %08x\n", i, nident[4 * i], nident[4 * i + 1], nident[4 * i + 2], nident[4 * i + 3], bits(closest[4 * i]),
             bits(closest[4 * i + 1]), bits(closest[4 * i + 2]), bits(closest[4 * i + 3]));
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
