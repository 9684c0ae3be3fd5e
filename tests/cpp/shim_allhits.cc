// A C++ caller of pbrlab::Scene::TraceAll and TraceAllDevice (include/pbrlab_hip.hpp): tests/cpp/shim_query.cc's scene -- a unit quad at
// z = 0 in front of a wall at z = -2 -- with a second, coinciding wall, so that a ray through all three meets two hits at one t.  Rays go
// to device memory through the HIP runtime the library links (three of its functions, declared here: the caller needs no HIP headers);
// counts and rows are printed as hexadecimal words, one ray per line, for tests/test_allhits_shim.py to compare with the Python binding's.
// Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = a result that breaks the contract.
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
    for (int k = 0; k < 3; k++) {
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
    // rays: through the quad and both walls, past the quad at the walls, away from all, one that stops short of the walls, an inactive
    // one (zero direction), an oblique one
    const std::vector<pbrhip_ray> rays = {{{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, inf},  {{3.0f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, inf},
                                          {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, 1}, inf},   {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, -1}, 3.5f},
                                          {{0.25f, 0.5f, 3.0f}, 0.0f, {0, 0, 0}, inf},   {{0.1f, -0.7f, 1.0f}, 0.0f, {0.3f, 0.2f, -1.0f}, 100.0f}};
    const size_t n = rays.size();
    const uint32_t K = 2;
    void *d_rays = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_rays, n * sizeof(pbrhip_ray)) || hipMalloc(&d_out, 4096)) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(d_rays, rays.data(), n * sizeof(pbrhip_ray), 1)) throw std::runtime_error("hipMemcpy failed");
    uint32_t* d_ident = static_cast<uint32_t*>(d_out);                                      // 16 K bytes per ray
    uint32_t* d_count = reinterpret_cast<uint32_t*>(static_cast<char*>(d_out) + 2048);      // 4
    std::vector<uint32_t> count(n), ident(4 * n * K), only(n), hcount, hident;
    scene.TraceAllDevice(d_rays, n, K, d_count, d_ident);
    if (hipMemcpy(count.data(), d_count, 4 * n, 2) || hipMemcpy(ident.data(), d_ident, 16 * n * K, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.TraceAllDevice(d_rays, n, 0, d_count, nullptr);  // the count alone
    if (hipMemcpy(only.data(), d_count, 4 * n, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.TraceAll(rays, K, &hcount, &hident);
    hipFree(d_rays), hipFree(d_out);
    if (hcount != count || hident != ident || only != count) return 2;  // host and device variants agree; the count does not depend on K
    // what the geometry says: ray 0 meets the quad at t = 3 and both walls at t = 5 (3 hits, the first two listed), ray 1 the two walls
    // at one t, the first wall -- the smaller id -- first; rays 2 and 4 nothing; ray 3 the quad alone
    if (count[0] != 3 || count[1] != 2 || count[2] != 0 || count[3] != 1 || count[4] != 0) return 2;
    if (ident[3] != bits(3.0f) || ident[7] != bits(5.0f) || ident[8 + 3] != bits(5.0f) || ident[8 + 7] != bits(5.0f) || ident[8] == ident[12]) return 2;
    if (ident[16] != PBRHIP_NONE || ident[20] != PBRHIP_NONE || ident[24] == PBRHIP_NONE || ident[28] != PBRHIP_NONE || ident[32] != PBRHIP_NONE) return 2;
    const std::vector<uint32_t> inst = scene.ObjectIds(ident, PBRHIP_ID_INSTANCE);
    if (inst.size() != n * K || inst[0] != 0 || inst[1] != 1 || inst[2] != 1 || inst[3] != 2 || inst[4] != PBRHIP_NONE) return 2;
    for (size_t i = 0; i < n; i++) {
      printf("A %zu %08x |", i, count[i]);
      for (size_t w = 0; w < 4 * K; w++) printf(" %08x", ident[4 * K * i + w]);
      printf("\n");
    }
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
