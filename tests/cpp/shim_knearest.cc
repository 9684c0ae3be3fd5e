// A C++ caller of pbrlab::Scene::KNearest and KNearestDevice (include/pbrlab_hip.hpp): tests/cpp/shim_allhits.cc's scene -- a unit quad at
// z = 0 in front of two coinciding walls at z = -2, so that a point on the walls has two primitives at one distance.  Points go to device
// memory through the HIP runtime the library links (three of its functions, declared here: the caller needs no HIP headers); counts and
// rows are printed as hexadecimal words, one query per line, for tests/test_knearest_shim.py to compare with the Python binding's.
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
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // queries: above the quad without a bound (all six triangles), the same with a radius that holds the quad alone, beside the quad
    // above the walls, an inactive one (a NaN coordinate), one with nothing in reach, one ON the walls with max_dist = 0
    const std::vector<pbrhip_point> points = {{{0.25f, 0.5f, 1.0f}, inf},  {{0.25f, 0.5f, 1.0f}, 1.5f}, {{3.0f, 0.5f, 1.0f}, 3.5f},
                                              {{0.25f, nan, 1.0f}, inf},   {{0.0f, 0.0f, -5.0f}, 1.0f}, {{3.0f, 0.5f, -2.0f}, 0.0f}};
    const size_t n = points.size();
    const uint32_t K = 2;
    void *d_points = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_points, n * sizeof(pbrhip_point)) || hipMalloc(&d_out, 4096)) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(d_points, points.data(), n * sizeof(pbrhip_point), 1)) throw std::runtime_error("hipMemcpy failed");
    uint32_t* d_ident = static_cast<uint32_t*>(d_out);                                    // 16 K bytes per query
    float* d_closest = reinterpret_cast<float*>(static_cast<char*>(d_out) + 1024);        // 16 K
    uint32_t* d_count = reinterpret_cast<uint32_t*>(static_cast<char*>(d_out) + 2048);    // 4
    std::vector<uint32_t> count(n), ident(4 * n * K), only(n), list(4 * n * K), hcount, hident;
    std::vector<float> closest(4 * n * K), hclosest;
    scene.KNearestDevice(d_points, n, K, d_count, d_ident, d_closest);
    if (hipMemcpy(count.data(), d_count, 4 * n, 2) || hipMemcpy(ident.data(), d_ident, 16 * n * K, 2) || hipMemcpy(closest.data(), d_closest, 16 * n * K, 2))
      throw std::runtime_error("hipMemcpy failed");
    scene.KNearestDevice(d_points, n, 0, d_count, nullptr, nullptr);  // the count alone
    if (hipMemcpy(only.data(), d_count, 4 * n, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.KNearestDevice(d_points, n, K, nullptr, d_ident, nullptr);  // the list alone
    if (hipMemcpy(list.data(), d_ident, 16 * n * K, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.KNearest(points, K, &hcount, &hident, &hclosest);
    hipFree(d_points), hipFree(d_out);
    // host and device variants agree; neither the count nor the list depends on the other
    if (hcount != count || hident != ident || only != count || list != ident) return 2;
    if (memcmp(hclosest.data(), closest.data(), 16 * n * K)) return 2;
    // what the geometry says: query 0 has all six triangles and the quad's at D2 = 1 first; query 1 the quad's two alone; queries 3 and 4
    // nothing; query 5 the two coinciding wall triangles at distance 0, the first wall -- the smaller id -- first
    if (count[0] != 6 || count[1] != 2 || count[3] != 0 || count[4] != 0 || count[5] != 2) return 2;
    if (ident[3] != bits(1.0f) || closest[3] != 1.0f || closest[0] != 0.25f || closest[1] != 0.5f || closest[2] != 0.0f) return 2;
    if (ident[8 * 3] != PBRHIP_NONE || ident[8 * 3 + 4] != PBRHIP_NONE || ident[8 * 4] != PBRHIP_NONE) return 2;
    if (ident[8 * 5 + 3] != 0u || ident[8 * 5 + 7] != 0u || ident[8 * 5] == ident[8 * 5 + 4]) return 2;
    const std::vector<uint32_t> inst = scene.ObjectIds(ident, PBRHIP_ID_INSTANCE);
    if (inst.size() != n * K || inst[0] != 0 || inst[1] != 0 || inst[6] != PBRHIP_NONE || inst[10] != 1 || inst[11] != 2) return 2;
    for (size_t i = 0; i < n; i++) {
      printf("K %zu %08x |", i, count[i]);
      for (size_t w = 0; w < 4 * K; w++) printf(" %08x", ident[4 * K * i + w]);
      printf(" |");
      for (size_t w = 0; w < 4 * K; w++) printf(" %08x", bits(closest[4 * K * i + w]));
      printf("\n");
    }
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
