// A C++ caller of pbrlab::Scene::SignedDistance, SignedDistanceDevice, SignedDistanceGridDevice and SignedDistanceInfo
// (include/pbrlab_hip.hpp): a closed box [-1, 1] x [-0.5, 0.5] x [-0.25, 0.25] of 12 triangles.  Points go to device memory through
// the HIP runtime the library links (three of its functions, declared here: the caller needs no HIP headers), the answers come back and
// are printed as hexadecimal words for tests/test_sdf_shim.py to compare with the Python binding's on the same scene.
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
    auto attr = std::make_shared<pbrlab::Attribute>();
    const float x = 1.0f, y = 0.5f, z = 0.25f;
    attr->vertices = {-x, -y, -z, 1, x, -y, -z, 1, x, y, -z, 1, -x, y, -z, 1, -x, -y, z, 1, x, -y, z, 1, x, y, z, 1, -x, y, z, 1};
    const std::vector<uint32_t> faces = {0, 2, 1, 0, 3, 2, 5, 6, 7, 5, 7, 4, 1, 5, 4, 1, 4, 0, 3, 6, 2, 3, 7, 6, 2, 6, 5, 2, 5, 1, 0, 7, 3, 0, 4, 7};  // outward
    const pbrlab::MeshPtr box = scene.AddTriangleMesh("box", attr, faces, std::vector<uint32_t>{}, std::vector<uint32_t>{}, std::vector<uint32_t>(12, mat));
    const uint32_t ls = scene.CreateLocalScene();
    scene.AddMeshToLocalScene(ls, box);
    scene.CreateInstance(ls, I);
    scene.CommitScene();
    const float inf = std::numeric_limits<float>::infinity();
    // points: above the top, the centre, beyond an edge, beyond a corner, inside near a side, one with a bound nothing meets, a NaN
    const std::vector<pbrhip_point> pts = {{{0.25f, 0.125f, 1.25f}, inf}, {{0.0f, 0.0f, 0.0f}, inf},        {{2.0f, 0.0f, 1.25f}, inf},  {{2.0f, 1.5f, 1.25f}, inf},
                                           {{0.5f, 0.375f, 0.0f}, inf},   {{0.25f, 0.125f, 1.25f}, 0.5f}, {{std::nanf(""), 0, 0}, inf}};
    const size_t np = pts.size();
    const pbrhip_sd_info info = scene.SignedDistanceInfo();
    if (info.triangles != 12 || info.vertices != 8 || info.edges_manifold != 18 || info.edges_boundary || info.edges_nonmanifold || info.edges_inconsistent) return 2;
    void *d_pts = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_pts, np * sizeof(pbrhip_point)) || hipMalloc(&d_out, 4096)) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(d_pts, pts.data(), np * sizeof(pbrhip_point), 1)) throw std::runtime_error("hipMemcpy failed");
    uint32_t* d_ident = static_cast<uint32_t*>(d_out);
    float* d_closest = reinterpret_cast<float*>(static_cast<char*>(d_out) + 1024);
    float* d_sd = reinterpret_cast<float*>(static_cast<char*>(d_out) + 2048);
    float* d_grid = reinterpret_cast<float*>(static_cast<char*>(d_out) + 3072);
    std::vector<uint32_t> ident(4 * np), hident;
    std::vector<float> closest(4 * np), sd(4 * np), hclosest, hsd;
    scene.SignedDistanceDevice(d_pts, np, d_ident, d_closest, d_sd);
    if (hipMemcpy(ident.data(), d_ident, 16 * np, 2) || hipMemcpy(closest.data(), d_closest, 16 * np, 2) || hipMemcpy(sd.data(), d_sd, 16 * np, 2)) throw std::runtime_error("hipMemcpy failed");
    scene.SignedDistance(pts, &hident, &hclosest, &hsd);
    const float origin[3] = {-1.5f, -0.75f, 0.0f}, spacing[3] = {1.5f, 0.75f, 0.5f};
    const uint32_t dims[3] = {3, 2, 2};
    std::vector<float> grid(12);
    scene.SignedDistanceGridDevice(origin, spacing, dims, inf, d_grid);
    if (hipMemcpy(grid.data(), d_grid, 4 * grid.size(), 2)) throw std::runtime_error("hipMemcpy failed");
    hipFree(d_pts), hipFree(d_out);
    if (hident != ident || memcmp(hclosest.data(), closest.data(), 16 * np) != 0 || memcmp(hsd.data(), sd.data(), 16 * np) != 0) return 2;  // host and device variants agree
    // what the geometry says: point 0 is 1 above the top (its face normal +z), the centre 0.25 inside, points 5 and 6 miss
    if (sd[3] != 1.0f || sd[0] != 0.0f || sd[1] != 0.0f || sd[2] != 1.0f || closest[2] != 0.25f) return 2;
    if (sd[7] != -0.25f || !(sd[11] > 0.0f) || !(sd[15] > 0.0f) || !(sd[19] < 0.0f)) return 2;
    if (ident[20] != PBRHIP_NONE || ident[24] != PBRHIP_NONE || sd[23] != 0.0f || sd[27] != 0.0f) return 2;
    if (!(grid[0] > 0.0f) || !(grid[1] > 0.0f) || grid[4] != -0.25f || !(grid[6 + 4] > 0.0f)) return 2;  // grid[4]: the centre; grid[10]: 0.25 above the top
    for (size_t i = 0; i < np; i++)
      printf("S %zu %08x %08x %08x %08x | %08x %08x %08x %08x | %08x %08x %08x %08x\n", i, ident[4 * i], ident[4 * i + 1], ident[4 * i + 2], ident[4 * i + 3],
             bits(closest[4 * i]), bits(closest[4 * i + 1]), bits(closest[4 * i + 2]), bits(closest[4 * i + 3]), bits(sd[4 * i]), bits(sd[4 * i + 1]),
             bits(sd[4 * i + 2]), bits(sd[4 * i + 3]));
    printf("G");
    for (float g : grid) printf(" %08x", bits(g));
    printf("\nT %u %u %u %u %u %u\n", info.triangles, info.vertices, info.edges_manifold, info.edges_boundary, info.edges_nonmanifold, info.edges_inconsistent);
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
