// A C++ caller of pbrlab::RenderAdaptive (include/pbrlab_hip.hpp): an emitting quad in front of nothing, seen by the reference's
// camera.  Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = a result that breaks the contract.
#include <cstdio>

#include "pbrlab_hip.hpp"

int main() {
  try {
    pbrlab::Scene scene;
    auto attr = std::make_shared<pbrlab::Attribute>();
    attr->vertices = {-1, -1, 0, 1, 1, -1, 0, 1, 1, 1, 0, 1, -1, 1, 0, 1};  // z = 0, facing +z
    pbrlab::CyclesPrincipledBsdfParameter grey;
    grey.base_color = pbrlab::float3(0.25f);
    const uint32_t mat = scene.AddMaterialParam(grey);
    const float I[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    const pbrlab::MeshPtr quad = scene.AddTriangleMesh("light", attr, std::vector<uint32_t>{0, 1, 2, 0, 2, 3}, std::vector<uint32_t>{},
                                                       std::vector<uint32_t>{}, std::vector<uint32_t>{mat, mat});
    const uint32_t ls = scene.CreateLocalScene();
    scene.AddMeshToLocalScene(ls, quad);
    const uint32_t inst = scene.CreateInstance(ls, I);
    pbrlab::AreaLightParameter lp;
    lp.emission = pbrlab::float3(2.0f);
    const uint32_t lid = scene.AddLightParam(lp);
    scene.AttachLightParamIdsToInstance(inst, {{lid, lid}});
    scene.CommitScene();
    std::atomic_bool cancel(false);
    std::atomic_size_t fin(0);
    pbrlab::RenderLayer layer;
    pbrlab::AdaptiveOptions o;
    o.first_level = 2;
    const pbrlab::AdaptiveResult r = pbrlab::RenderAdaptive(scene, 36, 20, 16, cancel, &layer, &fin, o);
    uint64_t sum = 0;
    for (const uint32_t c : layer.count) {
      if (c != 4 && c != 8 && c != 16) return 2;  // every pixel holds a level, and at least two of them
      sum += c;
    }
    if (sum != r.samples || r.rounds < 2 || r.rounds > 4 || r.tile_error.size() != 5 * 3 || fin.load() < 4) return 2;
    printf("adaptive ok: %llu samples in %u rounds\n", (unsigned long long)r.samples, r.rounds);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
