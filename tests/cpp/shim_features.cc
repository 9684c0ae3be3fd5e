// A C++ caller of pbrlab::RenderFeatures / pbrlab::Denoise (include/pbrlab_hip.hpp): a quad seen by the reference's camera -- its
// features, then the denoised frame.  Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = wrong features.
#include <cmath>
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
    if (!pbrlab::Render(scene, 32, 32, 4, cancel, &layer, &fin)) return 11;
    pbrlab::FeatureLayer feat;
    pbrlab::RenderFeatures(scene, 32, 32, 2, &feat);
    pbrlab::RenderFeatures(scene, 32, 32, 2, &feat, 2, true);  // passes 2, 3 on top
    const size_t c = (16 * 32 + 16) * 4;
    if (feat.count[16 * 32 + 16] != 4 || feat.albedo[c + 3] != 4.0f || feat.albedo[c] != 1.0f || feat.normal_depth[c + 2] != 4.0f) return 2;
    pbrlab::DenoiseOptions o;
    o.iterations = 3;
    const std::vector<float> out = pbrlab::Denoise(layer, &feat, o);
    if (out.size() != 32 * 32 * 4 || out[c + 3] != 1.0f || !std::isfinite(out[c])) return 2;
    printf("features ok: %f\n", out[c]);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
