// A C++ caller of Scene::SetCamera / ResetCamera (include/pbrlab_hip.hpp): a lit quad seen by the reference's camera, by a look-at
// pinhole and by a thin lens.  Exit code 0 = rendered, 3 = no HIP device (expected on a CPU box), 2 = a bad camera was accepted.
#include <cmath>
#include <cstdio>

#include "pbrlab_hip.hpp"

int main() {
  try {
    pbrlab::Scene scene;
    auto attr = std::make_shared<pbrlab::Attribute>();
    attr->vertices = {-1, -1, 0, 1, 1, -1, 0, 1, 1, 1, 0, 1, -1, 1, 0, 1};  // z = 0, facing +z
    pbrlab::CyclesPrincipledBsdfParameter black;
    black.base_color = pbrlab::float3(0.0f);
    const uint32_t mat = scene.AddMaterialParam(black);
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
    const float eye[3] = {0.5f, 0.5f, 4.0f}, at[3] = {0.5f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    scene.SetCamera(eye, at, up, 20.0f);  // before the commit
    scene.CommitScene();
    bool threw = false;
    try {
      scene.SetCamera(eye, eye, up);  // eye == lookat
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 2;
    std::atomic_bool cancel(false);
    std::atomic_size_t fin(0);
    double sums[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
      if (k == 1) scene.SetCamera(eye, at, up, 20.0f, 0.2f, 4.0f);
      if (k == 2) scene.ResetCamera();
      pbrlab::RenderLayer layer;
      if (!pbrlab::Render(scene, 32, 32, 2, cancel, &layer, &fin)) return 11;
      for (size_t i = 0; i < layer.rgba.size(); i += 4) sums[k] += layer.rgba[i];
      if (!(sums[k] > 0) || !std::isfinite(sums[k])) return 12 + k;
    }
    // the look-at camera centred on (0.5, 0.5) sees the quad's corner region; the reference's camera sees the whole quad
    printf("camera ok: %f %f %f\n", sums[0], sums[1], sums[2]);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
