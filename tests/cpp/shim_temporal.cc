// A C++ caller of pbrlab::Scene::SnapshotPose, RenderMotion and TemporalAccumulate (include/pbrlab_hip.hpp): an emitting quad that moves
// one world unit to the right between two frames under a fixed look-at camera: snapshot -> edit -> refit -> motion -> accumulate.
// Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = a result that breaks the contract.
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
    // vfov 90 degrees, 4 units away: the image plane at z = 0 is 8 x 8 units, a pixel of the 16 x 16 image half a unit
    const float eye[3] = {0, 0, 4}, lookat[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    scene.SetCamera(eye, lookat, up, 90.0f);
    const uint32_t W = 16, H = 16, spp = 4;
    std::atomic_bool cancel(false);
    std::atomic_size_t finish(0);
    pbrlab::MotionLayer m;
    bool refused = false;
    try {
      pbrlab::RenderMotion(scene, W, H, &m);  // no snapshot yet
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused) return 2;
    pbrlab::RenderLayer layer;
    // frame 0: no history
    scene.SnapshotPose();
    pbrlab::Render(scene, W, H, spp, cancel, &layer, &finish);
    pbrlab::RenderMotion(scene, W, H, &m);
    const pbrlab::TemporalHistory h0 = pbrlab::TemporalAccumulate(layer, m, nullptr);
    const size_t centre = 8 * W + 8;
    if (m.ident[4 * centre] == PBRHIP_NONE || m.motion[4 * centre + 3] != 1.0f || std::fabs(m.motion[4 * centre]) > 1e-3f) return 2;
    if (h0.rgba[4 * centre + 3] != 1.0f || m.ident[0] != PBRHIP_NONE || m.motion[3] != 0.0f) return 2;
    // frame 1: the quad one unit to the right = two pixels; the point under a pixel was two pixels to the left
    scene.SnapshotPose();
    const float T[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {1, 0, 0, 1}};
    scene.UpdateInstanceTransform(inst, T);
    scene.RefitScene();
    pbrlab::Render(scene, W, H, spp, cancel, &layer, &finish);
    pbrlab::RenderMotion(scene, W, H, &m);
    const size_t p = 8 * W + 9;
    if (m.motion[4 * p + 3] != 1.0f || std::fabs(m.motion[4 * p] + 2.0f) > 1e-3f || std::fabs(m.motion[4 * p + 1]) > 1e-3f) return 2;
    if (std::fabs(m.guide[4 * p + 2] - 1.0f) > 1e-6f || !(m.guide[4 * p + 3] > 3.9f)) return 2;
    const pbrlab::TemporalHistory h1 = pbrlab::TemporalAccumulate(layer, m, &h0);
    if (h1.rgba[4 * p + 3] != 2.0f || !(h1.rgba[4 * p] >= 1.999f)) return 2;  // two frames of the emitter seen head-on
    pbrlab::RenderLayer mean;
    h1.Layer(&mean);
    const std::vector<float> den = pbrlab::Denoise(mean, nullptr);
    if (den.size() != size_t(W) * H * 4 || mean.count[p] != 1u || mean.count[0] != 1u) return 2;
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
