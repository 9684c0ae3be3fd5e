// A C++ caller of pbrlab::Scene::ObjectIds, SvgfAccumulate and SvgfFilter (include/pbrlab_hip.hpp): shim_temporal.cc's emitting quad, which
// moves one world unit to the right between two frames under a fixed look-at camera, and a second quad behind it with another instance id:
// snapshot -> edit -> refit -> render -> features -> motion -> ids -> accumulate -> filter.
// Exit code 0 = done, 3 = no HIP device (expected on a CPU box), 2 = a result that breaks the contract.
#include <cmath>
#include <cstdio>

#include "pbrlab_hip.hpp"

int main() {
  try {
    pbrlab::Scene scene;
    pbrlab::CyclesPrincipledBsdfParameter grey;
    grey.base_color = pbrlab::float3(0.25f);
    const uint32_t mat = scene.AddMaterialParam(grey);
    const float I[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    uint32_t inst[2];
    for (int k = 0; k < 2; k++) {  // the quad at z = 0 and a wall of the same material at z = -2, both facing +z
      auto attr = std::make_shared<pbrlab::Attribute>();
      const float r = k ? 8.0f : 1.0f, z = k ? -2.0f : 0.0f;  // (the wall fills the frame)
      attr->vertices = {-r, -r, z, 1, r, -r, z, 1, r, r, z, 1, -r, r, z, 1};
      const pbrlab::MeshPtr quad = scene.AddTriangleMesh(k ? "wall" : "light", attr, std::vector<uint32_t>{0, 1, 2, 0, 2, 3}, std::vector<uint32_t>{},
                                                         std::vector<uint32_t>{}, std::vector<uint32_t>{mat, mat});
      const uint32_t ls = scene.CreateLocalScene();
      scene.AddMeshToLocalScene(ls, quad);
      inst[k] = scene.CreateInstance(ls, I);
    }
    pbrlab::AreaLightParameter lp;
    lp.emission = pbrlab::float3(2.0f);
    const uint32_t lid = scene.AddLightParam(lp);
    scene.AttachLightParamIdsToInstance(inst[0], {{lid, lid}});
    scene.CommitScene();
    const float eye[3] = {0, 0, 4}, lookat[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    scene.SetCamera(eye, lookat, up, 90.0f);
    const uint32_t W = 16, H = 16, spp = 4;
    std::atomic_bool cancel(false);
    std::atomic_size_t finish(0);
    pbrlab::MotionLayer m;
    pbrlab::RenderLayer layer;
    pbrlab::FeatureLayer feat;
    // frame 0: no history
    scene.SnapshotPose();
    pbrlab::Render(scene, W, H, spp, cancel, &layer, &finish);
    pbrlab::RenderFeatures(scene, W, H, spp, &feat);
    pbrlab::RenderMotion(scene, W, H, &m);
    const std::vector<uint32_t> ids0 = scene.ObjectIds(m.ident);
    const size_t centre = 8 * W + 8, corner = 0;
    if (ids0.size() != size_t(W) * H || ids0[centre] != inst[0] || ids0[corner] != inst[1]) return 2;
    if (scene.ObjectIds(m.ident, PBRHIP_ID_GEOM).size() != ids0.size()) return 2;
    const pbrlab::SvgfHistory h0 = pbrlab::SvgfAccumulate(layer, m, nullptr, &feat, &ids0);
    if (h0.illum[4 * centre + 3] != 1.0f || h0.var[centre] != 0.0f || h0.ids != ids0) return 2;
    if (std::fabs(h0.illum[4 * centre] - 2.0f / 0.25f) > 1e-3f) return 2;  // the emitter's radiance over its albedo
    // frame 1: the quad one unit to the right = two pixels
    scene.SnapshotPose();
    const float T[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {1, 0, 0, 1}};
    scene.UpdateInstanceTransform(inst[0], T);
    scene.RefitScene();
    pbrlab::Render(scene, W, H, spp, cancel, &layer, &finish);
    pbrlab::RenderFeatures(scene, W, H, spp, &feat);
    pbrlab::RenderMotion(scene, W, H, &m);
    const std::vector<uint32_t> ids1 = scene.ObjectIds(m.ident);
    const size_t p = 8 * W + 9;
    if (ids1[p] != inst[0]) return 2;
    const pbrlab::SvgfHistory h1 = pbrlab::SvgfAccumulate(layer, m, &h0, &feat, &ids1);
    if (h1.illum[4 * p + 3] != 2.0f || !(h1.var[p] >= 0.0f)) return 2;  // two frames of the emitter seen head-on
    pbrlab::SvgfHistory fed;
    const std::vector<float> out = pbrlab::SvgfFilter(h1, &feat, &fed);
    if (out.size() != size_t(W) * H * 4 || out[4 * p + 3] != 1.0f || std::fabs(out[4 * p] - 2.0f) > 1e-2f) return 2;
    if (fed.illum.size() != out.size() || fed.illum[4 * p + 3] != 2.0f || fed.var != h1.var || fed.ids != ids1) return 2;
    bool refused = false;
    try {
      pbrlab::SvgfFilterOptions bad;
      bad.iterations = 9;
      pbrlab::SvgfFilter(h1, &feat, nullptr, bad);
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused) return 2;
    printf("shim ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
