// A C++ caller of pbrlab::RenderRays, RenderFeaturesRays, ProjectionRays and RenderProjection (include/pbrlab_hip.hpp): an emitting quad
// seen along rays of the caller's own and through an orthographic view.  Exit code 0 = done, 3 = no HIP device (expected on a CPU box),
// 2 = a result that breaks the contract.
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
    // 8 x 4 parallel rays down the z axis over [-2, 2] x [-1, 1]: the quad covers x in [-1, 1]; the last ray is inactive
    const uint32_t W = 8, H = 4, spp = 4;
    std::vector<pbrhip_ray> rays(W * H);
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x) {
        pbrhip_ray& r = rays[y * W + x];
        r.org[0] = -2.0f + 4.0f * (float(x) + 0.5f) / float(W), r.org[1] = 1.0f - 2.0f * (float(y) + 0.5f) / float(H), r.org[2] = 3.0f;
        r.dir[0] = 0.0f, r.dir[1] = 0.0f, r.dir[2] = -1.0f;
        r.tmin = 0.0f, r.tmax = 1e30f;
      }
    rays.back().dir[2] = NAN;
    pbrlab::RenderLayer layer;
    pbrlab::RenderRays(scene, W, H, spp, rays, cancel, &layer);
    for (uint32_t i = 0; i < W * H; ++i) {
      const uint32_t x = i % W;
      const bool lit = x >= 2 && x < 6 && i + 1 != W * H;
      if (layer.count[i] != spp || layer.rgba[4 * i + 3] != float(spp)) return 2;
      if (lit ? !(layer.rgba[4 * i] >= 2.0f * spp) : layer.rgba[4 * i] != 0.0f) return 2;  // the emitter seen head-on, or nothing
    }
    pbrlab::FeatureLayer feat;
    pbrlab::RenderFeaturesRays(scene, W, H, spp, rays, &feat);
    if (feat.count[0] != spp || feat.albedo[4 * 2 + 3] != float(spp) || std::fabs(feat.normal_depth[4 * 2 + 3] - 3.0f * spp) > 1e-4f || feat.albedo[3] != 0.0f) return 2;
    // the same view as an orthographic projection about a look-at frame
    const float eye[3] = {0, 0, 3}, lookat[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    scene.SetCamera(eye, lookat, up);
    const std::vector<pbrhip_ray> pr = pbrlab::ProjectionRays(scene, pbrlab::kProjectionOrtho, 1.0f, W, H, 0, 2);
    if (pr.size() != size_t(2) * W * H || pr[0].dir[2] != -1.0f || !(pr[0].org[0] < -1.5f) || pr[0].org[2] != 3.0f) return 2;
    pbrlab::RenderProjection(scene, pbrlab::kProjectionOrtho, 1.0f, W, H, spp, cancel, &layer);
    if (layer.count[W + 3] != spp || !(layer.rgba[4 * (W + 3)] >= 2.0f * spp) || layer.rgba[0] != 0.0f) return 2;
    printf("rays ok\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "shim: %s\n", e.what());
    return 3;
  }
}
