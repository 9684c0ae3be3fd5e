// A C++ caller of pbrlab::RenderFeaturesEmission, SplitEmission and MergeEmission (include/pbrlab_hip.hpp): shim_svgf.cc's emitting quad
// in front of a wall under a fixed look-at camera:
// render -> features + emission -> motion -> ids -> split -> accumulate -> filter -> merge, and split -> denoise -> merge.
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
    const size_t centre = 8 * W + 8, corner = 0;
    std::atomic_bool cancel(false);
    std::atomic_size_t finish(0);
    pbrlab::MotionLayer m;
    pbrlab::RenderLayer layer, split;
    pbrlab::FeatureLayer feat, plain, sfeat;
    pbrlab::EmissionLayer em;
    scene.SnapshotPose();
    pbrlab::Render(scene, W, H, spp, cancel, &layer, &finish);
    pbrlab::RenderFeaturesEmission(scene, W, H, spp, &feat, &em);
    pbrlab::RenderFeatures(scene, W, H, spp, &plain);
    if (feat.albedo != plain.albedo || feat.normal_depth != plain.normal_depth || feat.count != plain.count) return 2;
    // the quad's pixels: every sample adds the light's emission; the wall's: none does
    for (int c = 0; c < 3; c++)
      if (em.emission[4 * centre + c] != 2.0f * spp || em.emission[4 * corner + c] != 0.0f) return 2;
    if (em.emission[4 * centre + 3] != float(spp) || em.emission[4 * corner + 3] != 0.0f) return 2;
    // two halves on top of each other are the whole
    pbrlab::FeatureLayer f2;
    pbrlab::EmissionLayer e2;
    pbrlab::RenderFeaturesEmission(scene, W, H, 2, &f2, &e2);
    pbrlab::RenderFeaturesEmission(scene, W, H, 2, &f2, &e2, 2, true);
    if (f2.albedo != feat.albedo || f2.count != feat.count || e2.emission != em.emission) return 2;
    pbrlab::SplitEmission(layer, em, &feat, &split, &sfeat);
    if (split.count != layer.count || sfeat.count != feat.count || sfeat.normal_depth != feat.normal_depth) return 2;
    if (split.rgba[4 * corner] != layer.rgba[4 * corner] || split.rgba[4 * centre + 3] != layer.rgba[4 * centre + 3]) return 2;
    if (!(split.rgba[4 * centre] >= 0.0f) || split.rgba[4 * centre] != std::fmax(layer.rgba[4 * centre] - em.emission[4 * centre], 0.0f)) return 2;
    if (sfeat.albedo[4 * centre + 3] != float(spp) || sfeat.albedo[4 * centre] != feat.albedo[4 * centre]) return 2;
    // a filtered image of nothing + the emission is the emission's mean, exactly
    const std::vector<float> only = pbrlab::MergeEmission(std::vector<float>(size_t(W) * H * 4, 0.0f), em, layer.count);
    if (only[4 * centre] != 2.0f || only[4 * corner] != 0.0f || only[4 * centre + 3] != 0.0f) return 2;
    // split -> accumulate -> filter -> merge
    pbrlab::RenderMotion(scene, W, H, &m);
    const std::vector<uint32_t> ids = scene.ObjectIds(m.ident);
    const pbrlab::SvgfHistory h = pbrlab::SvgfAccumulate(split, m, nullptr, &sfeat, &ids);
    const std::vector<float> out = pbrlab::MergeEmission(pbrlab::SvgfFilter(h, &sfeat), em, layer.count);
    if (out.size() != size_t(W) * H * 4 || out[4 * centre + 3] != 1.0f || !(out[4 * centre] >= 2.0f) || !(out[4 * centre] < 3.0f)) return 2;
    if (!(out[4 * corner] >= 0.0f) || !(out[4 * corner] < 2.0f)) return 2;
    // split -> denoise -> merge
    const std::vector<float> dn = pbrlab::MergeEmission(pbrlab::Denoise(split, &sfeat), em, layer.count);
    if (!(dn[4 * centre] >= 2.0f) || !(dn[4 * centre] < 3.0f) || dn[4 * centre + 3] != 1.0f) return 2;
    // in place
    pbrlab::SplitEmission(layer, em, &feat, &layer, &feat);
    if (layer.rgba != split.rgba || feat.albedo != sfeat.albedo) return 2;
    bool refused = false;
    try {
      pbrlab::EmissionLayer small(8, 8);
      pbrlab::SplitEmission(layer, small, nullptr, &split);
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
