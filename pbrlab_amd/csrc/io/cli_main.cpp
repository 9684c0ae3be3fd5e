// pbrlab-hip-cli -- pbrlab-cli (pc/pbrlab-cli.cc:16-60) on the MI355X path tracer.
//
//   pbrlab-hip-cli scene.obj [more.obj ...] [strands.hair ...] [--width W] [--height H] [--spp N] [--out FILE.png]
//                  [--gpus N] [--bvh host|gpu|gpu-wide] [--env FILE [--env-scale S]]
//                  [--eye X,Y,Z --lookat X,Y,Z [--up X,Y,Z] [--fov DEG] [--lens-radius R] [--focus D]]
//                  [--aov PREFIX] [--denoise] [--feature-spp N] [--split-emission] [--adaptive THRESHOLD [--min-spp N]]
//                  [--projection latlong|fisheye|ortho [--ortho-height H]]
//
// Without options it does what the reference binary does: 512 x 512, 32 samples per pixel, "rgba.png" in the current
// directory = sRGB(rgba / count) quantised as byte(x * 256).  --gpus N deals 16 x 16 pixel blocks to N ranks, rank g on
// GPU g % (GPUs present): one host thread per rank, the scene is ingested once and copied device-to-device, the shards
// are gathered on the first GPU over xGMI inside the library (pbrhip_render_multi).  --bvh gpu builds the acceleration structure
// on the GPU (faster commit, slightly slower traversal, same image); --bvh gpu-wide also collapses that tree
// on the GPU into the 4-wide quantised tree the production kernels read.  --env FILE lights the scene with a lat-long environment map
// (.hdr, .exr or any LDR format pbrio_image_load reads), times --env-scale (default 1).  --eye / --lookat replace
// the reference's camera with a look-at camera: --up (default 0,1,0), vertical --fov in degrees (default 30), a thin
// lens of --lens-radius (default 0: a pinhole) focused at --focus along the view direction (default 0: |lookat - eye|).
// --aov PREFIX writes the first-hit features: PREFIX.albedo.png (mean albedo, sRGB like the image), PREFIX.normal.png
// (0.5 N + 0.5, linear) and PREFIX.depth.png ((z - z_min) / (z_max - z_min) over the covered pixels, background 1).  --denoise filters the
// frame with the edge-avoiding A-trous filter before it is written.  Both use the features of the first --feature-spp passes (default:
// min(spp, 16)), rendered on the first GPU.  --split-emission (with --aov or --denoise) renders the first-hit emission
// layer of all --spp passes beside the features: --denoise then filters only the reflected light (the albedo counts a miss and an
// emitter as black) and adds the emission back, and --aov also writes PREFIX.emission.png (the mean emission, sRGB like the image).
// Not with --adaptive.  Without the flag every command line writes what it wrote before.
// --adaptive THRESHOLD renders with adaptive sampling: --spp is then the MAXIMUM per pixel, 8 x 8 tiles whose error
// estimate has fallen to THRESHOLD stop early (0 = the library's default), and --min-spp N is the first level (default 8; every pixel
// holds at least twice that, or --spp).  The image is rgba / count with each pixel's own count; --denoise works on the result.  One GPU.
// --projection replaces the --eye / --lookat camera's perspective projection: latlong = a 360 degree panorama with the
// image centre along the view direction, fisheye = equidistant with --fov (up to 360) across the image height and black corners, ortho =
// parallel rays over a view --ortho-height world units high.  One GPU; not with --adaptive, --aov or --denoise.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "pbrhip_io.h"
#include "pbrlab_hip.hpp"

int main(int argc, char** argv) {
  size_t width = 512, height = 512, samples = 32;  // pbrlab-cli.cc:36-38
  int gpus = 1, bvh = PBRHIP_BVH_HOST_SAH;
  std::string out = "rgba.png";
  const char* env = nullptr;
  float env_scale = 1.0f;
  bool have_eye = false, have_lookat = false;
  float eye[3] = {0, 0, 0}, lookat[3] = {0, 0, 0}, up[3] = {0, 1, 0}, fov = 30.0f, lens_radius = 0.0f, focus = 0.0f;
  const char* aov = nullptr;
  bool denoise = false, split_emission = false;
  size_t feature_spp = 0, min_spp = 0;
  bool adaptive = false;
  float adaptive_threshold = PBRHIP_ADAPTIVE_THRESHOLD;
  int projection = -1;  // pbrlab::Projection, or none
  float ortho_height = 0.0f;
  std::vector<const char*> files;
  files.push_back(argv[0]);
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto value = [&](const char* name) -> const char* {
      if (i + 1 >= argc) {
        std::cerr << "missing value for " << name << std::endl;
        exit(EXIT_FAILURE);
      }
      return argv[++i];
    };
    // a positive integer that fits the library's uint32_t fields
    auto number = [&](const char* name, unsigned long max) -> size_t {
      const char* v = value(name);
      char* end = nullptr;
      errno = 0;
      const unsigned long n = strtoul(v, &end, 10);
      if (errno || end == v || *end || v[0] == '-' || n == 0 || n > max) {
        std::cerr << name << " needs an integer in 1.." << max << ", got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
      return size_t(n);
    };
    if (a == "--width") width = number("--width", 0xFFFFFFFFul);
    else if (a == "--height") height = number("--height", 0xFFFFFFFFul);
    else if (a == "--spp") samples = number("--spp", 0xFFFFFFFFul);
    else if (a == "--out") out = value("--out");
    else if (a == "--gpus") gpus = int(number("--gpus", 1024));
    else if (a == "--bvh") {
      const std::string b = value("--bvh");
      bvh = b == "gpu-wide" ? PBRHIP_BVH_GPU_LBVH_WIDE : (b == "gpu" ? PBRHIP_BVH_GPU_LBVH : PBRHIP_BVH_HOST_SAH);
    }
    else if (a == "--env") env = value("--env");
    else if (a == "--aov") aov = value("--aov");
    else if (a == "--denoise") denoise = true;
    else if (a == "--split-emission") split_emission = true;
    else if (a == "--feature-spp") feature_spp = number("--feature-spp", 0xFFFFFFFFul);
    else if (a == "--min-spp") min_spp = number("--min-spp", 0xFFFFFFFFul);
    else if (a == "--adaptive") {
      const char* v = value("--adaptive");
      char* end = nullptr;
      const float x = strtof(v, &end);
      if (end == v || *end || !(x >= 0.0f) || x > 3.0e38f) {
        std::cerr << "--adaptive needs a finite threshold >= 0 (0: the default), got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
      adaptive = true;
      if (x > 0.0f) adaptive_threshold = x;
    }
    else if (a == "--projection") {
      const std::string v = value("--projection");
      projection = v == "latlong" ? int(pbrlab::kProjectionLatLong) : v == "fisheye" ? int(pbrlab::kProjectionFisheye) : v == "ortho" ? int(pbrlab::kProjectionOrtho) : -1;
      if (projection < 0) {
        std::cerr << "--projection needs latlong, fisheye or ortho, got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
    }
    else if (a == "--ortho-height") {
      const char* v = value("--ortho-height");
      char* end = nullptr;
      ortho_height = strtof(v, &end);
      if (end == v || *end || !(ortho_height > 0.0f) || ortho_height > 3.0e38f) {
        std::cerr << "--ortho-height needs a finite number > 0, got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
    }
    else if (a == "--env-scale") {
      const char* v = value("--env-scale");
      char* end = nullptr;
      env_scale = strtof(v, &end);
      if (end == v || *end || !(env_scale >= 0.0f) || env_scale > 3.0e38f) {
        std::cerr << "--env-scale needs a finite number >= 0, got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
    }
    else if (a == "--eye" || a == "--lookat" || a == "--up") {  // X,Y,Z
      const char* v = value(a.c_str());
      float* dst = a == "--eye" ? eye : a == "--lookat" ? lookat : up;
      const char* p = v;
      bool ok = true;
      for (int k = 0; k < 3 && ok; ++k) {
        char* end = nullptr;
        dst[k] = strtof(p, &end);
        ok = end != p && std::isfinite(dst[k]) && (k < 2 ? *end == ',' : *end == '\0');
        p = end + 1;
      }
      if (!ok) {
        std::cerr << a << " needs three finite numbers X,Y,Z, got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
      if (a == "--eye") have_eye = true;
      if (a == "--lookat") have_lookat = true;
    }
    else if (a == "--fov" || a == "--lens-radius" || a == "--focus") {
      const char* v = value(a.c_str());
      char* end = nullptr;
      const float x = strtof(v, &end);
      if (end == v || *end || !std::isfinite(x)) {
        std::cerr << a << " needs a finite number, got '" << v << "'" << std::endl;
        exit(EXIT_FAILURE);
      }
      if (a == "--fov") fov = x;
      else if (a == "--lens-radius") lens_radius = x;
      else focus = x;
    }
    else files.push_back(argv[i]);
  }
  if (have_eye != have_lookat) {
    std::cerr << (have_eye ? "--eye needs --lookat" : "--lookat needs --eye") << std::endl;
    return EXIT_FAILURE;
  }
  if (feature_spp && !aov && !denoise) {
    std::cerr << "--feature-spp needs --aov or --denoise" << std::endl;
    return EXIT_FAILURE;
  }
  if (split_emission && ((!aov && !denoise) || adaptive)) {
    std::cerr << "--split-emission needs --aov or --denoise, and a fixed sample count (no --adaptive)" << std::endl;
    return EXIT_FAILURE;
  }
  if (min_spp && !adaptive) {
    std::cerr << "--min-spp needs --adaptive" << std::endl;
    return EXIT_FAILURE;
  }
  if (adaptive && gpus != 1) {
    std::cerr << "--adaptive renders on one GPU (--gpus 1)" << std::endl;
    return EXIT_FAILURE;
  }
  if (projection >= 0 && !have_eye) {
    std::cerr << "--projection needs --eye and --lookat" << std::endl;
    return EXIT_FAILURE;
  }
  if (projection >= 0 && (adaptive || aov || denoise || gpus != 1)) {
    std::cerr << "--projection renders on one GPU, without --adaptive, --aov or --denoise" << std::endl;
    return EXIT_FAILURE;
  }
  if ((projection == int(pbrlab::kProjectionOrtho)) != (ortho_height > 0.0f)) {
    std::cerr << (ortho_height > 0.0f ? "--ortho-height needs --projection ortho" : "--projection ortho needs --ortho-height") << std::endl;
    return EXIT_FAILURE;
  }
  if (projection == int(pbrlab::kProjectionFisheye) && !(fov > 0.0f && fov <= 360.0f)) {
    std::cerr << "--projection fisheye needs --fov in (0, 360]" << std::endl;
    return EXIT_FAILURE;
  }
  if (files.size() < 2) {
    std::cerr << "not specified obj filename" << std::endl;
    return EXIT_FAILURE;
  }
  if (uint64_t(width) * uint64_t(height) >= (1ull << 32)) {
    std::cerr << "width x height must stay below 2^32 pixels" << std::endl;
    return EXIT_FAILURE;
  }
  int ndev = 0;
  if (pbrhip_device_count(&ndev) != PBRHIP_OK || ndev < 1) {
    std::cerr << "no HIP device: " << pbrhip_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  // the scene is ingested and its BVH built once; the other GPUs get device-to-device copies
  pbrlab::RenderLayer layer;
  pbrlab::Scene scene;
  pbrhip_scene_set_bvh_builder(scene.handle(), bvh);
  if (pbrio_create_scene(int(files.size()), files.data(), scene.handle()) != PBRHIP_OK) {
    std::cerr << "scene: " << pbrio_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  if (env) {  // the map as RGB (one channel: grey; two: grey + alpha, alpha dropped; four: alpha dropped)
    float* px = nullptr;
    size_t w = 0, h = 0, c = 0;
    const std::string path(env);
    const size_t cut = path.find_last_of('/');
    const std::string edir = cut == std::string::npos ? "./" : path.substr(0, cut + 1);
    const std::string ename = cut == std::string::npos ? path : path.substr(cut + 1);
    if (pbrio_image_load(ename.c_str(), edir.c_str(), &px, &w, &h, &c) != PBRHIP_OK) {
      std::cerr << "--env: " << pbrio_last_error() << std::endl;
      return EXIT_FAILURE;
    }
    std::vector<float> rgb(w * h * 3);
    for (size_t i = 0; i < w * h; ++i)
      for (size_t k = 0; k < 3; ++k) rgb[3 * i + k] = px[c * i + (c >= 3 ? k : 0)];
    pbrio_free(px);
    try {
      scene.SetEnvironment(rgb.data(), uint32_t(w), uint32_t(h), env_scale);
    } catch (const std::exception& e) {
      std::cerr << "--env: " << e.what() << std::endl;
      return EXIT_FAILURE;
    }
  }
  if (have_eye) {
    try {
      // (a projection takes the frame alone: a fisheye's field of view goes to it, beyond what a perspective camera accepts)
      scene.SetCamera(eye, lookat, up, projection >= 0 ? 30.0f : fov, lens_radius, focus);
    } catch (const std::exception& e) {
      std::cerr << "camera: " << e.what() << std::endl;
      return EXIT_FAILURE;
    }
  }
  std::atomic_bool cancel_render_flag(false);
  std::atomic_size_t finish_pass(0);
  if (adaptive) {
    try {
      pbrlab::AdaptiveOptions o;
      o.threshold = adaptive_threshold, o.first_level = uint32_t(min_spp);
      const pbrlab::AdaptiveResult r = pbrlab::RenderAdaptive(scene, uint32_t(width), uint32_t(height), uint32_t(samples), cancel_render_flag, &layer, &finish_pass, o);
      std::cerr << "adaptive: " << r.samples << " samples (" << double(r.samples) / double(width * height) << " per pixel, at most " << samples << ") in "
                << r.rounds << " rounds" << std::endl;
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return EXIT_FAILURE;
    }
  } else if (projection >= 0) {
    try {
      const float param = projection == int(pbrlab::kProjectionOrtho) ? 0.5f * ortho_height : projection == int(pbrlab::kProjectionFisheye) ? fov : 0.0f;
      pbrlab::RenderProjection(scene, pbrlab::Projection(projection), param, uint32_t(width), uint32_t(height), uint32_t(samples), cancel_render_flag, &layer,
                               &finish_pass);
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return EXIT_FAILURE;
    }
  } else if (gpus == 1) {
    if (!pbrlab::Render(scene, uint32_t(width), uint32_t(height), uint32_t(samples), cancel_render_flag, &layer, &finish_pass))
      return EXIT_FAILURE;
  } else {
    std::vector<std::unique_ptr<pbrlab::Scene>> replicas;
    std::vector<const pbrlab::Scene*> scenes{&scene};
    try {
      for (int g = 1; g < gpus; ++g) {  // rank g renders on GPU g % ndev
        replicas.push_back(scene.Replicate(g % ndev));
        scenes.push_back(replicas.back().get());
      }
    } catch (const std::exception& e) {
      std::cerr << "scene copy: " << e.what() << std::endl;
      return EXIT_FAILURE;
    }
    if (!pbrlab::Render(scenes, uint32_t(width), uint32_t(height), uint32_t(samples), cancel_render_flag, &layer, &finish_pass))
      return EXIT_FAILURE;
  }

  // a path as WritePNG takes it: directory (with the slash) + file name
  auto split = [](const std::string& path, std::string* dir, std::string* name) {
    const size_t slash = path.find_last_of('/');
    *dir = slash == std::string::npos ? "./" : path.substr(0, slash + 1);
    *name = slash == std::string::npos ? path : path.substr(slash + 1);
  };
  std::string dir, name;
  const size_t npx = width * height;
  if (aov || denoise) {
    pbrlab::FeatureLayer feat;
    pbrlab::EmissionLayer emission;
    const std::vector<uint32_t> ones(npx, 1u), samples_taken = layer.count;
    const uint32_t fspp = uint32_t(std::min<size_t>(samples, feature_spp ? feature_spp : 16));
    try {
      if (split_emission) {
        // the features of the first passes, the emission of all of them: the rest of the passes continues the emission sums alone
        pbrlab::RenderFeaturesEmission(scene, uint32_t(width), uint32_t(height), fspp, &feat, &emission);
        if (fspp < samples) {
          pbrhip_render_desc d = {};
          d.width = uint32_t(width), d.height = uint32_t(height), d.num_sample = uint32_t(samples) - fspp, d.first_pass = fspp;
          d.seed_seq = 1234567890, d.tile_world = 1, d.flags = PBRHIP_RENDER_NO_CLEAR;
          if (pbrhip_render_features_emission(scene.handle(), &d, nullptr, nullptr, nullptr, emission.emission.data()) != PBRHIP_OK)
            throw std::runtime_error(std::string("--split-emission: ") + pbrhip_last_error());
        }
      } else {
        pbrlab::RenderFeatures(scene, uint32_t(width), uint32_t(height), uint32_t(feature_spp ? feature_spp : std::min<size_t>(samples, 16)), &feat);
      }
      if (denoise && split_emission) {  // filter the reflected light, add the emission back
        pbrlab::FeatureLayer black;
        pbrlab::SplitEmission(layer, emission, &feat, &layer, &black);
        layer.rgba = pbrlab::MergeEmission(pbrlab::Denoise(layer, &black), emission, samples_taken);
        layer.count = ones;
      } else if (denoise) {  // the mean colour takes the layer's place: sum = mean, count = 1
        layer.rgba = pbrlab::Denoise(layer, &feat);
        layer.count = ones;
      }
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return EXIT_FAILURE;
    }
    if (aov) {
      std::vector<float> albedo(npx * 4, 1.0f);
      std::vector<uint8_t> normal(npx * 3), depth(npx * 3);
      auto byte = [](float x) { return uint8_t(std::min(255.0f, std::max(0.0f, x * 256.0f))); };
      float zmin = INFINITY, zmax = -INFINITY;
      for (size_t i = 0; i < npx; ++i)
        if (feat.albedo[4 * i + 3] > 0.0f) {
          const float z = feat.normal_depth[4 * i + 3] / feat.albedo[4 * i + 3];
          zmin = std::min(zmin, z), zmax = std::max(zmax, z);
        }
      for (size_t i = 0; i < npx; ++i) {
        const float m = float(feat.count[i]), k = feat.albedo[4 * i + 3];
        const float* nd = &feat.normal_depth[4 * i];
        const float len = std::sqrt(nd[0] * nd[0] + nd[1] * nd[1] + nd[2] * nd[2]);
        for (size_t c = 0; c < 3; ++c) {
          if (m > 0.0f) albedo[4 * i + c] = (feat.albedo[4 * i + c] + (m - k)) / m;  // a miss counts as white
          normal[3 * i + c] = byte(len > 0.0f ? 0.5f * nd[c] / len + 0.5f : 0.5f);
          depth[3 * i + c] = byte(k > 0.0f && zmax > zmin ? (nd[3] / k - zmin) / (zmax - zmin) : (k > 0.0f ? 0.0f : 1.0f));
        }
      }
      split(std::string(aov) + ".albedo.png", &dir, &name);
      int rc = pbrio_write_layer_png(name.c_str(), dir.c_str(), albedo.data(), ones.data(), width, height);
      split(std::string(aov) + ".normal.png", &dir, &name);
      if (rc == PBRHIP_OK) rc = pbrio_write_png_u8(name.c_str(), dir.c_str(), normal.data(), width, height, 3);
      split(std::string(aov) + ".depth.png", &dir, &name);
      if (rc == PBRHIP_OK) rc = pbrio_write_png_u8(name.c_str(), dir.c_str(), depth.data(), width, height, 3);
      if (split_emission) {  // the emission sums over the samples taken
        split(std::string(aov) + ".emission.png", &dir, &name);
        if (rc == PBRHIP_OK) rc = pbrio_write_layer_png(name.c_str(), dir.c_str(), emission.emission.data(), samples_taken.data(), width, height);
      }
      if (rc != PBRHIP_OK) {
        std::cerr << "--aov: " << pbrio_last_error() << std::endl;
        return EXIT_FAILURE;
      }
    }
  }
  split(out, &dir, &name);
  if (pbrio_write_layer_png(name.c_str(), dir.c_str(), layer.rgba.data(), layer.count.data(), width, height) != PBRHIP_OK) {
    std::cerr << pbrio_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
