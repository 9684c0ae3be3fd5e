// env_tables.cpp -- host tables of the lat-long environment light: radiance, pdf and an alias table over lum * solid angle.
#include "env_tables.h"

#include <math.h>

#include <algorithm>

namespace pb {

constexpr uint64_t kMaxEnvTexels = 1ull << 26;  // 64 Mi texels (1 GB of radiance + pdf on the device)

double env_texel_solid_angle(uint32_t row, uint32_t w, uint32_t h) {
  const double pi = 3.14159265358979323846;
  return (2.0 * pi / (double)w) * (cos(pi * (double)row / (double)h) - cos(pi * (double)(row + 1u) / (double)h));
}

int build_env_tables(const float* rgb, uint32_t width, uint32_t height, float scale, EnvTables* out) {
  *out = EnvTables();
  if (!rgb || width == 0 || height == 0 || (uint64_t)width * height > kMaxEnvTexels) return -1;
  if (!(scale >= 0.0f) || !isfinite(scale)) return -1;
  const size_t n = (size_t)width * height;
  for (size_t i = 0; i < 3 * n; i++)
    if (!(rgb[i] >= 0.0f) || !isfinite(rgb[i])) return -1;
  EnvTables& t = *out;
  t.width = width, t.height = height;
  t.weight.resize(n);
  double norm = 0.0;
  std::vector<double> lum(n);
  for (uint32_t r = 0; r < height; r++) {
    const double omega = env_texel_solid_angle(r, width, height);
    for (uint32_t c = 0; c < width; c++) {
      const size_t i = (size_t)r * width + c;
      lum[i] = scale > 0.0f ? env_lum(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]) : 0.0;
      t.weight[i] = lum[i] * omega;
      norm += t.weight[i];
    }
  }
  if (!(norm > 0.0)) {  // an all-black map is no environment
    t.weight.clear();
    return 0;
  }
  t.present = true, t.norm = norm;
  t.texels.resize(4 * n);
  for (size_t i = 0; i < n; i++) {
    t.texels[4 * i] = rgb[3 * i] * scale, t.texels[4 * i + 1] = rgb[3 * i + 1] * scale, t.texels[4 * i + 2] = rgb[3 * i + 2] * scale;
    t.texels[4 * i + 3] = (float)(lum[i] / norm);
  }
  // Vose's alias method on q_i = n * weight_i / norm (mean 1)
  std::vector<double> q(n);
  std::vector<uint32_t> small, large;
  small.reserve(n), large.reserve(n);
  for (size_t i = 0; i < n; i++) {
    q[i] = (double)n * (t.weight[i] / norm);
    (q[i] < 1.0 ? small : large).push_back((uint32_t)i);
  }
  t.prob.assign(n, 1.0f), t.alias.resize(n);
  for (size_t i = 0; i < n; i++) t.alias[i] = (uint32_t)i;
  while (!small.empty() && !large.empty()) {
    const uint32_t s = small.back(), l = large.back();
    small.pop_back();
    t.prob[s] = (float)q[s], t.alias[s] = l;
    q[l] = (q[l] + q[s]) - 1.0;
    if (q[l] < 1.0) {
      large.pop_back();
      small.push_back(l);
    }
  }
  // what rounding leaves over has q ~ 1: kept with probability 1 -- except a black texel, which must never be chosen
  uint32_t any_lit = 0;
  while (t.weight[any_lit] == 0.0) any_lit++;
  for (uint32_t s : small) {
    if (t.weight[s] == 0.0) t.prob[s] = 0.0f, t.alias[s] = any_lit;
    else t.prob[s] = 1.0f, t.alias[s] = s;
  }
  for (uint32_t l : large) t.prob[l] = 1.0f, t.alias[l] = l;
  t.keep.resize(n);
  for (size_t i = 0; i < n; i++) t.keep[i] = (uint32_t)std::min(ceil((double)t.prob[i] * 4294967296.0), 4294967295.0);
  return 0;
}

}  // namespace pb
