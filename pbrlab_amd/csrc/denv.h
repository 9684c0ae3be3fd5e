// denv.h -- the lat-long environment light's mapping between directions and texels (host and device).
//
// An environment is an equirectangular map of W x H texels, nearest-sampled.  In env space d = (x, y, z), +y up:
//   theta = acos(clamp(y, -1, 1)), phi = atan2(x, -z) + pi;  column = floor(phi / 2pi * W), row = floor(theta / pi * H), both
//   clamped to the image; row 0 is the top (theta = 0).  A ray along -z lands mid-image.
// World directions are rotated into env space by DScene::env_m (row-major world_to_env; a rotation).
#pragma once
#include "dmath.h"

namespace pb {

// atan2 to a few ulp (Cephes' atanf on the octant, reduced once by pi/4), in plain float operations: the same bits on the host and the
// device, and a fraction of the registers of the device library's atan2f / acosf
PB_HD float env_atan2(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  float a = mx > 0.0f ? mn / mx : 0.0f, base = 0.0f;
  if (a > 0.4142135623730950f) a = (a - 1.0f) / (a + 1.0f), base = 0.7853981633974483f;
  const float z = a * a;
  float p = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
  p = fmaf(p, z, 1.99777106478e-1f);
  p = fmaf(p, z, -3.33329491539e-1f);
  float r = base + fmaf(p * z, a, a);
  if (ay > ax) r = 1.5707963267948966f - r;
  if (x < 0.0f) r = kPi - r;
  return y < 0.0f ? -r : r;
}

// texel index (row * W + column) of an env-space direction
PB_HD uint32_t env_texel_index(V3 d, uint32_t w, uint32_t h) {
  const float y = fminf(fmaxf(d.y, -1.0f), 1.0f);
  const float theta = env_atan2(sqrtf((1.0f - y) * (1.0f + y)), y);  // acos(y), accurate near the poles too
  const float phi = env_atan2(d.x, -d.z) + kPi;
  // (fmaxf first: a NaN direction reads texel 0 instead of converting NaN to an integer)
  const float fc = fminf(fmaxf(floorf(phi / (2.0f * kPi) * (float)w), 0.0f), (float)(w - 1u));
  const float fr = fminf(fmaxf(floorf(theta / kPi * (float)h), 0.0f), (float)(h - 1u));
  return (uint32_t)fr * w + (uint32_t)fc;
}

// sine and cosine for sampling directions: the project's f_cos / f_sin, the same bits on the host and the device (the host checker,
// scripts/fuzz/env_check.cpp, runs what the kernels run)
PB_HD float env_cos(float x) { return f_cos(x); }
PB_HD float env_sin(float x) { return f_sin(x); }

// the env-space direction at (u, v) in [0, 1)^2 of texel (col, row): uniform in phi and in cos(theta) over the texel, i.e. uniform
// over its solid angle
PB_HD V3 env_texel_dir(uint32_t col, uint32_t row, uint32_t w, uint32_t h, float u, float v) {
  const float phi = 2.0f * kPi * (((float)col + u) / (float)w) - kPi;  // atan2(x, -z)
  const float c0 = env_cos(kPi * ((float)row / (float)h)), c1 = env_cos(kPi * ((float)(row + 1u) / (float)h));
  const float ct = c0 + v * (c1 - c0);
  const float st = sqrtf(fmaxf(0.0f, 1.0f - ct * ct));
  return V3(st * env_sin(phi), ct, -(st * env_cos(phi)));
}

// m: world_to_env, row-major
PB_HD V3 env_from_world(const float* m, V3 a) {
  return V3(m[0] * a.x + m[1] * a.y + m[2] * a.z, m[3] * a.x + m[4] * a.y + m[5] * a.z, m[6] * a.x + m[7] * a.y + m[8] * a.z);
}
PB_HD V3 env_to_world(const float* m, V3 d) {  // (the transpose: m is a rotation)
  return V3(m[0] * d.x + m[3] * d.y + m[6] * d.z, m[1] * d.x + m[4] * d.y + m[7] * d.z, m[2] * d.x + m[5] * d.y + m[8] * d.z);
}

}  // namespace pb
