// dcamera_pixel.h -- the cameras of dcamera.h with the jitter given instead of drawn, and their inverses (device): what the motion
// kernel (temporal.hip) needs of a camera.  dcamera.h's arithmetic, operation for operation; the lens point is the lens
// centre, so the ray of a thin-lens camera is its pinhole's.
#pragma once

#include "dscene.h"

namespace pb {

// user_camera_ray with jx, jy given and the lens point at the lens centre (lo = 0: d = normalize_raw(p) whatever the focus distance)
__device__ __forceinline__ void user_camera_ray_at(const UserCamera& c, uint32_t x, uint32_t y, uint32_t width, uint32_t height, float jx,
                                                   float jy, V3& o, V3& d) {
  const float sx = (2.0f * ((float)x + jx) / (float)width - 1.0f) * c.ha;
  const float sy = (1.0f - 2.0f * ((float)y + jy) / (float)height) * c.h;
  const V3 f(c.f[0], c.f[1], c.f[2]), r(c.r[0], c.r[1], c.r[2]), u(c.u[0], c.u[1], c.u[2]);
  const V3 p = f + sx * r + sy * u;
  o = V3(c.eye[0], c.eye[1], c.eye[2]);
  d = normalize_raw(p);
}

// reference_camera_ray with jx, jy given
__device__ __forceinline__ void reference_camera_ray_at(const Camera& c, uint32_t x, uint32_t y, float jx, float jy, V3& o, V3& d) {
  o = V3(c.org[0], c.org[1], c.org[2]);
  const V3 target(c.x_corner + c.dx * ((float)x + jx), c.y_corner - c.dy * ((float)y + jy), c.z_corner);
  d = normalize_raw(target - o);
}

// The inverses: the continuous pixel coordinates (px, py) = (x + jx, y + jy) whose ray passes through the world point X, and
// dist = |X - eye|.  False when X is not in front of the camera (px, py, dist are then not meaningful).
// User camera: with v = X - eye, the point of the ray on the unit image plane is v / (v . f), so sx = (v . r) / (v . f), sy = (v . u) / (v . f)
// (f, r, u orthonormal), px = (sx / ha + 1) W / 2, py = (1 - sy / h) H / 2.
__device__ __forceinline__ bool user_camera_project(const UserCamera& c, uint32_t width, uint32_t height, V3 X, float& px, float& py, float& dist) {
  const V3 f(c.f[0], c.f[1], c.f[2]), r(c.r[0], c.r[1], c.r[2]), u(c.u[0], c.u[1], c.u[2]);
  const V3 v = X - V3(c.eye[0], c.eye[1], c.eye[2]);
  const float z = dot(v, f);
  if (!(z > 0.0f)) return false;
  const float sx = dot(v, r) / z, sy = dot(v, u) / z;
  px = (sx / c.ha + 1.0f) * (0.5f * (float)width);
  py = (1.0f - sy / c.h) * (0.5f * (float)height);
  dist = sqrtf(dot(v, v));
  return true;
}
// Reference camera: the ray from org through X meets the image plane z = z_corner at org + k v, k = (z_corner - org.z) / v.z, which has
// to be positive; px = (org.x + k v.x - x_corner) / dx, py = (y_corner - (org.y + k v.y)) / dy.
__device__ __forceinline__ bool reference_camera_project(const Camera& c, V3 X, float& px, float& py, float& dist) {
  const V3 v = X - V3(c.org[0], c.org[1], c.org[2]);
  const float k = (c.z_corner - c.org[2]) / v.z;
  if (!(k > 0.0f) || !(k < __builtin_huge_valf())) return false;
  px = ((c.org[0] + k * v.x) - c.x_corner) / c.dx;
  py = (c.y_corner - (c.org[1] + k * v.y)) / c.dy;
  dist = sqrtf(dot(v, v));
  return true;
}

}  // namespace pb
