// dcamera.h -- the camera ray of one sample (device), shared by the render kernels (kernels.hip) and the feature kernel (features.hip).
#pragma once

#include "dscene.h"

namespace pb {

// ------------------------------------------------------------------ the user camera
// The camera ray of pixel (x, y) from a generator seeded for its sample: jx, jy, then (thin lens only) u1, u2 for the lens point
// rho (cos phi, sin phi), rho = lens sqrt(u1), phi = 2 pi u2.  Direction: through the pixel's point on the focal plane.
__device__ __forceinline__ void user_camera_ray(const UserCamera& c, uint32_t x, uint32_t y, uint32_t width, uint32_t height, Rng& rng, V3& o,
                                                V3& d) {
  const float jx = draw(rng);
  const float jy = draw(rng);
  const float sx = (2.0f * ((float)x + jx) / (float)width - 1.0f) * c.ha;
  const float sy = (1.0f - 2.0f * ((float)y + jy) / (float)height) * c.h;
  const V3 f(c.f[0], c.f[1], c.f[2]), r(c.r[0], c.r[1], c.r[2]), u(c.u[0], c.u[1], c.u[2]);
  const V3 p = f + sx * r + sy * u;
  o = V3(c.eye[0], c.eye[1], c.eye[2]);
  if (c.lens > 0.0f) {
    const float u1 = draw(rng);
    const float u2 = draw(rng);
    const float rho = c.lens * sqrtf(u1), phi = 2.0f * kPi * u2;
    const V3 lo = (rho * cosf(phi)) * r + (rho * sinf(phi)) * u;
    o = o + lo;
    d = normalize_raw(c.focus * p - lo);
  } else {
    d = normalize_raw(p);
  }
}

// The reference's camera (render.cc:160-171; kernels.hip::camera_sample's arithmetic): jx, jy, then the direction through the pixel's
// point on the image plane.
__device__ __forceinline__ void reference_camera_ray(const Camera& c, uint32_t x, uint32_t y, Rng& rng, V3& o, V3& d) {
  const float jx = draw(rng);
  const float jy = draw(rng);
  o = V3(c.org[0], c.org[1], c.org[2]);
  const V3 target(c.x_corner + c.dx * ((float)x + jx), c.y_corner - c.dy * ((float)y + jy), c.z_corner);
  d = normalize_raw(target - o);
}

}  // namespace pb
