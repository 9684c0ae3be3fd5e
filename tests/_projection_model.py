"""A float64 model of the three projections of pbrhip_projection_rays_device, written from the formulas in
include/pbrhip.h and from nothing else: the camera frame, the sample jitter from a PCG32 of its own, and the ray of every pixel."""
import numpy as np

LATLONG, FISHEYE, ORTHO = 0, 1, 2
KINF = np.float32(1.844e18)
MASK = (1 << 64) - 1
MUL = 6364136223846793005


def frame(eye, lookat, up):
    """eye, r, u, f in float64: f towards lookat, r = f x up, u = r x f, normalised"""
    eye, lookat, up = (np.asarray(np.asarray(v, np.float32), np.float64) for v in (eye, lookat, up))
    f = lookat - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    return eye, r, np.cross(r, f), f


def _pcg32(state, inc):
    new = (state * MUL + inc) & MASK
    xs = (((state >> 18) ^ state) >> 27) & 0xFFFFFFFF
    rot = state >> 59
    return new, ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF


def jitter(gpix, npass_pass, seed_seq=1234567890):
    """the first two draws of the generator of (pixel, pass): rng_seed((pass << 32) + pixel, seed_seq), each (bits >> 9 | 0x3f800000) - 1"""
    inc = ((seed_seq << 1) | 1) & MASK
    state, _ = _pcg32(0, inc)
    state = (state + (npass_pass << 32) + gpix) & MASK
    state, _ = _pcg32(state, inc)
    out = []
    for _ in range(2):
        state, bits = _pcg32(state, inc)
        out.append(float(np.array((bits >> 9) | 0x3F800000, np.uint32).view(np.float32)) - 1.0)
    return out


def jitters(width, height, npass_pass, seed_seq=1234567890):
    j = np.array([jitter(p, npass_pass, seed_seq) for p in range(width * height)], np.float64)
    return j[:, 0].reshape(height, width), j[:, 1].reshape(height, width)


def rays(projection, cam, width, height, jx, jy, param=0.0, fov=30.0):
    """-> (org (H, W, 3), dir (H, W, 3), active (H, W), rho (H, W)) in float64.  cam = frame(...); jx, jy (H, W) in [0, 1).
    fisheye: param = the field of view in degrees, 0 = fov; ortho: param = half the height"""
    eye, r, u, f = cam
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    fx, fy = x + jx, y + jy
    org = np.broadcast_to(eye, (height, width, 3)).copy()
    active = np.ones((height, width), bool)
    rho = np.zeros((height, width))
    if projection == LATLONG:
        phi, theta = 2 * np.pi * fx / width - np.pi, np.pi * fy / height
        d = (np.sin(theta) * np.sin(phi))[..., None] * r + np.cos(theta)[..., None] * u + (np.sin(theta) * np.cos(phi))[..., None] * f
    else:
        sx, sy = (2 * fx / width - 1) * (width / height), 1 - 2 * fy / height
        if projection == FISHEYE:
            rho = np.hypot(sx, sy)
            ang = rho * np.radians(param if param > 0 else fov) / 2
            k = np.where(rho > 0, np.sin(ang) / np.where(rho > 0, rho, 1), 0.0)
            d = (k * sx)[..., None] * r + (k * sy)[..., None] * u + np.cos(ang)[..., None] * f
            active = rho <= 1
        else:
            org = eye + (sx * param)[..., None] * r + (sy * param)[..., None] * u
            d = np.broadcast_to(f, (height, width, 3)).copy()
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return org, d, active, rho
