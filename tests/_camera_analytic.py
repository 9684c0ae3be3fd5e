"""Float64 models of the look-at camera and of the generator draws that feed it.

`LookAt` has the duck type tests/_analytic.py's classify_and_expect and pixel_mean take (org, dirs(px, py, jx, jy), width, height):
for a pinhole it is the camera itself; for a thin lens `dirs` gives the pinhole through eye with the same frame, whose footprint on
the focal plane is the thin lens's footprint there.  `rays` gives the thin lens's origins and directions from the same draws."""
import numpy as np

_MULT = np.uint64(6364136223846793005)


def _pcg32(state, inc):
    old = state
    state = old * _MULT + inc
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
    rot = (old >> np.uint64(59)).astype(np.uint32)
    out = (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))
    return state, out.astype(np.uint32)


def draws(initstate, initseq, n):
    """the first n draws (float32 in [0, 1), as float64) of pcg32 generators seeded like rng_seed (dmath.h): (len(initstate), n)"""
    with np.errstate(over="ignore"):
        init = np.atleast_1d(np.asarray(initstate, np.uint64))
        inc = np.uint64((int(initseq) << 1 | 1) & 0xFFFFFFFFFFFFFFFF)
        state = np.zeros_like(init)
        state, _ = _pcg32(state, inc)
        state = state + init
        state, _ = _pcg32(state, inc)
        out = np.zeros((len(init), n))
        for k in range(n):
            state, x = _pcg32(state, inc)
            f = ((x >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
            out[:, k] = f
    return out


def sample_draws(width, x, y, pas, seed_seq, n):
    """the draws of the samples (x, y, pass) of a width-wide image (the renderer's seeding: (pass << 32) + y width + x)"""
    x, y, pas = (np.asarray(v, np.uint64) for v in (x, y, pas))
    return draws((pas << np.uint64(32)) + y * np.uint64(width) + x, seed_seq, n)


class LookAt:
    """the look-at camera in float64 from the float32 values the caller passes"""

    def __init__(self, eye, lookat, up, fov, width, height, lens_radius=0.0, focus_distance=0.0):
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
        self.eye, lookat, up = f32(eye), f32(lookat), f32(up)
        f = lookat - self.eye
        dist = np.linalg.norm(f)
        self.f = f / dist
        r = np.cross(self.f, up)
        self.r = r / np.linalg.norm(r)
        self.u = np.cross(self.r, self.f)
        self.h = np.tan(np.radians(float(np.float32(fov))) / 2)
        self.width, self.height = width, height
        self.lens = float(np.float32(lens_radius))
        self.focus = float(np.float32(focus_distance)) if focus_distance > 0 else dist
        self.org = self.eye

    def points(self, px, py, jx, jy):
        """the unit-distance image-plane points f + sx r + sy u of image positions (px + jx, py + jy)"""
        sx = (2.0 * (px + jx) / self.width - 1.0) * self.h * self.width / self.height
        sy = (1.0 - 2.0 * (py + jy) / self.height) * self.h
        return self.f + np.asarray(sx)[..., None] * self.r + np.asarray(sy)[..., None] * self.u

    def dirs(self, px, py, jx, jy):
        p = self.points(px, py, jx, jy)
        return p / np.linalg.norm(p, axis=-1, keepdims=True)

    def rays(self, px, py, d):
        """origins and unit directions of samples at pixels (px, py) from their draws d (n, 2 or 4)"""
        p = self.points(np.asarray(px, np.float64), np.asarray(py, np.float64), d[:, 0], d[:, 1])
        if self.lens == 0.0:
            return np.broadcast_to(self.eye, p.shape).copy(), p / np.linalg.norm(p, axis=-1, keepdims=True)
        rho, phi = self.lens * np.sqrt(d[:, 2]), 2.0 * np.pi * d[:, 3]
        lo = (rho * np.cos(phi))[:, None] * self.r + (rho * np.sin(phi))[:, None] * self.u
        v = self.focus * p - lo
        return self.eye + lo, v / np.linalg.norm(v, axis=-1, keepdims=True)
