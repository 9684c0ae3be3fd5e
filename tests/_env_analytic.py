"""Float64 expectations for the environment light on a Lambert floor with nothing above it.

The floor (z = 0, normal +z) sees the whole upper hemisphere of the map, so the reflected radiance is the same at every
floor point: E = (rho / pi) * integral of L(w) cos(w, n) over the hemisphere."""
import numpy as np

import _analytic as A

RHO = np.array([0.7, 0.5, 0.3])
LAMBERT = dict(base_color=tuple(RHO), specular=0.0)
# world +z (the floor's normal) -> env +y: env = M world
Z_UP = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])


def floor_scene():
    """the floor, and a tiny black sliver in its plane that widens the scene's box (so the camera also sees the background)
    without hiding any of the sky from the floor (it is coplanar with it)"""
    v, f = A.quad((0, 0, 0), (1.0, 0, 0), (0, 0.75, 0))
    sv = np.array([[1.6, -0.001, 0.0], [1.7, -0.001, 0.0], [1.7, 0.001, 0.0]])
    return A.Scene([A.Mesh("floor", v, f, A.material(**LAMBERT)), A.Mesh("sliver", sv, np.array([[0, 1, 2]]), A.material(**A.BLACK))])


def constant_expectation(L):
    return RHO * np.asarray(L, np.float64)


def skewed_constant_expectation(L, n=200000):
    """what a Lambert floor under a constant sky would converge to if the environment's NEE weight took Q3's skewed pdf
    pdf_env / |cos| while the miss weight kept the solid-angle pdf: the two weights no longer sum to 1"""
    mu = (np.arange(n) + 0.5) / n                       # cos(theta), midpoint rule
    pdf_env, pdf_bsdf = 1.0 / (4.0 * np.pi), mu / np.pi
    a = pdf_env / mu
    w_nee = a * a / (a * a + pdf_bsdf * pdf_bsdf)
    w_bsdf = pdf_bsdf * pdf_bsdf / (pdf_bsdf * pdf_bsdf + pdf_env * pdf_env)
    s = np.mean(mu * (w_nee + w_bsdf)) * 2.0 * np.pi / np.pi   # (rho / pi) L * 2 pi * int mu (w + w') dmu, over rho L
    return RHO * np.asarray(L, np.float64) * s


def map_expectation(rgb, scale):
    """a map rotated by Z_UP (env-up = the floor's normal): rows 0 .. H/2 - 1 are the floor's sky, and texel t contributes
    (rho / pi) L_t (phi1 - phi0) (sin^2 theta1 - sin^2 theta0) / 2"""
    h, w, _ = rgb.shape
    assert h % 2 == 0
    th = np.pi * np.arange(h + 1) / h
    band = (np.sin(th[1:]) ** 2 - np.sin(th[:-1]) ** 2) / 2.0      # int cos sin dtheta over each row
    band[h // 2:] = 0.0
    dphi = 2.0 * np.pi / w
    e = (np.asarray(rgb, np.float64) * scale * band[:, None, None] * dphi).sum((0, 1))
    return RHO / np.pi * e


def env_texel(d_env, w, h):
    """float64 version of denv.h::env_texel_index: (row, col) of env-space directions (N, 3)"""
    y = np.clip(d_env[:, 1], -1.0, 1.0)
    theta = np.arccos(y)
    phi = np.arctan2(d_env[:, 0], -d_env[:, 2]) + np.pi
    col = np.clip(np.floor(phi / (2 * np.pi) * w), 0, w - 1).astype(int)
    row = np.clip(np.floor(theta / np.pi * h), 0, h - 1).astype(int)
    return row, col


def background_texels(S, cam, m, w, h, probe=6):
    """per pixel: the texel (row, col) every probe ray of its slightly widened footprint that misses the scene lands in, or
    (-1, -1) when the footprint touches geometry or spans texels"""
    W, H = cam.width, cam.height
    py, px = np.mgrid[0:H, 0:W]
    js = np.linspace(-0.02, 1.02, probe)
    jx, jy = np.meshgrid(js, js, indexing="ij")
    d = cam.dirs(px[..., None].astype(np.float64), py[..., None].astype(np.float64), jx.ravel(), jy.ravel()).reshape(-1, 3)
    mesh, _, _, _ = A.cast(S, cam.org, d)
    r, c = env_texel(d @ np.asarray(m, np.float64).T, w, h)
    mesh, r, c = mesh.reshape(H, W, -1), r.reshape(H, W, -1), c.reshape(H, W, -1)
    ok = np.all(mesh < 0, -1) & np.all(r == r[..., :1], -1) & np.all(c == c[..., :1], -1)
    return np.where(ok, r[..., 0], -1), np.where(ok, c[..., 0], -1)


def sky_map(w=32, h=16, sun=(3, 21), sun_rgb=(400.0, 380.0, 300.0)):
    """a sky gradient (blue at the zenith, pale at the horizon, dark ground) and one bright sun texel"""
    rows = (np.arange(h) + 0.5) / h
    sky = np.stack([0.3 + 0.5 * rows, 0.45 + 0.35 * rows, 0.9 - 0.1 * rows], -1)
    sky[h // 2:] = [0.12, 0.1, 0.08]
    rgb = np.repeat(sky[:, None, :], w, 1) * (1.0 + 0.25 * np.sin(np.arange(w) * 2 * np.pi / w))[None, :, None]
    rgb[sun] = sun_rgb
    return rgb.astype(np.float32)


def polygon_form_factor(x, n, poly):
    """Lambert's formula: the point-to-polygon form factor (1 / pi) * integral of cos over the polygon's solid angle, for points x
    (N, 3) with normal n and a planar convex polygon (V, 3) wholly above their tangent planes"""
    R = np.asarray(poly, np.float64)[None] - np.asarray(x, np.float64)[:, None]
    R /= np.linalg.norm(R, axis=-1, keepdims=True)
    Rn = np.roll(R, -1, axis=1)
    c = np.cross(R, Rn)
    gamma = np.arccos(np.clip(np.sum(R * Rn, -1), -1.0, 1.0))
    c /= np.linalg.norm(c, axis=-1, keepdims=True)
    return np.abs(np.sum(gamma * (c @ np.asarray(n, np.float64)), -1)) / (2.0 * np.pi)


class SkyExpectation:
    """E(x) = rho L (1 - sum of the blockers' form factors) (+ an area-light expectation): a constant sky over the floor, seen
    past convex blockers that do not overlap as seen from the floor"""

    def __init__(self, L, blockers, area=None):
        self.L, self.blockers, self.area = np.asarray(L, np.float64), [np.asarray(b, np.float64) for b in blockers], area

    def __call__(self, x, wo, order=None):
        F = sum(polygon_form_factor(x, (0.0, 0.0, 1.0), b) for b in self.blockers)
        e = RHO[None] * self.L[None] * (1.0 - F)[:, None]
        return e if self.area is None else e + self.area(x, wo)
