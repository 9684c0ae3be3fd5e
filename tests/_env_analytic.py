"""Float64 expectations for the environment light.

A Lambert floor with nothing above it (z = 0, normal +z) sees the whole upper hemisphere of the map, so the reflected radiance
is the same at every floor point: E = (rho / pi) * integral of L(w) cos(w, n) over the hemisphere.  A white Lambert box open
to a constant sky is a furnace: every pixel converges to L, however often its paths bounce.  A principled floor (metallic GGX, or a
mix of the Lambert, GGX and clearcoat closures) under a constant sky keeps the reference's skewed GGX pdf (Q15) and the clearcoat's
sampler on the BSDF side: GGXSkyExpectation."""
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


WHITE = dict(base_color=(1.0, 1.0, 1.0), specular=0.0)


def deep_box_scene(depth=3.0):
    """a white Lambert box (albedo 1), 1 wide and `depth` deep, open towards +z (the reference camera looks into it); every face
    faces inwards.  The image is wider than the box: the columns beyond its rim see only the sky."""
    d = 0.5 * depth
    parts = [A.quad((0, 0, -depth), (0.5, 0, 0), (0, 0.5, 0)),                  # floor, +z
             A.quad((-0.5, 0, -d), (0, 0.5, 0), (0, 0, d)),                      # x = -1/2, +x
             A.quad((0.5, 0, -d), (0, 0, d), (0, 0.5, 0)),                       # x = +1/2, -x
             A.quad((0, -0.5, -d), (0, 0, d), (0.5, 0, 0)),                      # y = -1/2, +y
             A.quad((0, 0.5, -d), (0.5, 0, 0), (0, 0, d))]                       # y = +1/2, -y
    v = np.concatenate([p[0] for p in parts])
    f = np.concatenate([p[1] + 4 * k for k, p in enumerate(parts)])
    return A.Scene([A.Mesh("box", v, f, A.material(**WHITE))])


def sky_pixels(S, cam):
    """pixels that no triangle's image can reach: outside the box, widened by a pixel, of every triangle's vertices projected through
    the camera onto its image plane (probe rays alone can slip past a sliver thinner than their spacing)"""
    W, H = cam.width, cam.height
    free = np.ones((H, W), bool)
    for m in S.meshes:
        v = np.asarray(m.verts, np.float64)
        assert (v[:, 2] < cam.org[2]).all()
        p = cam.org + (v - cam.org) * ((cam.zc - cam.org[2]) / (v[:, 2] - cam.org[2]))[:, None]
        px, py = (p[:, 0] - cam.xc) / cam.dx, (cam.yc - p[:, 1]) / cam.dy
        for f in np.asarray(m.faces):
            x0, x1 = int(np.floor(px[f].min())) - 1, int(np.ceil(px[f].max())) + 1
            y0, y1 = int(np.floor(py[f].min())) - 1, int(np.ceil(py[f].max())) + 1
            free[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = False
    return free


GGX_METAL = dict(base_color=(0.9, 0.6, 0.3), metallic=1.0, roughness=0.7, specular=0.5, anisotropic=0.0)


def ggx_floor_scene(mat=None):
    """floor_scene with the receiver of test_analytic_radiance's ggx_metallic case, or with the principled material `mat`"""
    S = floor_scene()
    return A.Scene([A.Mesh("floor", S.meshes[0].verts, S.meshes[0].faces, A.material(**(mat or GGX_METAL))), S.meshes[1]])


class GGXSkyExpectation:
    """E(wo) for an isotropic principled floor (A.closure_set: any mix of the Lambert, GGX and clearcoat closures) under a constant
    sky L, no area light (p_env = 1, pdf_env = 1 / 4 pi).  With (f, q, p_true) = A.lobes, q the pdf the shader reports (GGX and
    clearcoat with Q15's extra 1 / cos_i) and p = 1 / 4 pi:
        NEE:  E f L cos_i / p x p^2 / (p^2 + q^2)   over the env sample  ->  int f L cos_i w_env dw
        BSDF: wi is drawn with density p_true and the path carries f cos_i / q, weighted q^2 / (q^2 + p^2) at the miss
                                                                         ->  int f L cos_i (p_true / q) w_bsdf dw
    (the metallic GGX floor alone: p_true / q = cos_i).  Below the floor (cos_i <= 0, reached by the GGX samplers only, with
    density p_true) f is the Lambert closure's alone and q its negative pdf: the ray misses everything and adds the NEGATIVE
    f |cos_i| / q L w_bsdf -- the lower part of the same integral, zero for a floor without a Lambert closure.
    below=False: without that lower part (a sampler that never left the hemisphere).
    q15=False: what a shader whose pdf were its sampling density would converge to, int f L cos_i dw (the weights sum to 1).
    The floor is isotropic, so E depends on cos_o alone: a Gauss-Legendre (cos_i) x trapezoid (phi, periodic) rule over the
    hemisphere at Chebyshev nodes of cos_o, interpolated by their polynomial.  The lower part: Gauss-Legendre on cos_i in (-cos_o, 0) and in the azimuth (see at())."""

    def __init__(self, S, L, q15=True, n_mu=96, n_phi=192, n_grid=32, below=True):
        self.cl = A.closure_set(S.meshes[S.receiver].material)
        sp = self.cl["specular"]
        assert sp is None or sp["ax"] == sp["ay"], "E must depend on cos_o alone"
        self.L, self.q15, self.below = np.asarray(L, np.float64), q15, below
        self.n_mu, self.n_phi, self.n_grid = n_mu, n_phi, n_grid
        self.grid = None

    def at(self, co, n_mu=None, n_phi=None, lower=None):
        """E for view cosines co (N,), (N, 3)"""
        n_mu, n_phi = n_mu or self.n_mu, n_phi or self.n_phi
        lower = self.below if lower is None else lower
        mu, wmu = A.gauss_legendre01(n_mu)
        phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
        co = np.asarray(co, np.float64)
        wo = np.stack([np.sqrt(1.0 - co * co), np.zeros_like(co), co], -1)
        sel = tuple(w[:, None] for w in A.selection_weights(self.cl, wo))
        p = 1.0 / (4.0 * np.pi)

        def part(M, wq, phi, wphi):
            """sum over directions with cos_i = M (N or 1, n_mu), weights wq (same), and azimuths phi, weights wphi"""
            st = np.sqrt(1.0 - M * M)
            wi = np.stack([st[..., None] * np.cos(phi), st[..., None] * np.sin(phi), M[..., None] * np.ones(n_phi)], -1)
            wi = wi.reshape(M.shape[0], -1, 3)                                     # (N or 1, Q, 3)
            w2 = (wq[..., None] * wphi).reshape(M.shape[0], -1)
            f, q, pt = A.lobes(self.cl, wi, wo[:, None], sel=sel)
            ci = wi[..., 2]
            if self.q15:
                w_env, w_bsdf = p * p / (p * p + q * q), q * q / (q * q + p * p)
                ratio = np.where(q != 0, pt / np.where(q != 0, q, 1.0), 0.0)
                k = np.where(ci > 0, ci * w_env, 0.0) + np.abs(ci) * ratio * w_bsdf
            else:
                k = np.where(ci > 0, ci, 0.0) * np.ones_like(q)
            return np.einsum("nqc,nq,nq->nc", f, k, np.broadcast_to(w2, k.shape))
        e = part(mu[None], wmu[None], phi, np.full(n_phi, 2.0 * np.pi / n_phi))
        if lower and self.q15 and self.cl["diffuse"] is not None and A.lobe_width(self.cl) is not None:
            # p_true's half vector is undefined at wi = -wo (cos_i = -cos_o, phi = pi), a corner of this part's domain, and the
            # density's limit there depends on the direction of approach: Gauss-Legendre in t with phi = pi (1 + t^3) packs
            # the azimuths around it (cos_i's own nodes already crowd towards -cos_o)
            t, wt = np.polynomial.legendre.leggauss(n_phi)
            e = e + part(-co[:, None] * mu[None], co[:, None] * wmu[None], np.pi * (1.0 + t ** 3), 3.0 * np.pi * t * t * wt)
        return e * self.L

    def __call__(self, x, wo, order=None):
        co = np.abs(np.asarray(wo, np.float64)[:, 2])                         # the floor's normal is +z
        if self.grid is None:
            # E is smooth in cos_o: the polynomial through its values at n_grid Chebyshev nodes of [0.5, 1]
            self.grid = 0.75 + 0.25 * np.cos(np.pi * (np.arange(self.n_grid) + 0.5) / self.n_grid)
            self.table = np.polynomial.chebyshev.chebfit(4.0 * self.grid - 3.0, self.at(self.grid), self.n_grid - 1)
        assert co.min() >= 0.5
        return np.polynomial.chebyshev.chebval(4.0 * co - 3.0, self.table).T
