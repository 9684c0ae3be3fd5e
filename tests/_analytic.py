"""Float64 expectations for single-bounce scenes: what a pixel of the renderer should converge to, derived from the
reference's rules (SURVEY.md §8(a')) and not from the oracle's code.  Test infrastructure only.

Scope: untransformed triangle meshes; one receiver, a planar principled surface with any set of the non-subsurface closures
(closure_set: Lambert, anisotropic GGX with its Fresnel tint, clearcoat; cycles-principled-shader.cc:244-412) in the shader's
own tangent frame (branchless_onb), its base colour a parameter or a texture read per point (tests/_texture_model.py; Textured,
texel_pieces); emitters and occluders with a black material; area lights with constant shading normals
per face.  A camera ray that hits such a receiver gathers light along exactly one bounce:

  E(x) = sum over the light faces of  int_{V(x)}  f(w) Le (cos_p cos_l / d^2) [w_nee(y) + w_bsdf(y)] dA(y)     (Lambert)

with, from the rows of SURVEY §8(a'):
  p_A(y)  = max(Le_f) / sum_faces(max(Le) area)                                   (Q10: face weight max(Le)*area)
  q_nee   = p_A d^2 / (cos_l cos_p)                                                (Q3: both cosines)
  q_bsdf  = the BSDF pdf the shader returns for w                                  (Lambert: cos_p / pi)
  w_nee   = q_nee^2 / (q_nee^2 + q_bsdf^2)                                         (power heuristic)
  w_bsdf  = q_bsdf^2 / (q_bsdf^2 + (p_A d^2 / |n_s.w|)^2), only for kFront hits   (Q2: the light's SHADING normal, and
            (w.n_g < 0 and w.n_s < 0)                                                 kFront needs both normals)
so w_nee + w_bsdf != 1 wherever cos_p is not 1 (Q3's inconsistency).

The closure set (lobes): f is the sum of the enabled closures; q_bsdf = q_rep = sum_k w_k pdf_k with the selection weights
w_k of Q7 (selection_weights); the BSDF-sampled path draws wi with p_true = sum_k w_k p_k and carries f cos_p / q_rep, so
  E(x) = sum over the light faces of  int_{V(x)}  f Le (cos_p cos_l / d^2) [w_nee + (p_true / q_rep) w_bsdf] dA(y)
with both weights built from q_rep.  Lambert alone: p_true / q_rep = 1.  GGX alone: p_true / q_rep = cos_p (Q15, below).
A modelled quirk (Q16): MicrofacetGGXSample draws from the GTR2 distribution of visible normals whatever `distrib` is, so
the clearcoat is SAMPLED from GTR2 at its own alpha while its reported pdf is GTR1 with alpha^2 = 0.0625 inside G (Q8);
ggx_vndf_pdf is that density, and tests/test_analytic_radiance.py::test_ggx_sampler_density_matches_model holds it to the
reference's own sampler.  The sampler can also put wi below the surface; in these scenes nothing emits there
(tests/_env_analytic.py models what an environment adds along such rays).

Q15 (the GGX pdf, microfacet-ggx.h:233-238): MicrofacetGGXBsdfPdf returns pdf = G1o D / (4 cos_o cos_i), the density
of its VNDF sampler G1o D / (4 cos_o) divided once more by cos_i.  For the GGX receiver the BSDF-sampled path then
carries f cos_i / pdf = G1i cos_i and the MIS weights use the skewed pdf; the expectation of that path is
int f Le cos_i^2 w_bsdf dw instead of int f Le cos_i w_bsdf dw.  NEE is unaffected except through w_nee.

Why nothing else contributes at these geometries:
  Q1 (Russian roulette with p = max(throughput), unclamped): at depth 0 the throughput is (1,1,1), p = 1 > every draw
     in [0,1), so the camera path always survives; the only emission it can reach after that is added (render.cc:43-61)
     before the roulette of depth 1, and every later vertex has throughput 0: emitters and occluders are black (their
     closure weights are all 0, the shader's throughput is 0/0 -> 0), a planar receiver cannot be hit again by a ray
     leaving it, and a miss ends the path.
  Q9 (absolute 1e-3 offsets): the shadow ray spans [1e-3, d - 1e-3] and the next ray starts at 1e-3; every separation
     in these scenes (receiver to emitter or occluder, occluder to emitter) is >= 5e-2, so neither interval cuts off
     geometry that matters, and the planar emitter cannot occlude itself.
  Camera rays that land on an emitter's front face are worth exactly Le (depth-0 weight 1, black shader adds 0);
  rays that land on black geometry, on a back face of an emitter, or miss are worth exactly 0.

Visibility: the shadow of a convex black occluder seen from x, projected onto the light's plane, is the convex hull of
its projected vertices (valid when the occluder lies between x and that plane, which is asserted); the visible part of a
light face, P \\ Q, is split into convex pieces by successive half-planes of Q and every piece is integrated with a
collapsed Gauss-Legendre rule.  The hemisphere and kFront conditions are half-planes in y as well (n_s is constant per
face), so every integrand is smooth on its piece."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

REFINE = 1.0        # quadrature: a triangle's longest edge <= REFINE x (its distance from x) ...
MAX_SPLITS = 8      # ... reached by at most this many 4-way splits
STEEP = 0.3       # pixel footprint: a 2 x 2 Gauss-Legendre rule; pixels whose 4 nodes spread by more than STEEP are left out
CHUNK = 20000       # triangles per vectorised quadrature step


# ------------------------------------------------------------------------------------------------- scene description
@dataclass
class Mesh:
    name: str
    verts: np.ndarray                    # (V,3)
    faces: np.ndarray                    # (F,3)
    material: dict                       # principled parameters (scenes.PRINCIPLED_DEFAULTS keys)
    emission: Optional[np.ndarray] = None  # (F,3) per-face Le, or None: not an emitter
    normals: Optional[np.ndarray] = None   # (V,3) per-vertex shading normals, or None (geometric)
    texcoords: Optional[np.ndarray] = None     # (T,2) texture coordinates, looked up through texcoord_ids ...
    texcoord_ids: Optional[np.ndarray] = None  # ... (F,3); an id may be 0xFFFFFFFF: that face then has none (tests/_texture_model.py)


@dataclass
class Scene:
    meshes: List[Mesh]
    receiver: int = 0                    # index of the receiving (non-black) mesh
    occluders: List[int] = field(default_factory=list)   # convex black meshes that can shadow the lights
    textures: List[np.ndarray] = field(default_factory=list)  # (H,W,C) images; a material's *_tex_id is an index into this list


def build(scene, S: Scene, make_principled):
    """Replay S through the builder methods of pbrlab's Scene (both back ends: OracleScene / pbrlab_amd.Scene), one mesh +
    local scene + identity instance per mesh, per-face light params where Le differs between faces.  The textures come first and
    the materials' texture ids are remapped to what AddTexture returned, as scenes.build_scene does."""
    tex_ids = [scene.AddTexture(np.asarray(t, np.float32)) for t in S.textures]
    for m in S.meshes:
        mat = m.material
        if tex_ids:
            mat = dict(mat)
            for k in ("base_color_tex_id", "subsurface_color_tex_id"):
                if mat[k] != 0xFFFFFFFF:
                    mat[k] = tex_ids[mat[k]]
        mid = scene.AddMaterialParam(make_principled(mat))
        v4 = np.concatenate([np.asarray(m.verts, np.float32), np.ones((len(m.verts), 1), np.float32)], 1)
        f = np.asarray(m.faces, np.uint32)
        if m.normals is not None:
            n4 = np.concatenate([np.asarray(m.normals, np.float32), np.zeros((len(m.normals), 1), np.float32)], 1)
            nid = f
        else:
            n4, nid = None, None
        if m.texcoord_ids is not None:
            tc, tid = np.asarray(m.texcoords, np.float32), np.asarray(m.texcoord_ids, np.uint32)
        else:
            tc, tid = None, None
        mesh = scene.AddTriangleMesh(v4, n4, tc, f, nid, tid, np.full(len(f), mid, np.uint32))
        ls = scene.CreateLocalScene()
        scene.AddMeshToLocalScene(ls, mesh)
        inst = scene.CreateInstance(ls, None)
        if m.emission is not None:
            ids, seen = np.zeros(len(f), np.uint32), {}
            for k, e in enumerate(np.asarray(m.emission, np.float32)):
                key = tuple(float(c) for c in e)
                if key not in seen:
                    seen[key] = scene.AddLightParam(key)
                ids[k] = seen[key]
            scene.AttachLightParamIdsToInstance(inst, [ids])
    scene.CommitScene()
    return scene


def material(**kw):
    from pbrlab_amd import scenes
    d = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")
    d.update(kw)
    return d


BLACK = dict(base_color=(0.0, 0.0, 0.0), specular=0.0)


def quad(c, a, b):
    """quad centre c, half-edges a, b: two triangles with geometric normal along a x b"""
    c, a, b = (np.asarray(x, np.float64) for x in (c, a, b))
    return np.array([c - a - b, c + a - b, c + a + b, c - a + b]), np.array([[0, 1, 2], [0, 2, 3]])


# ------------------------------------------------------------------------------------------------- float64 leaves
def fresnel_dielectric_cos(c, eta):
    """closure-util.h:10-29 in float64 (vectorised over c)"""
    c = np.asarray(c, np.float64)
    eta = np.where(c < 0, 1.0 / eta, eta)
    c = np.abs(c)
    g = eta * eta - 1 + c * c
    gs = np.sqrt(np.maximum(g, 0.0))
    A = (gs - c) / (gs + c)
    B = (c * (gs + c) - 1) / (c * (gs - c) + 1)
    return np.where(g > 0, 0.5 * A * A * (1 + B * B), 1.0)


Y_WEIGHT = np.array([0.212671, 0.715160, 0.072169])     # RgbToY, pbrlab-util.h:48-51
CUT_OFF = 1e-3                                           # kClosureWeightCutOff = kEps, pbrlab_math.h:10
F32_EPS = float(np.finfo(np.float32).eps)


def branchless_onb(n):
    """shader-utils.h:44-50 in float64: the tangent frame (ex, ey) the shader builds around ez = n, n (...,3)"""
    n = np.asarray(n, np.float64)
    sign = np.copysign(1.0, n[..., 2])
    a = -1.0 / (sign + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    ex = np.stack([1.0 + sign * n[..., 0] * n[..., 0] * a, sign * b, -sign * n[..., 0]], -1)
    ey = np.stack([b, sign + n[..., 1] * n[..., 1] * a, -n[..., 1]], -1)
    return ex, ey


def _ggx_parts(wi, wo, ax, ay):
    """the anisotropic GTR2 branch of microfacet-ggx.h:195-229 (it equals the isotropic one, :188-194, when ax == ay) for any
    wi with wi.z + wo.z > 0: (D(m), G1o, G1(wi)) with m = the half vector; G1(wi) is 0 where wi.z <= 0"""
    co, ci = wo[..., 2], wi[..., 2]
    m = wi + wo
    m = m / np.linalg.norm(m, axis=-1, keepdims=True)
    mz = np.where(m[..., 2] > 0, m[..., 2], 1.0)
    sx, sy = -m[..., 0] / (mz * ax), -m[..., 1] / (mz * ay)
    sl = 1 + sx * sx + sy * sy
    D = 1.0 / (sl * sl * np.pi * ax * ay * mz ** 4)          # = alpha^2 / (pi c^4 (alpha^2 + tan^2)^2) when ax == ay

    def g1(w, c):
        cp2 = w[..., 0] ** 2 + w[..., 1] ** 2
        a2 = np.where(cp2 > 0, (w[..., 0] ** 2 * ax * ax + w[..., 1] ** 2 * ay * ay) / np.where(cp2 > 0, cp2, 1.0), ax * ay)
        return 2 / (1 + np.sqrt(1 + a2 * (1 - c * c) / (c * c)))
    return np.where(m[..., 2] > 0, D, 0.0), g1(wo, co), np.where(ci > 0, g1(wi, np.where(ci > 0, ci, 1.0)), 0.0), m


def ggx_eval(wi, wo, ax, ay, distrib=2):
    """Microfacet reflection, microfacet-ggx.h:164-245 read in float64: returns (f, pdf) with the reference's pdf
    G1o D / (4 cos_o cos_i) (Q15).  wi, wo: (...,3) in the local frame (z = normal).  distrib = 2: GTR2 (GGX).  distrib = 1
    (the clearcoat, Q8): where ax == ay, D is GTR1 (:48-53), both G1 take alpha^2 = 0.0625 whatever ax is, and f carries an
    extra 0.25 (:236); where ax != ay the anisotropic GTR2 branch runs and only the 0.25 remains of distrib."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    ax, ay = np.asarray(ax, np.float64), np.asarray(ay, np.float64)
    co, ci = wo[..., 2], wi[..., 2]
    ok = (co > 0) & (ci > 0)
    wi_, wo_ = np.where(ok[..., None], wi, [0.0, 0.0, 1.0]), np.where(ok[..., None], wo, [0.0, 0.0, 1.0])
    co_, ci_ = wo_[..., 2], wi_[..., 2]
    D, G1o, G1i, m = _ggx_parts(wi_, wo_, ax, ay)
    scale = 1.0
    if distrib == 1:
        iso = np.abs(ax - ay) < F32_EPS
        a2 = np.minimum(ax * ax, 0.999999)                     # (alpha >= 1: D = 1 / pi, :49)
        t = 1.0 + (a2 - 1.0) * m[..., 2] ** 2
        D1 = np.where(ax >= 1.0, 1.0 / np.pi, (a2 - 1.0) / (np.pi * np.log(a2) * t))
        g = lambda c: 2 / (1 + np.sqrt(1 + 0.0625 * (1 - c * c) / (c * c)))  # noqa: E731
        D, G1o, G1i = np.where(iso, D1, D), np.where(iso, g(co_), G1o), np.where(iso, g(ci_), G1i)
        scale = 0.25
    common = D * 0.25 / co_ / ci_
    return np.where(ok, scale * G1o * G1i * common, 0.0), np.where(ok, G1o * common, 0.0)


def ggx_vndf_pdf(wi, wo, ax, ay):
    """The density (per solid angle of wi) MicrofacetGGXSample actually draws from, whatever `distrib` is
    (microfacet-ggx.h:65-162, 247-286): MicrofacetSampleStretched draws a normal m from the GTR2 distribution of visible
    normals G1o (m.wo) D(m) / cos_o and wi is wo's mirror image about m, so p(wi) = G1o D(m) / (4 cos_o).  That holds for
    every wi with wi.z + wo.z > 0 (m.z > 0), below the surface as well: the sampler does not reject such wi."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    ok = (wo[..., 2] > 0) & (wi[..., 2] + wo[..., 2] > 0)
    wi_, wo_ = np.where(ok[..., None], wi, [0.0, 0.0, 1.0]), np.where(ok[..., None], wo, [0.0, 0.0, 1.0])
    D, G1o, _, _ = _ggx_parts(wi_, wo_, np.asarray(ax, np.float64), np.asarray(ay, np.float64))
    return np.where(ok, G1o * D * 0.25 / wo_[..., 2], 0.0)


def specular_color(wi, wo, color, ior, shared=None, key=None):
    """cycles-principled-shader.cc:54-61: Fresnel tint with the half vector of (wi, wo).  shared, key: a dict that keeps the Fresnel
    term, which does not depend on the colour, under that key (see lobes)"""
    if shared is not None and key in shared:
        fh = shared[key]
    else:
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        f0 = fresnel_dielectric_cos(1.0, ior)
        fh = (fresnel_dielectric_cos(np.sum(h * wo, -1), ior) - f0) / (1.0 - f0)
        if shared is not None:
            shared[key] = fh
    return color * (1 - fh[..., None]) + fh[..., None]


def closure_set(mat, base=None):
    """ParamToBsdf, cycles-principled-shader.cc:244-412, for a material without subsurface: the enabled closures with their
    weights, or None per closure.  base: None (the material's base_color parameter), or the base colours (N, 3) a textured material
    reads at N points (:281-289; tests/_texture_model.py): the colour-valued weights (diffuse, the specular closure's color) then have
    that shape.  Which closures exist must not depend on the point: the enabling tests are asserted to come out alike for all N."""
    sat = lambda v: min(max(float(v), 0.0), 1.0)  # noqa: E731
    base = np.asarray(mat["base_color"] if base is None else base, np.float64)
    metallic, spec, transmission = float(mat["metallic"]), float(mat["specular"]), float(mat["transmission"])
    assert float(mat["subsurface"]) == 0, "the random-walk closure is modelled by tests/_sss_analytic.py, not here"
    diffuse_w = (1 - sat(metallic)) * (1 - sat(transmission))                       # :326-327
    final_transmission = sat(transmission) * (1 - sat(metallic))                    # :328-329
    specular_w = 1 - final_transmission                                             # :330
    out = dict(diffuse=None, specular=None, clearcoat=None)
    if base.ndim == 2:
        bright = base.mean(1) > CUT_OFF
        assert bright.all() or not bright.any(), "the diffuse closure exists for some texels and not for others"
        if bright.all() and diffuse_w > CUT_OFF:                                    # :338-342, per point
            out["diffuse"] = base * diffuse_w
        if specular_w > CUT_OFF and (spec > CUT_OFF or metallic > CUT_OFF):         # :374-394, per point
            ior = 2.0 / (1.0 - np.sqrt(max(0.08 * spec, 0.0))) - 1.0
            aspect = np.sqrt(max(1.0 - float(mat["anisotropic"]) * 0.9, 0.0))
            r2 = float(mat["roughness"]) ** 2
            y = base @ Y_WEIGHT
            rho_tint = np.where(y[:, None] > 0, base / np.where(y > 0, y, 1.0)[:, None], 0.0)
            tint = float(mat["specular_tint"])
            color = (1 - metallic) * (0.08 * spec * ((1 - tint) * np.ones(3) + tint * rho_tint)) + metallic * base
            out["specular"] = dict(weight=specular_w, ax=r2 / aspect, ay=r2 * aspect, ior=ior, color=color)
        cc = float(mat["clearcoat"])
        if cc > CUT_OFF:                                                            # :397-409
            out["clearcoat"] = dict(weight=0.25 * cc, alpha=float(mat["clearcoat_roughness"]) ** 2, ior=1.5, color=np.full(3, 0.04))
        return out
    if base.mean() > CUT_OFF and diffuse_w > CUT_OFF:                               # :338-342 (subsurface == 0 < cut-off)
        out["diffuse"] = base * diffuse_w
    if specular_w > CUT_OFF and (spec > CUT_OFF or metallic > CUT_OFF):             # :374-394
        ior = 2.0 / (1.0 - np.sqrt(max(0.08 * spec, 0.0))) - 1.0
        aspect = np.sqrt(max(1.0 - float(mat["anisotropic"]) * 0.9, 0.0))
        r2 = float(mat["roughness"]) ** 2
        y = float(Y_WEIGHT @ base)
        rho_tint = base / y if y > 0 else np.zeros(3)
        tint = float(mat["specular_tint"])
        rho_specular = (1 - tint) * np.ones(3) + tint * rho_tint
        color = (1 - metallic) * (0.08 * spec * rho_specular) + metallic * base
        out["specular"] = dict(weight=specular_w, ax=r2 / aspect, ay=r2 * aspect, ior=ior, color=color)
    cc = float(mat["clearcoat"])
    if cc > CUT_OFF:                                                                # :397-409
        out["clearcoat"] = dict(weight=0.25 * cc, alpha=float(mat["clearcoat_roughness"]) ** 2, ior=1.5, color=np.full(3, 0.04))
    return out


def selection_weights(cl, wo, shared=None):
    """FetchClosureSampleWeight, :63-112 (Q7): (w_diffuse, w_specular, w_clearcoat) per wo (...,3), each the luminance of the
    closure's weight x SpecularColor(refl, wo) with refl = wo mirrored about the normal, normalised to sum 1.  Colour-valued weights
    per point (closure_set with base (N, 3)) must broadcast against wo's leading shape."""
    wo = np.asarray(wo, np.float64)
    refl = wo * np.array([-1.0, -1.0, 1.0])
    zero = np.zeros(wo.shape[:-1])
    if cl["diffuse"] is not None and cl["diffuse"].ndim > 1:
        wd = zero + cl["diffuse"] @ Y_WEIGHT
    else:
        wd = zero + (float(Y_WEIGHT @ cl["diffuse"]) if cl["diffuse"] is not None else 0.0)
    ws = wc = zero
    if cl["specular"] is not None:
        sp = cl["specular"]
        ws = (sp["weight"] * specular_color(refl, wo, sp["color"], sp["ior"], shared, "select specular")) @ Y_WEIGHT
    if cl["clearcoat"] is not None:
        c = cl["clearcoat"]
        wc = (c["weight"] * specular_color(refl, wo, c["color"], c["ior"], shared, "select clearcoat")) @ Y_WEIGHT
    s = wd + ws + wc
    assert np.all(s > 0), "a receiver with no closure at all"
    return wd / s, ws / s, wc / s


def lobes(cl, wi, wo, sel=None, parts=False, shared=None):
    """EvalBsdf (:114-155) and what SampleBsdf (:169-242) draws, per pair of local directions (...,3):
      f       the sum of the enabled closures, (...,3)
      q_rep   the pdf the shader reports, sum_k w_k pdf_k (GGX and clearcoat with Q15's extra 1 / cos_i)
      p_true  the density wi is actually drawn from, sum_k w_k p_k: Lambert cos_i / pi, GGX and the clearcoat the GTR2
              density of ggx_vndf_pdf at their own alpha (the clearcoat REPORTS the GTR1 pdf but is SAMPLED from GTR2).
    wi may lie below the surface (the GGX sampler can put it there): the GGX closures are then 0, while LambertBrdfPdf
    (lambert.h:11-20) still returns f = 1 / pi and the NEGATIVE pdf cos_i / pi.
    parts=True: the clearcoat's share of f is returned as a fourth value.
    shared: a dict that keeps the GGX and Fresnel terms, which do not depend on any colour, between calls for closure sets that differ in their
    colours alone, at the same wi and wo."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    shared = {} if shared is None else shared
    wd, ws, wc = sel if sel is not None else selection_weights(cl, wo, shared)
    shape = np.broadcast(wi[..., 0], wo[..., 0]).shape
    f, q, p = np.zeros(shape + (3,)), np.zeros(shape), np.zeros(shape)
    ci = np.broadcast_to(wi[..., 2], shape)
    if cl["diffuse"] is not None:
        f = f + cl["diffuse"] / np.pi
        q = q + wd * ci / np.pi
        p = p + wd * np.maximum(ci, 0.0) / np.pi
    if cl["specular"] is not None:
        sp = cl["specular"]
        if "specular" not in shared:
            shared["specular"] = ggx_eval(wi, wo, sp["ax"], sp["ay"], 2) + (ggx_vndf_pdf(wi, wo, sp["ax"], sp["ay"]),)
        g, pdf, drawn = shared["specular"]
        f = f + sp["weight"] * specular_color(wi, wo, sp["color"], sp["ior"], shared, "tint specular") * g[..., None]
        q = q + ws * pdf
        p = p + ws * drawn
    if cl["clearcoat"] is not None:
        c = cl["clearcoat"]
        if "clearcoat" not in shared:
            shared["clearcoat"] = ggx_eval(wi, wo, c["alpha"], c["alpha"], 1) + (ggx_vndf_pdf(wi, wo, c["alpha"], c["alpha"]),)
        g, pdf, drawn = shared["clearcoat"]
        f_cc = c["weight"] * specular_color(wi, wo, c["color"], c["ior"], shared, "tint clearcoat") * g[..., None]
        f = f + f_cc
        q = q + wc * pdf
        p = p + wc * drawn
    else:
        f_cc = np.zeros_like(f)
    return (f, q, p, f_cc) if parts else (f, q, p)


def lobe_width(cl):
    """the narrowest GGX alpha of the set (the angular scale on which f and the pdfs vary near the mirror direction), or None"""
    a = []
    if cl["specular"] is not None:
        a += [cl["specular"]["ax"], cl["specular"]["ay"]]
    if cl["clearcoat"] is not None:
        a += [cl["clearcoat"]["alpha"]]
    return min(a) if a else None


# ------------------------------------------------------------------------------------------------- ray casting (float64)
def _tris(S: Scene):
    out = []
    for mi, m in enumerate(S.meshes):
        v = np.asarray(m.verts, np.float64)
        for fi, f in enumerate(np.asarray(m.faces)):
            out.append((mi, fi, v[f[0]], v[f[1]], v[f[2]]))
    return out


def cast(S: Scene, org, dirs):
    """closest hit of rays (org (3,), dirs (N,3)) over all triangles in float64: (mesh, face, t, front) per ray;
    mesh = -1 for a miss.  front: the ray meets the face against its geometric normal."""
    tris = _tris(S)
    v0 = np.array([t[2] for t in tris]); e1 = np.array([t[3] for t in tris]) - v0; e2 = np.array([t[4] for t in tris]) - v0
    d = dirs[:, None, :]
    p = np.cross(d, e2[None])
    det = np.sum(e1[None] * p, -1)
    inv = 1.0 / np.where(det != 0, det, 1.0)
    s = org[None, None, :] - v0[None]
    u = np.sum(s * p, -1) * inv
    q = np.cross(s, e1[None])
    v = np.sum(d * q, -1) * inv
    t = np.sum(e2[None] * q, -1) * inv
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(ok, t, np.inf)
    k = np.argmin(t, 1)
    tk = t[np.arange(len(dirs)), k]
    hit = np.isfinite(tk)
    mesh = np.where(hit, np.array([tr[0] for tr in tris])[k], -1)
    face = np.where(hit, np.array([tr[1] for tr in tris])[k], -1)
    ng = np.cross(e1, e2)[k]
    front = np.sum(dirs * ng, -1) < 0
    return mesh, face, tk, front


# ------------------------------------------------------------------------------------------------- camera (render.cc:132-171)
class Camera:
    """RenderingTile's pinhole camera in float64 from the scene's float32 AABB (pbr_oracle.c make_camera / camera_ray)"""

    def __init__(self, bmin, bmax, width, height):
        bmin, bmax = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
        if bmax[0] - bmin[0] > bmax[1] - bmin[1]:
            hs = bmax[0] - bmin[0]
            vs = hs * height / width
        else:
            vs = bmax[1] - bmin[1]
            hs = vs * width / height
        self.org = np.array([(bmax[0] + bmin[0]) * 0.5, (bmax[1] + bmin[1]) * 0.5, bmax[2] + hs * 0.5 * np.sqrt(3.0)])
        self.xc, self.yc, self.zc = (bmax[0] + bmin[0]) * 0.5 - hs * 0.5, (bmax[1] + bmin[1]) * 0.5 + vs * 0.5, bmax[2]
        self.dx, self.dy = hs / width, vs / height
        self.width, self.height = width, height

    def dirs(self, px, py, jx, jy):
        """unit directions through image positions (px + jx, py + jy), jitter j in [0,1)"""
        tgt = np.stack([self.xc + self.dx * (px + jx), self.yc - self.dy * (py + jy), np.full(np.shape(px + jx), self.zc)], -1)
        d = tgt - self.org
        return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------- polygon clipping (2D)
def _clip(poly, a, b, c):
    """Sutherland-Hodgman: keep the part of convex polygon poly (list of (u,w)) with a*u + b*w + c >= 0"""
    out = []
    n = len(poly)
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        fp, fq = a * p[0] + b * p[1] + c, a * q[0] + b * q[1] + c
        if fp >= 0:
            out.append(p)
        if (fp >= 0) != (fq >= 0):
            s = fp / (fp - fq)
            out.append((p[0] + s * (q[0] - p[0]), p[1] + s * (q[1] - p[1])))
    return out if len(out) >= 3 else []


def _hull(pts):
    """convex hull, counter-clockwise (monotone chain)"""
    pts = sorted(set(pts))
    if len(pts) < 3:
        return pts

    def cr(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lo, hi = [], []
    for p in pts:
        while len(lo) >= 2 and cr(lo[-2], lo[-1], p) <= 0:
            lo.pop()
        lo.append(p)
    for p in reversed(pts):
        while len(hi) >= 2 and cr(hi[-2], hi[-1], p) <= 0:
            hi.pop()
        hi.append(p)
    return lo[:-1] + hi[:-1]


def subtract(poly, hull):
    """P \\ Q for convex P and convex CCW Q: piece k = P outside edge k of Q and inside edges 0..k-1 (disjoint, convex)"""
    if len(hull) < 3:
        return [poly]
    pieces, rest = [], poly
    for k in range(len(hull)):
        p, q = hull[k], hull[(k + 1) % len(hull)]
        # left of p->q (inside Q): (q-p) x (y-p) >= 0  ->  a u + b w + c >= 0
        a, b = -(q[1] - p[1]), (q[0] - p[0])
        c = -(a * p[0] + b * p[1])
        out = _clip(rest, -a, -b, -c)
        if out:
            pieces.append(out)
        rest = _clip(rest, a, b, c)
        if not rest:
            break
    return pieces


# ------------------------------------------------------------------------------------------------- the expectation
def gauss_legendre01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1), 0.5 * w


class Textured:
    """A receiver mesh with a base-colour texture (H, W, C): the colour and the texture coordinates its points read, through
    tests/_texture_model.py.  continuous: the faces agree on the texcoords of every vertex they share (a face without texcoord ids
    reads its own barycentrics, which jump across its edges)."""

    def __init__(self, mesh, tex):
        import _texture_model as TM
        self.TM, self.MUTANTS, self.mesh = TM, TM.MUTANTS, mesh
        self.tex = np.asarray(tex, np.float64)
        if self.tex.ndim == 2:
            self.tex = self.tex[..., None]
        faces = np.asarray(mesh.faces)
        fi = np.repeat(np.arange(len(faces)), 3)
        tu, tv = TM.texcoord(mesh, fi, np.tile([0.0, 1.0, 0.0], len(faces)), np.tile([0.0, 0.0, 1.0], len(faces)))
        seen, self.continuous = {}, True
        for vid, c in zip(faces.ravel(), zip(tu, tv)):
            self.continuous &= np.allclose(seen.setdefault(int(vid), c), c, atol=1e-12)

    def coords(self, x):
        face, u, v = self.TM.barycentrics(self.mesh, x)
        return self.TM.texcoord(self.mesh, face, u, v)

    def base_color(self, x, mutant=None):
        return self.TM.base_color(self.mesh, self.tex, x, mutant)


def texel_pieces(tx: Textured, S: Scene, cam, xs, ys):
    """Where a bilinear texture kinks inside pixel footprints.  The model's fetch is bilinear between the texel lines W u = 0 .. W and
    H v = 0 .. H (the clamp begins at the outer ones), and within a face the texcoords are affine in the receiver point, which is
    affine in the jitter for a receiver parallel to the image plane: per pixel the lines are straight in jitter space.
    Returns ({pixel index: convex pieces of the unit jitter square cut along every line that crosses it}, affine (P,) bool: the
    fourth corner of the footprint has the texcoords the other three predict -- False where a jump of the texcoords, or a receiver
    that is not parallel to the image plane, breaks that; such pixels are not cut)."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    cj = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    d = cam.dirs(xs[:, None], ys[:, None], cj[:, 0], cj[:, 1]).reshape(-1, 3)
    m, _, t, _ = cast(S, cam.org, d)
    assert np.all(m == S.receiver)
    c = np.stack(tx.coords(cam.org + t[:, None] * d), -1).reshape(len(xs), 4, 2)
    affine = np.abs(c[:, 1] + c[:, 2] - c[:, 0] - c[:, 3]).max(1) < 1e-9
    pieces = {}
    square = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    for k, n in enumerate((tx.tex.shape[1], tx.tex.shape[0])):
        lo, hi = c[:, :, k].min(1), c[:, :, k].max(1)
        for line in range(n + 1):
            for p in np.nonzero(affine & (lo < line / n - 1e-9) & (hi > line / n + 1e-9))[0]:
                c0, a, b = c[p, 0, k], c[p, 1, k] - c[p, 0, k], c[p, 2, k] - c[p, 0, k]
                cut = []
                for poly in pieces.get(p, [square]):
                    cut += [q for q in (_clip(poly, -a, -b, line / n - c0), _clip(poly, a, b, c0 - line / n)) if q]
                pieces[p] = cut
    return pieces, affine


class Expectation:
    """E(x) for points x on the receiver seen along camera directions, per RGB channel."""

    def __init__(self, S: Scene, order=5, physical_mis=False, lobe=None, alts=()):
        """physical_mis: w_nee + w_bsdf replaced by 1.  lobe: see __call__'s refinement.  alts: mutations of the model that the
        tests must reject, each evaluated alongside E at the same nodes and returned as three more channels, in this order:
        "honest_pdf" (p_true := q_rep, a shader whose reported pdf were its sampling density), "clearcoat_unscaled" (the
        clearcoat lobe without microfacet-ggx.h:236's 0.25).
        A receiver whose material carries base_color_tex_id reads its base colour per point x through tests/_texture_model.py, and
        the closure set, the selection weights and both pdfs follow it; alts may then also name that model's mutants
        (_texture_model.MUTANTS): the expectation of a renderer that read the texture that way."""
        import _texture_model as TM
        assert all(a in ("honest_pdf", "clearcoat_unscaled") + TM.MUTANTS for a in alts)
        self.S, self.order, self.physical_mis, self.alts = S, order, physical_mis, tuple(alts)
        self.channels = 3 * (1 + len(self.alts))
        rm = S.meshes[S.receiver]
        tex_id = rm.material["base_color_tex_id"]
        self.textured = None if tex_id == TM.NONE else Textured(rm, S.textures[tex_id])
        assert self.textured is not None or not any(a in TM.MUTANTS for a in alts)
        if self.textured is not None:
            texels = np.asarray(self.textured.tex, np.float64)
            # every texel enables the same closures (closure_set asserts it); a bilinear mix of texels then does as well
            self.closures = closure_set(rm.material, TM.fetch(texels, *np.meshgrid(np.arange(texels.shape[1]) / texels.shape[1],
                                                                                   np.arange(texels.shape[0]) / texels.shape[0])).reshape(-1, 3))
        else:
            self.closures = closure_set(rm.material)
        self.lobe = lobe                                   # None: triangles are refined by 1 / d^2 alone
        self.width = lobe_width(self.closures) if lobe else None
        rv = np.asarray(S.meshes[S.receiver].verts, np.float64)
        rf = np.asarray(S.meshes[S.receiver].faces)
        n = np.cross(rv[rf[:, 1]] - rv[rf[:, 0]], rv[rf[:, 2]] - rv[rf[:, 0]])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert np.allclose(n, n[0], atol=1e-12), "the receiver must be planar"
        self.n_geo = n[0]
        # the light table: every emitting face, p_A = max(Le) / sum(max(Le) area)  (Q10)
        faces, total = [], 0.0
        for m in S.meshes:
            if m.emission is None:
                continue
            v = np.asarray(m.verts, np.float64)
            for k, f in enumerate(np.asarray(m.faces)):
                p0, p1, p2 = v[f[0]], v[f[1]], v[f[2]]
                ng = np.cross(p1 - p0, p2 - p0)
                area = 0.5 * np.linalg.norm(ng)
                le = np.asarray(m.emission[k], np.float64)
                if m.normals is not None:
                    ns = np.asarray(m.normals, np.float64)[f]
                    assert np.allclose(ns, ns[0], atol=1e-12), "shading normals must be constant per face (kFront is a half-plane)"
                    ns = ns[0] / np.linalg.norm(ns[0])
                else:
                    ns = ng / np.linalg.norm(ng)
                faces.append(dict(p=(p0, p1, p2), ng=ng / np.linalg.norm(ng), ns=ns, area=area, le=le))
                total += le.max() * area
        for fc in faces:
            fc["pA"] = fc["le"].max() / total
            # 2D frame of the face's plane
            e1 = fc["p"][1] - fc["p"][0]
            e1 = e1 / np.linalg.norm(e1)
            fc["e"] = (fc["p"][0], e1, np.cross(fc["ng"], e1))
            fc["uv"] = [self._to2(fc, p) for p in fc["p"]]
        self.faces = faces
        self.occ = [np.asarray(S.meshes[i].verts, np.float64) for i in S.occluders]

    @staticmethod
    def _to2(fc, p):
        o, e1, e2 = fc["e"]
        return (float(np.dot(p - o, e1)), float(np.dot(p - o, e2)))

    def _pieces(self, x, n_r, fc):
        """convex pieces (2D, in fc's frame) of the light face visible from x, each tagged with kFront(n_s)"""
        o, e1, e2 = fc["e"]
        if np.dot(x - o, fc["ng"]) <= 0:           # cos_l <= 0 over the whole face: NEE's hemisphere test, and never kFront
            return []
        poly = list(fc["uv"])
        # receiver hemisphere (y - x).n_r > 0
        poly = _clip(poly, float(np.dot(e1, n_r)), float(np.dot(e2, n_r)), float(np.dot(o - x, n_r)))
        if not poly:
            return []
        pieces = [poly]
        phx = float(np.dot(x - o, fc["ng"]))
        for ov in self.occ:
            phv = (ov - o) @ fc["ng"]
            ratio = phv / phx
            if np.all(ratio >= 1):                 # the occluder is not between x and the light's plane
                continue
            assert np.all((ratio > 0) & (ratio < 1)), "occluder straddles x or the light's plane: the hull rule does not hold"
            t = phx / (phx - phv)
            proj = x + t[:, None] * (ov - x)
            hull = _hull([(float(np.dot(p - o, e1)), float(np.dot(p - o, e2))) for p in proj])
            pieces = [q for p in pieces for q in subtract(p, hull)]
        # kFront on the light needs w.n_s < 0 as well:  (y - x).n_s < 0
        ns = fc["ns"]
        a, b, c = float(np.dot(e1, ns)), float(np.dot(e2, ns)), float(np.dot(o - x, ns))
        out = []
        for p in pieces:
            fr = _clip(p, -a, -b, -c)
            bk = _clip(p, a, b, c)
            if fr:
                out.append((fr, True))
            if bk:
                out.append((bk, False))
        return out

    def __call__(self, x, wo, order=None):
        """x: (N,3) points on the receiver, wo: (N,3) unit directions towards the camera.  Returns (N,3)."""
        order = order or self.order
        x, wo = np.asarray(x, np.float64), np.asarray(wo, np.float64)
        N = len(x)
        n_r = np.where((wo @ self.n_geo)[:, None] > 0, self.n_geo, -self.n_geo)   # ez: the side the camera sees (kBack flips)
        gs, gw = gauss_legendre01(order)
        S_, T_ = np.meshgrid(gs, gs, indexing="ij")
        W_ = np.outer(gw, gw).ravel()
        S_, T_ = S_.ravel(), T_.ravel()
        out = np.zeros((N, self.channels))
        cl_pts = None
        if self.textured is not None:
            # the closure set per point: the model's, then one per texture mutant among the alts
            mat = self.S.meshes[self.S.receiver].material
            cl_pts = {a: closure_set(mat, self.textured.base_color(x, a)) for a in (None,) + self.alts if a is None or a in self.textured.MUTANTS}
        for fi, fc in enumerate(self.faces):
            o, e1, e2 = fc["e"]
            owner, tri, front = [], [], []
            for i in range(N):
                for poly, fr in self._pieces(x[i], n_r[i], fc):
                    for k in range(1, len(poly) - 1):
                        owner.append(i)
                        tri.append((poly[0], poly[k], poly[k + 1]))
                        front.append(fr)
            if not owner:
                continue
            owner = np.asarray(owner)
            tri = np.asarray(tri)                                     # (M,3,2)
            front = np.asarray(front)
            # 1/d^2 peaks near the foot of x on the light's plane: split a triangle into 4 while its longest edge exceeds
            # REFINE x its distance from x (estimated from the distance to the plane and the distance to the centroid less the edge),
            # at most MAX_SPLITS times
            # A GGX lobe of width alpha varies on the angular scale alpha around the mirror direction and more slowly away from
            # it: with lobe = c the triangle's angular size (edge / distance) is also held below c x (alpha + its angle from the mirror
            # direction / 2)
            h = np.abs((x - o) @ fc["ng"])
            x2 = np.stack([(x - o) @ e1, (x - o) @ e2], -1)
            mirror = 2.0 * np.sum(wo * n_r, -1, keepdims=True) * n_r - wo
            for _ in range(MAX_SPLITS):
                edge = np.max(np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=-1), -1)
                cen = tri.mean(1)
                r = np.linalg.norm(cen - x2[owner], axis=-1)
                near = np.sqrt(h[owner] ** 2 + np.maximum(r - edge, 0.0) ** 2)
                big = edge > REFINE * near
                if self.width is not None:
                    dc = o + cen[:, :1] * e1 + cen[:, 1:] * e2 - x[owner]
                    dist = np.linalg.norm(dc, axis=-1)
                    ang = np.arccos(np.clip(np.sum(dc * mirror[owner], -1) / dist, -1.0, 1.0))
                    big |= edge > self.lobe * (self.width + 0.5 * np.maximum(ang - edge / near, 0.0)) * near
                if not big.any():
                    break
                t4 = tri[big]
                a, b, c = t4[:, 0], t4[:, 1], t4[:, 2]
                ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
                sub = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
                tri = np.concatenate([tri[~big], sub])
                owner = np.concatenate([owner[~big], np.tile(owner[big], 4)])
                front = np.concatenate([front[~big], np.tile(front[big], 4)])
            for c0 in range(0, len(tri), CHUNK):
                self._integrate(fc, tri[c0:c0 + CHUNK], owner[c0:c0 + CHUNK], front[c0:c0 + CHUNK], x, n_r, wo, S_, T_, W_, out, cl_pts)
        return out

    def _lobes(self, wi, wo):
        """(f, q_rep, p_true, the clearcoat's share of f) for local directions (M,Q,3): the receiver's closure set"""
        return lobes(self.closures, wi, wo, parts=True)

    def _integrate(self, fc, tri, owner, front, x, n_r, wo, S_, T_, W_, out, cl_pts=None):
        o, e1, e2 = fc["e"]
        A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
        area2 = np.abs((B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0]))
        # collapsed square -> triangle: y = A + s (B - A) + s t (C - B), dA = area2 * s ds dt
        uv = A[:, None] + S_[None, :, None] * (B - A)[:, None] + (S_ * T_)[None, :, None] * (C - B)[:, None]
        wq = area2[:, None] * S_[None] * W_[None]
        y = o + uv[..., :1] * e1 + uv[..., 1:] * e2               # (M,Q,3)
        xm, nrm, wom = x[owner][:, None], n_r[owner][:, None], wo[owner][:, None]
        dv = y - xm
        d2 = np.sum(dv * dv, -1)
        w = dv / np.sqrt(d2)[..., None]
        cos_p = np.sum(w * nrm, -1)
        cos_l = -np.sum(w * fc["ng"], -1)
        ns_dot = np.abs(np.sum(w * fc["ns"], -1))
        pA = fc["pA"]
        q_nee = pA * d2 / (cos_l * cos_p)
        q_light = pA * d2 / ns_dot
        ex, ey = branchless_onb(nrm)                             # the shader's own tangent frame: alpha_x lies along ex
        loc = lambda v: np.stack([np.sum(v * ex, -1), np.sum(v * ey, -1), np.sum(v * nrm, -1)], -1)  # noqa: E731
        wi_l, wo_l = loc(w), loc(np.broadcast_to(wom, w.shape))

        def paths(f, q_bsdf, p_true):
            """what both sampling strategies carry per unit f: (NEE's share, the BSDF-sampled path's share, that path's cosine)"""
            # the BSDF-sampled path: wi ~ p_true carries f cos / q_rep  ->  f cos (p_true / q_rep); Lambert alone: ratio 1,
            # GGX alone (Q15): ratio cos
            bsdf_cos = cos_p * p_true / q_bsdf
            if self.physical_mis:
                w_nee = np.ones_like(q_nee)
                w_bsdf = np.zeros_like(q_nee)
            else:
                w_nee = q_nee ** 2 / (q_nee ** 2 + q_bsdf ** 2)
                w_bsdf = np.where(front[:, None], q_bsdf ** 2 / (q_bsdf ** 2 + q_light ** 2), 0.0)
            return cos_p * cos_l / d2 * w_nee, cos_l / d2 * w_bsdf, bsdf_cos

        def at_owner(cl):
            """a per-point closure set (closure_set with base (N, 3)) at this chunk's triangles, shaped (M, 1, 3) for lobes()"""
            cl = dict(cl)
            if cl["diffuse"] is not None:
                cl["diffuse"] = cl["diffuse"][owner][:, None]
            if cl["specular"] is not None:
                cl["specular"] = dict(cl["specular"], color=cl["specular"]["color"][owner][:, None])
            return cl
        if cl_pts is None:
            f, q_bsdf, p_true, f_cc = self._lobes(wi_l, wo_l)
        else:
            shared = {}                                          # (wo is one direction per triangle: its selection weights are taken once)
            pick = lambda cl: selection_weights(cl, wo_l[:, :1], shared)  # noqa: E731
            cl = at_owner(cl_pts[None])
            f, q_bsdf, p_true, f_cc = lobes(cl, wi_l, wo_l, sel=pick(cl), parts=True, shared=shared)
        k_nee, k_bsdf, bsdf_cos = paths(f, q_bsdf, p_true)
        g = [(k_nee + bsdf_cos * k_bsdf)[..., None] * f]
        for a in self.alts:
            if a == "honest_pdf":
                g.append((k_nee + cos_p * k_bsdf)[..., None] * f)
            elif a == "clearcoat_unscaled":
                g.append((k_nee + bsdf_cos * k_bsdf)[..., None] * (f + 3.0 * f_cc))
            else:                                                # a texture mutant: its own closure set per point, the same transport
                cl = at_owner(cl_pts[a])
                fa, qa, pa = lobes(cl, wi_l, wo_l, sel=pick(cl), shared=shared)
                ka_nee, ka_bsdf, a_cos = paths(fa, qa, pa)
                g.append((ka_nee + a_cos * ka_bsdf)[..., None] * fa)
        val = np.concatenate([np.sum(gi * wq[..., None], 1) * fc["le"] for gi in g], -1)
        np.add.at(out, owner, val)


# ------------------------------------------------------------------------------------------------- Student's t
def _betacf(a, b, x):
    """continued fraction of the regularised incomplete beta function (modified Lentz)"""
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 500):
        for num in (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)), -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))):
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-15:
            break
    return h


def betainc(a, b, x):
    """regularised incomplete beta I_x(a, b)"""
    import math
    if x <= 0.0 or x >= 1.0:
        return float(x >= 1.0)
    lf = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)
    if x < (a + 1.0) / (a + b + 2.0):
        return math.exp(lf) * _betacf(a, b, x) / a
    return 1.0 - math.exp(lf) * _betacf(b, a, 1.0 - x) / b


def student_t_two_sided(x, dof):
    """P(|T| > x) for Student's t with dof degrees of freedom"""
    return betainc(dof / 2.0, 0.5, dof / (dof + x * x))


def student_t_bar(p_two_sided, dof):
    """x with P(|T| > x) = p_two_sided (bisection; P is monotone in x)"""
    lo, hi = 0.0, 1e3
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if student_t_two_sided(mid, dof) > p_two_sided:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ------------------------------------------------------------------------------------------------- per-pixel classes
PIX_MIXED, PIX_RECEIVER, PIX_ZERO, PIX_LIGHT = 0, 1, 2, 3


def classify_and_expect(S: Scene, cam: Camera, expectation: Expectation, sub=2, probe=6):
    """Per pixel: its class (from a probe x probe grid over the slightly widened footprint, float64 rays), the exact value of
    PIX_LIGHT / PIX_ZERO pixels and, for PIX_RECEIVER pixels, the mean of E over the footprint (the jitter is uniform over
    the pixel) by a sub x sub Gauss-Legendre rule (exact for polynomials of degree 2 sub - 1 in each direction); receiver
    pixels whose nodes spread by more than STEEP (next to an emitter) become PIX_MIXED.  tests/test_analytic_radiance.py
    checks the rule against an 8 x 8 one.
    Returns (cls (H,W), value (H,W,3), (receiver points, directions to the camera))."""
    W, H = cam.width, cam.height
    py, px = np.mgrid[0:H, 0:W]
    js = np.linspace(-0.02, 1.02, probe)
    jx, jy = np.meshgrid(js, js, indexing="ij")
    d = cam.dirs(px[..., None].astype(np.float64), py[..., None].astype(np.float64), jx.ravel(), jy.ravel())
    mesh, face, t, front = cast(S, cam.org, d.reshape(-1, 3))
    mesh, face, front = mesh.reshape(H, W, -1), face.reshape(H, W, -1), front.reshape(H, W, -1)
    emits = np.array([m.emission is not None for m in S.meshes] + [False])
    cls = np.full((H, W), PIX_MIXED)
    nrep = getattr(expectation, "channels", 3) // 3            # E and the expectation's alternatives, three channels each
    value = np.zeros((H, W, 3 * nrep))
    on_recv = np.all(mesh == S.receiver, -1)
    zero = np.all((mesh < 0) | ~emits[mesh] & (mesh != S.receiver) | emits[mesh] & ~front, -1)
    cls[zero] = PIX_ZERO
    for mi, m in enumerate(S.meshes):
        if m.emission is None:
            continue
        em = np.asarray(m.emission, np.float64)
        for k in range(len(em)):
            same = np.all(em == em[k], 1)
            lit = np.all((mesh == mi) & front & same[np.where(mesh == mi, face, 0)], -1)
            cls[lit] = PIX_LIGHT
            value[lit] = np.tile(em[k], nrep)
    cls[on_recv] = PIX_RECEIVER
    # E over the footprints of the receiver pixels
    ys, xs = np.nonzero(on_recv)
    info = {}
    e, ev, pts, wo = pixel_mean(S, cam, expectation, xs, ys, sub, nodes=True, info=info)
    value[ys, xs] = e
    # where E is steep on the scale of a pixel (right next to an emitter) the rule is not trusted: such pixels are left out
    steep = (ev[..., :3].max(1) - ev[..., :3].min(1)).max(1) > STEEP * np.abs(e[:, :3]).max(1)
    cls[ys[steep], xs[steep]] = PIX_MIXED
    tx = getattr(expectation, "textured", None)
    if tx is not None:
        # a jump of the texcoords (between a face that has them and one that reads its barycentrics) inside the widened footprint
        jump = ~info["affine"]
        if not tx.continuous:
            jump |= np.any(face != face[..., :1], -1)[ys, xs]
        cls[ys[jump], xs[jump]] = PIX_MIXED
    return cls, value, (pts, wo)


def on_receiver(S: Scene, cam: Camera, probe=6):
    """(H,W) bool: the pixels whose whole (slightly widened) footprint sees the receiver, by classify_and_expect's probe rays"""
    W, H = cam.width, cam.height
    py, px = np.mgrid[0:H, 0:W]
    js = np.linspace(-0.02, 1.02, probe)
    jx, jy = np.meshgrid(js, js, indexing="ij")
    d = cam.dirs(px[..., None].astype(np.float64), py[..., None].astype(np.float64), jx.ravel(), jy.ravel())
    return np.all(cast(S, cam.org, d.reshape(-1, 3))[0].reshape(H, W, -1) == S.receiver, -1)


def pixel_mean(S, cam, expectation, xs, ys, sub, nodes=False, info=None):
    """mean of E over the footprints of receiver pixels (xs, ys) by a sub x sub Gauss-Legendre rule; with nodes=True also
    the values at the nodes (P, sub^2, 3), the nodes' receiver points and their directions towards the camera.
    A textured receiver (expectation.textured): E has a kink along every texel line, so a footprint that such lines cross is cut
    along them (texel_pieces) and every piece, fanned into triangles, gets a collapsed n x n rule of its own, n = max(sub, 3) (the
    collapse costs a rule of n points two degrees); the values at the nodes stay those of the uncut rule.  info: a dict that receives texel_pieces' `affine`."""
    g, gw = gauss_legendre01(sub)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    d = cam.dirs(np.asarray(xs, np.float64)[:, None], np.asarray(ys, np.float64)[:, None], gx.ravel(), gy.ravel()).reshape(-1, 3)
    m, _, t, _ = cast(S, cam.org, d)
    assert np.all(m == S.receiver)
    pts = cam.org + t[:, None] * d
    v = expectation(pts, -d).reshape(len(xs), sub * sub, -1)
    e = np.einsum("pqc,q->pc", v, np.outer(gw, gw).ravel())
    tx = getattr(expectation, "textured", None)
    if tx is not None:
        pieces, affine = texel_pieces(tx, S, cam, xs, ys)
        if info is not None:
            info["affine"] = affine
        s, ws = gauss_legendre01(max(sub, 3))
        s_, t_ = (a.ravel() for a in np.meshgrid(s, s, indexing="ij"))
        w_ = np.outer(ws, ws).ravel()
        pi, jx, jy, wq = [], [], [], []
        for p, polys in pieces.items():
            for poly in polys:
                for k in range(1, len(poly) - 1):
                    A, B, C = (np.asarray(q) for q in (poly[0], poly[k], poly[k + 1]))
                    area2 = abs((B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0]))
                    # collapsed square -> triangle, as Expectation._integrate: j = A + s (B - A) + s t (C - B), dj = area2 s ds dt
                    j = A + s_[:, None] * (B - A) + (s_ * t_)[:, None] * (C - B)
                    pi.append(np.full(len(s_), p)); jx.append(j[:, 0]); jy.append(j[:, 1]); wq.append(area2 * s_ * w_)
        if pi:
            pi, jx, jy, wq = (np.concatenate(a) for a in (pi, jx, jy, wq))
            dp = cam.dirs(np.asarray(xs, np.float64)[pi], np.asarray(ys, np.float64)[pi], jx, jy)
            mp, _, tp, _ = cast(S, cam.org, dp)
            assert np.all(mp == S.receiver)
            acc, area = np.zeros_like(e), np.zeros(len(e))
            np.add.at(acc, pi, expectation(cam.org + tp[:, None] * dp, -dp) * wq[:, None])
            np.add.at(area, pi, wq)
            cutp = np.array(sorted(pieces))
            assert np.allclose(area[cutp], 1.0, atol=1e-12), "the pieces do not tile the footprint"
            e[cutp] = acc[cutp]
    return (e, v, pts, -d) if nodes else e
