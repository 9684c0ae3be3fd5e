"""Float64 model of a textured base colour: which texel colour a hit on a triangle mesh reads.  Test infrastructure only, written
from the reference's text and not from the kernels or the oracle:

  cycles-principled-shader.cc:281-301   ParamToBsdf takes base_color from Texture::FetchFloat3(texcoord.x, texcoord.y) when the
                                        material carries base_color_tex_id, else from the base_color parameter
  scene.cc:230-249                      the texcoord of a triangle hit is TriangleMesh::FetchTexcoord(prim_id, u, v), untransformed
  mesh/triangle-mesh.cc:126-156         = Lerp3(t0, t1, t2, u, v) = (1 - u - v) t0 + u t1 + v t2 (pbrlab_math.h:35-38) through the
                                        face's TEXCOORD ids; a face with any id == uint32(-1) yields float2(u, v) itself
  texture.cc:43-68                      FetchFloatN: BilinearFilter without wrapping; channels the image lacks read 0, channels
                                        beyond the n asked for (FetchFloat3: a fourth one) are dropped
  image-utils.cc:99-167                 BilinearFilter: u, v clamped to [0, 1]; px = width * u, py = height * v (NO half-texel
                                        offset, :120-121); x0 = clamp(int(px), 0, width - 1), x1 = min(x0 + 1, width - 1) (:123-131);
                                        dx = px - x0; weights (1-dx)(1-dy) | (1-dx) dy [+y] | dx (1-dy) [+x] | dx dy (:142-146);
                                        texel (x, y) at image[(y * width + x) * channels] (:150-153): rows follow v, columns u

Quirks the model carries (they follow from those lines): the last column is constant over u in [(W-1)/W, 1] (x1 == x0 there), the
first texel alone is reached only at u = 0, and the picture is not symmetric under u -> 1 - u.

u, v are the intersection contract's barycentrics of the face's second and third vertex.

Mutants: one-line departures from the model that the radiance tests must reject (tests/test_texture_radiance.py), selected by
name.  FETCH_MUTANTS act in fetch(), TEXCOORD_MUTANTS in texcoord()."""
import numpy as np

NONE = 0xFFFFFFFF
FETCH_MUTANTS = ("half_texel", "swap_uv", "flip_v", "wrap", "weights_transposed", "nearest", "param_color")
TEXCOORD_MUTANTS = ("corner_order", "vertex_indexed", "fallback_whole_mesh")
MUTANTS = FETCH_MUTANTS + TEXCOORD_MUTANTS


def fetch(tex, u, v, mutant=None, param_color=None):
    """Texture::FetchFloat3 in float64.  tex: (H, W, C) with C in 1..4, u, v: (...,) -> (..., 3).
    mutant: None or one of FETCH_MUTANTS; param_color: the material's base_color parameter (the `param_color` mutant returns it)."""
    assert mutant is None or mutant in FETCH_MUTANTS, mutant
    tex = np.asarray(tex, np.float64)
    if tex.ndim == 2:
        tex = tex[..., None]
    H, W, C = tex.shape
    u, v = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))
    if mutant == "param_color":
        return np.broadcast_to(np.asarray(param_color, np.float64), u.shape + (3,)).copy()
    if mutant == "swap_uv":
        u, v = v, u
    if mutant == "flip_v":
        v = 1.0 - v
    wrap = mutant == "wrap"
    uu, vv = (u - np.floor(u), v - np.floor(v)) if wrap else (np.clip(u, 0.0, 1.0), np.clip(v, 0.0, 1.0))    # :105-118
    px, py = W * uu, H * vv                                                                                  # :120-121
    if mutant == "half_texel":
        px, py = px - 0.5, py - 0.5
    fx, fy = np.floor(px), np.floor(py)                      # int(px) truncates; px >= 0 in the model itself
    x0, y0 = np.clip(fx, 0, W - 1).astype(int), np.clip(fy, 0, H - 1).astype(int)                           # :123-124
    if wrap:
        x1, y1 = np.where(x0 + 1 >= W, 0, x0 + 1), np.where(y0 + 1 >= H, 0, y0 + 1)                          # :129, :135
    else:
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)                                        # :131, :137
    dx, dy = px - x0, py - y0                                                                                # :139-140
    if mutant == "half_texel":
        dx, dy = np.clip(dx, 0.0, 1.0), np.clip(dy, 0.0, 1.0)  # (a centred lookup clamps at the border texels' centres)
    if mutant == "nearest":
        dx, dy = np.zeros_like(dx), np.zeros_like(dy)
    w00, w_py, w_px, w11 = (1 - dx) * (1 - dy), (1 - dx) * dy, dx * (1 - dy), dx * dy                        # :142-146
    if mutant == "weights_transposed":
        w_py, w_px = w_px, w_py
    out = (tex[y0, x0] * w00[..., None] + tex[y1, x0] * w_py[..., None] + tex[y0, x1] * w_px[..., None]      # :150-166
           + tex[y1, x1] * w11[..., None])
    rgb = np.zeros(u.shape + (3,))                           # texture.cc:50-56: missing channels read 0, a fourth is not asked for
    rgb[..., :min(C, 3)] = out[..., :min(C, 3)]
    return rgb


def texcoord(mesh, face, u, v, mutant=None):
    """TriangleMesh::FetchTexcoord in float64.  mesh: anything with .faces (F, 3), .texcoords (T, 2) or None and .texcoord_ids (F, 3)
    or None; face: (...,) int, u, v: (...,) the barycentrics of the face's second and third vertex -> (tu, tv), each (...,).
    A mesh without texcoord ids has none on any face (every face falls back to (u, v))."""
    assert mutant is None or mutant in TEXCOORD_MUTANTS, mutant
    face = np.asarray(face)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if mesh.texcoord_ids is None:
        return u, v
    tc = np.asarray(mesh.texcoords, np.float64)
    ids = np.asarray(mesh.texcoord_ids, np.int64)
    if mutant == "vertex_indexed":
        ids = np.where(ids == NONE, NONE, np.asarray(mesh.faces, np.int64))
    missing = np.any(ids == NONE, 1)                         # :130-133, any of the three
    if mutant == "fallback_whole_mesh":
        missing = np.full(len(ids), missing.any())
    safe = np.where(ids == NONE, 0, ids)[face]               # (..., 3)
    t0, t1, t2 = tc[safe[..., 0]], tc[safe[..., 1]], tc[safe[..., 2]]
    if mutant == "corner_order":
        t1, t2 = t2, t1
    lerp = (1.0 - u - v)[..., None] * t0 + u[..., None] * t1 + v[..., None] * t2                             # pbrlab_math.h:37
    if mutant == "corner_order":
        fb = np.stack([v, u], -1)                            # (the fallback with the corners exchanged as well)
    else:
        fb = np.stack([u, v], -1)
    out = np.where(missing[face][..., None], fb, lerp)
    return out[..., 0], out[..., 1]


def barycentrics(mesh, x):
    """For points x (N, 3) on the planar mesh: (face, u, v) with u, v the barycentrics of the face's second and third vertex, the
    face being the one that holds x (the one x is deepest inside, so that points on a shared edge go to either side consistently
    with a continuous texcoord)"""
    x = np.asarray(x, np.float64)
    vv = np.asarray(mesh.verts, np.float64)
    best, bu, bv, bf = np.full(len(x), -np.inf), np.zeros(len(x)), np.zeros(len(x)), np.zeros(len(x), int)
    for fi, f in enumerate(np.asarray(mesh.faces)):
        p0, e1, e2 = vv[f[0]], vv[f[1]] - vv[f[0]], vv[f[2]] - vv[f[0]]
        n = np.cross(e1, e2)
        d = x - p0
        u = np.cross(d, e2) @ n / (n @ n)
        v = np.cross(e1, d) @ n / (n @ n)
        inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
        take = inside > best
        best, bu, bv, bf = np.where(take, inside, best), np.where(take, u, bu), np.where(take, v, bv), np.where(take, fi, bf)
    assert (best > -1e-9).all(), "a point off the mesh"
    return bf, bu, bv


def base_color(mesh, tex, x, mutant=None):
    """the base colour ParamToBsdf reads at points x (N, 3) of a mesh whose material carries the texture `tex`: (N, 3)"""
    face, u, v = barycentrics(mesh, x)
    tu, tv = texcoord(mesh, face, u, v, mutant if mutant in TEXCOORD_MUTANTS else None)
    return fetch(tex, tu, tv, mutant if mutant in FETCH_MUTANTS else None, mesh.material["base_color"])
