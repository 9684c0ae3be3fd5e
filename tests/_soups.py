"""Adversarial primitive sets for the intersection contract: exact duplicates, coplanar overlaps, grid-snapped
shared vertices / edges, zero-area triangles and numerically degenerate slivers (they can pass the triangle test with a
meaningless distance far from the sliver: the case the contract's validation rule exists for).  Shared by the CPU test
(checker tree == checker brute force) and the GPU tests (every GPU tree == checker brute force).

PLACEMENTS puts the same soups elsewhere in float32 space -- other scales, far from the origin, anisotropic, flat, collapsed --
and placed_soup adds the rays that meet vertices' coordinates exactly there (tests/test_placements_cpu.py, test_placements_gpu.py)."""
import numpy as np

import _oracle as O
from pbrlab_amd import scenes

F = np.float32


def triangle_soup(seed, extra_slivers=0):
    """-> (desc, rays).  extra_slivers = 0 is the soup of rounds 1-2 (seed 1, ray 6858 is the documented ray on which a
    brute-force loop and a near-first traversal disagreed before the validation rule); extra_slivers > 0 appends that many
    slivers / needles of several kinds and aims a share of the rays at them."""
    rng = np.random.RandomState(500 + seed)
    n = 400
    v = (rng.rand(n, 3, 3).astype(np.float32) * 2 - 1)
    v[:, 1:] = v[:, :1] + (v[:, 1:] - v[:, :1]) * np.float32(0.3)           # smallish triangles
    v[:60] = np.round(v[:60] * 4) / 4                                        # snapped to a grid: shared vertices / edges
    v[60:100, :, 2] = np.float32(0.25)                                      # coplanar, overlapping
    v[100:120] = v[60:80]                                                    # exact duplicates
    v[120:130, 2] = v[120:130, 1]                                            # degenerate
    v[130:140, 2] = v[130:140, 0] + (v[130:140, 1] - v[130:140, 0]) * np.float32(1.000001)   # slivers
    if extra_slivers:
        r2 = np.random.RandomState(7000 + seed)
        e = (r2.rand(extra_slivers, 3, 3).astype(np.float32) * 2 - 1)
        e[:, 1] = e[:, 0] + (e[:, 1] - e[:, 0]) * np.float32(0.6)
        f = np.float32(1.0) + np.float32(2.0) ** (-r2.randint(12, 24, size=extra_slivers)).astype(np.float32) * r2.choice([-1, 1], size=extra_slivers).astype(np.float32)
        f[::5] = np.float32(0.5)                                             # third corner ON the edge, in its middle
        e[:, 2] = e[:, 0] + (e[:, 1] - e[:, 0]) * f[:, None]
        k = np.arange(extra_slivers) % 3 == 1                                # needles: a hair's breadth off the edge
        e[k, 2] += (r2.rand(int(k.sum()), 3).astype(np.float32) - np.float32(0.5)) * np.float32(1e-6)
        v = np.concatenate([v, e])
        n += extra_slivers
    verts = np.concatenate([v.reshape(-1, 3), np.ones((n * 3, 1), np.float32)], 1)
    faces = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")
    desc = scenes.SceneDesc(verts, np.zeros((0, 4), np.float32), [mat],
                            [scenes.Shape("a", faces[:250], None, np.zeros(250, np.uint32)),
                             scenes.Shape("b", faces[250:], None, np.zeros(n - 250, np.uint32))])
    so = O.oracle_scene_from_desc(desc)
    lo, hi = so.FetchSceneAABB()
    rays = scenes.random_rays((lo, hi), 6000, seed=seed)
    extra = np.zeros(2000, O.RAY_DT)                                         # straight at vertices / along grid lines
    tgt = verts[rng.randint(len(verts), size=2000), :3]
    org = np.array([0.3, -0.2, 3.0], np.float32)
    extra["org"] = org
    extra["dir"] = tgt - org
    extra[:500]["org"] = tgt[:500] + np.array([0, 0, 2], np.float32)
    extra[:500]["dir"] = (0, 0, -1)
    extra["tmin"], extra["tmax"] = 0.0, 1e30
    rays = np.concatenate([rays, extra])
    if extra_slivers:
        # rays through points of the slivers' long edges, from random origins (most pass the sliver's plane test region)
        r3 = np.random.RandomState(9000 + seed)
        m = 3000
        which = r3.randint(400, n, size=m)
        w = r3.rand(m, 1).astype(np.float32)
        tgt = v[which, 0] * (1 - w) + v[which, 1] * w
        aim = np.zeros(m, O.RAY_DT)
        o = (r3.rand(m, 3).astype(np.float32) * 2 - 1) * np.float32(1.5)
        aim["org"], aim["dir"] = o, (tgt - o) * np.float32(0.5 + r3.rand())   # hit distances around 1 / that factor
        aim["tmin"], aim["tmax"] = 0.0, 1e30
        rays = np.concatenate([rays, aim])
    return desc, so, rays


# ---------------------------------------------------------------------------------------------------------- placements
# name -> (per-axis scale, offset): a vertex v goes to v * scale + offset, evaluated in float32.  A scale of 0 flattens that axis into
# the offset's plane.  "unit" is the control: the bytes of triangle_soup.
PLACEMENTS = {
    "unit":          ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "scale_2^-20":   ((2.0 ** -20,) * 3, (0.0, 0.0, 0.0)),
    "scale_1e-6":    ((1e-6,) * 3, (0.0, 0.0, 0.0)),
    "scale_1e-10":   ((1e-10,) * 3, (0.0, 0.0, 0.0)),
    "scale_3e7":     ((3e7,) * 3, (0.0, 0.0, 0.0)),
    "scale_1e10":    ((1e10,) * 3, (0.0, 0.0, 0.0)),
    "offset_4096":   ((1.0, 1.0, 1.0), (4096.0, -4096.0, 4096.0)),
    "offset_1e5":    ((1.0, 1.0, 1.0), (1e5, 3e4, -7e4)),
    "scale_1e3_offset_1e7": ((1e3,) * 3, (1e7, 1e7, 1e7)),
    "anisotropic":   ((1e4, 1.0, 1e-3), (0.0, 0.0, 0.0)),
    "anisotropic_2": ((1e-3, 1e4, 1.0), (0.0, 0.0, 0.0)),
    "flat_z":        ((1.0, 1.0, 0.0), (0.0, 0.0, 0.25)),
    "flat_z_1000":   ((100.0, 100.0, 0.0), (0.0, 0.0, 1000.0)),
    "flat_x":        ((0.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "line":          ((1.0, 0.0, 0.0), (0.0, 0.5, -0.25)),
    "point":         ((0.0, 0.0, 0.0), (0.5, -0.25, 0.125)),
}
N_AXIS_RAYS, N_PLANE_RAYS = 3000, 2000


def placement(name):
    """-> (scale, offset, ray scale) as float32 triples; the ray scale is the scale with 1 on a flattened axis.  Beside the names of
    PLACEMENTS, "scale_<float>" is that uniform scale about the origin (the sweeps over 10^k)."""
    s, t = PLACEMENTS[name] if name in PLACEMENTS else ((float(name[len("scale_"):]),) * 3, (0.0, 0.0, 0.0))
    s, t = np.array(s, F), np.array(t, F)
    return s, t, np.where(s == 0, F(1), s).astype(F)


def kept_dimensions(name):
    return int((placement(name)[0] != 0).sum())


def place(p, s, t):
    """p * s + t in float32, two roundings (what every placed vertex and point goes through)"""
    return (np.asarray(p, F) * s + t).astype(F)


def place_rays(rays, s, t):
    """carry rays along: both end points org and org + dir are placed, dir is their difference, all in float32; tmin and tmax stay (dir
    scales with the scene, so the parameter does not)"""
    out = rays.copy()
    end = (rays["org"] + rays["dir"]).astype(F)
    out["org"] = place(rays["org"], s, t)
    out["dir"] = place(end, s, t) - out["org"]
    return out


def edge_rays(verts, rs, seed):
    """Two ray families through a placed vertex set verts (n, 3) float32, rs = the ray scale (the size of the scene per axis):
      * N_AXIS_RAYS axis-parallel rays whose origin shares two coordinates EXACTLY with a vertex, so that the ray runs through it; the two
        components of the direction that are zero are +0 or -0;
      * N_PLANE_RAYS rays with one zero direction component (+0 or -0) that lie in the coordinate plane of a vertex and pass that vertex
        within a tenth of the scene's size.
    tmin = 0, tmax = 3e38."""
    rng = np.random.RandomState(12000 + seed)
    rs = np.asarray(rs, F)
    n = N_AXIS_RAYS
    P = verts[rng.randint(len(verts), size=n)]
    axis = rng.randint(3, size=n)
    sign = rng.choice([-1.0, 1.0], size=n).astype(F)
    zero = np.where(rng.rand(n, 3) < 0.5, F(0.0), F(-0.0)).astype(F)
    d = zero.copy()
    d[np.arange(n), axis] = sign
    o = P.copy()
    o[np.arange(n), axis] = P[np.arange(n), axis] - sign * F(2.5) * rs[axis]
    a = np.zeros(n, O.RAY_DT)
    a["org"], a["dir"] = o, d
    m = N_PLANE_RAYS
    P = verts[rng.randint(len(verts), size=m)]
    axis = rng.randint(3, size=m)
    ang = rng.rand(m) * 2 * np.pi
    w = np.zeros((m, 3), F)                                                  # a direction inside the plane, in units of the scene's size
    w[np.arange(m), (axis + 1) % 3], w[np.arange(m), (axis + 2) % 3] = np.cos(ang), np.sin(ang)
    jit = ((rng.rand(m, 3) * 2 - 1) * 0.1).astype(F)
    jit[np.arange(m), axis] = 0
    o = (P + (jit - F(2.5) * w) * rs).astype(F)
    o[np.arange(m), axis] = P[np.arange(m), axis]
    d = (w * rs).astype(F)
    d[np.arange(m), axis] = np.where(rng.rand(m) < 0.5, F(0.0), F(-0.0))
    b = np.zeros(m, O.RAY_DT)
    b["org"], b["dir"] = o, d
    rays = np.concatenate([a, b])
    rays["tmin"], rays["tmax"] = 0.0, 3e38
    return rays


def placed_desc(desc, name):
    """desc with every vertex placed (the shapes, materials and indices are shared with desc)"""
    import dataclasses
    s, t, _ = placement(name)
    verts = desc.vertices.copy()
    verts[:, :3] = place(desc.vertices[:, :3], s, t)
    return dataclasses.replace(desc, vertices=verts)


def placed_scene(desc, scale, offset):
    """any description without instance transforms under a uniform scale and an offset: mesh vertices and curve control points placed,
    curve radii scaled"""
    import dataclasses
    assert all(sh.transform is None for sh in list(desc.shapes) + list(desc.curves))
    s, t = np.full(3, scale, F), np.array(offset, F)
    verts = desc.vertices.copy()
    verts[:, :3] = place(desc.vertices[:, :3], s, t)
    curves = []
    for c in desc.curves:
        cv = c.vertices.copy()
        cv[:, :3], cv[:, 3] = place(c.vertices[:, :3], s, t), c.vertices[:, 3] * F(scale)
        curves.append(dataclasses.replace(c, vertices=cv))
    return dataclasses.replace(desc, vertices=verts, curves=curves)


def placed_soup(seed, extra_slivers, name):
    """triangle_soup at PLACEMENTS[name] -> (desc, so, rays): the soup's own rays carried along (place_rays), then the two families of
    edge_rays.  ray_families(rays) names the three parts."""
    desc, so, rays = triangle_soup(seed, extra_slivers)
    s, t, rs = placement(name)
    if name != "unit":
        desc = placed_desc(desc, name)
        so = O.oracle_scene_from_desc(desc)
        rays = place_rays(rays, rs, t)
    rays = np.concatenate([rays, edge_rays(np.ascontiguousarray(desc.vertices[:, :3]), rs, seed)])
    return desc, so, rays


def ray_families(rays):
    """-> {family: slice} of placed_soup's rays"""
    n = len(rays) - N_AXIS_RAYS - N_PLANE_RAYS
    return {"soup": slice(0, n), "axis-parallel": slice(n, n + N_AXIS_RAYS), "in-plane": slice(n + N_AXIS_RAYS, len(rays))}


# ---------------------------------------------------------------------------------------------------------- curves
def curve_soup(seed, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """-> (desc, so, rays).  300 cubic ribbons incl. duplicates, degenerate (all control points equal), zero-radius, straight and
    grid-aligned ones, two triangles behind them; random rays and axis-aligned rays aimed at control points.  A uniform scale and an offset
    move the scene (radii scale with it) and carry the rays along; the defaults leave every byte as it is."""
    rng = np.random.RandomState(900 + seed)
    nc = 300
    cp = (rng.rand(nc, 4, 4).astype(np.float32) * 2 - 1)
    cp[:, 1:, :3] = cp[:, :1, :3] + np.cumsum((rng.rand(nc, 3, 3).astype(np.float32) - 0.5) * np.float32(0.3), axis=1)
    cp[..., 3] = np.float32(0.004) + rng.rand(nc, 4).astype(np.float32) * np.float32(0.03)
    cp[:20] = cp[20:40]                                     # duplicates
    cp[40:50, 1:] = cp[40:50, :1]                           # degenerate: a point
    cp[50:60, :, 3] = 0.0                                   # zero radius
    cp[60:70, 1:, :3] = cp[60:70, :1, :3] + np.arange(1, 4, dtype=np.float32)[None, :, None] * np.float32(0.1)   # straight
    cp[70:90, :, :3] = np.round(cp[70:90, :, :3] * 8) / 8   # grid-aligned control points
    tv = np.array([[-1, -1, -0.9, 1], [1, -1, -0.9, 1], [1, 1, -0.9, 1], [-1, 1, -0.9, 1]], np.float32)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")

    def describe(cp, tv):
        curve = scenes.CurveShape("c", cp.reshape(-1, 4), (np.arange(nc, dtype=np.uint32) * 4))
        return scenes.SceneDesc(tv, np.zeros((0, 4), np.float32), [mat],
                                [scenes.Shape("back", np.array([[0, 1, 2], [0, 2, 3]], np.uint32), None, np.zeros(2, np.uint32))], [curve])
    desc = describe(cp, tv)
    so = O.oracle_scene_from_desc(desc)
    lo, hi = so.FetchSceneAABB()
    rays = scenes.random_rays((lo, hi), 5000, seed=seed)
    extra = np.zeros(1500, O.RAY_DT)
    tgt = cp.reshape(-1, 4)[rng.randint(nc * 4, size=1500), :3]
    axis = rng.randint(3, size=1500)
    dirs = np.zeros((1500, 3), np.float32)
    dirs[np.arange(1500), axis] = rng.choice([-1.0, 1.0], size=1500)
    extra["org"], extra["dir"] = tgt - dirs * np.float32(2.5), dirs
    extra["tmin"], extra["tmax"] = 0.0, 1e30
    rays = np.concatenate([rays, extra])
    s, t = np.full(3, scale, F), np.array(offset, F)
    if scale != 1.0 or t.any():
        cp, tv = cp.copy(), tv.copy()
        cp[..., :3], cp[..., 3], tv[:, :3] = place(cp[..., :3], s, t), cp[..., 3] * F(scale), place(tv[:, :3], s, t)
        desc = describe(cp, tv)
        so = O.oracle_scene_from_desc(desc)
        rays = place_rays(rays, s, t)
    return desc, so, rays
