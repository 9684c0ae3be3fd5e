"""The signed-distance contract of DESIGN.md §20 restated for the tests.

* adjacency and the topology report of an indexed triangle set, and its angle-weighted pseudonormals in float64 (`pseudonormals64`);
* the float32 feature choice and sign on top of tests/_query_model.py, operation for operation as pbrlab_amd/csrc/dnearest.h and
  sdf.hip evaluate them (`tri_feature`, `signed_model`), given a pseudonormal table;
* ground truth for closed meshes: the float64 generalized winding number by brute force over Van Oosterom-Strackee solid angles
  (`winding_number`; a point is inside iff it rounds to 1) and the float64 distance to the surface (`dist64`);
* the shapes and the points of the tests.

A vertex is (object, position index); equal positions under different indices are not welded.  Table rows per triangle: ab, bc, ca, a, b,
c, face."""
import functools

import numpy as np

import _query_model as QM

F = np.float32
NONE = 0xFFFFFFFF
FEAT_AB, FEAT_BC, FEAT_CA, FEAT_A, FEAT_B, FEAT_C, FEAT_FACE, FEAT_CURVE = range(8)
SCALES = (1e-3, 1e-2, 1e-1, 1.0)  # displacements along the pseudonormal, in diameters
NEAR = 1e-5                       # points closer to the surface than this many diameters are not held to the ground truth


# ------------------------------------------------------------------------------------------------ shapes (closed, outward oriented)
def _outward_convex(v, f):
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64).copy()
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    flip = (n * (v[f].mean(axis=1) - v.mean(axis=0))).sum(axis=1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f


def tetrahedron():
    return _outward_convex([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def needle():
    """a square pyramid whose sides meet the base at atan(0.4) = 21.8 degrees: four edges far sharper than a right angle"""
    v = [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0.1, -0.05, 0.4]]
    return _outward_convex(v, [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])


def cube():
    """12 triangles: the diagonals give the corners 4 or 5 faces each, so the angle weights matter"""
    v = [[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]]
    f = [[0, 1, 2], [0, 2, 3], [5, 6, 7], [5, 7, 4], [1, 5, 4], [1, 4, 0], [3, 2, 6], [3, 6, 7], [2, 6, 5], [2, 5, 1], [0, 3, 7], [0, 7, 4]]
    return _outward_convex(np.array(v, np.float64) * [0.5, 0.7, 0.6], f)


def l_prism():
    """an L whose inner corner is pulled in to (0.5, 0.5): the reflex edge opens 293 degrees inside, its two neighbours are sharper than a
    right angle.  20 triangles; the caps are fans around the inner corner (valence 7)."""
    poly = np.array([[0, 0], [3, 0], [3, 1], [0.5, 0.5], [1, 3], [0, 3]], np.float64)
    n = len(poly)
    v = np.concatenate([np.c_[poly, np.zeros(n)], np.c_[poly, np.ones(n)]])
    fan = [[3, 4, 5], [3, 5, 0], [3, 0, 1], [3, 1, 2]]  # counter-clockwise seen from +z
    f = [[a + n, b + n, c + n] for a, b, c in fan] + [[a, c, b] for a, b, c in fan]
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, j + n], [i, j + n, i + n]]
    return v, np.array(f, np.int64)


def icosphere():
    from pbrlab_amd import scenes
    v, f = scenes._icosphere(1)  # 80 triangles
    return _outward_convex(v * 0.8, f)


def torus(nu=16, nv=8, R=1.0, r=0.35):
    th, ph = np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv
    v = np.array([[(R + r * np.cos(p)) * np.cos(t), (R + r * np.cos(p)) * np.sin(t), r * np.sin(p)] for t in th for p in ph])
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [[a, b, c], [a, c, d]]
    f = np.array(f, np.int64)
    if signed_volume(v, f) < 0:
        f = f[:, [0, 2, 1]]
    return v, f


SHAPES = {"tetrahedron": tetrahedron, "needle": needle, "cube": cube, "l_prism": l_prism, "icosphere": icosphere, "torus": torus}


@functools.lru_cache(maxsize=None)
def shape(name):
    """-> (vertices (V, 3) float32 as float64, faces (T, 3) int64): what a float32 scene holds, so that model and scene agree"""
    v, f = SHAPES[name]()
    return np.asarray(v, F).astype(np.float64), np.asarray(f, np.int64)


def signed_volume(v, f):
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def diameter(v):
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


# ------------------------------------------------------------------------------------------------ adjacency, report, pseudonormals
def features(idx, obj=None):
    """idx (T, 3) position indices, obj (T,) object ids -> (edge_of (T, 3) ids of the edges ab, bc, ca, vert_of (T, 3) ids of the corners,
    edge_faces {edge id: [(face, forward)]} in ascending face order)"""
    idx = np.asarray(idx, np.int64)
    obj = np.zeros(len(idx), np.int64) if obj is None else np.asarray(obj, np.int64)
    edges, verts, edge_faces = {}, {}, {}
    edge_of, vert_of = np.zeros((len(idx), 3), np.int64), np.zeros((len(idx), 3), np.int64)
    for t in range(len(idx)):
        for k in range(3):
            a, b = int(idx[t, k]), int(idx[t, (k + 1) % 3])
            e = edges.setdefault((int(obj[t]), min(a, b), max(a, b)), len(edges))
            edge_of[t, k] = e
            edge_faces.setdefault(e, []).append((t, a < b))
            vert_of[t, k] = verts.setdefault((int(obj[t]), a), len(verts))
    return edge_of, vert_of, edge_faces


def topology_report(idx, obj=None):
    edge_of, vert_of, edge_faces = features(idx, obj)
    r = dict(triangles=len(np.asarray(idx)), vertices=len(np.unique(vert_of)) if len(vert_of) else 0, edges_manifold=0, edges_boundary=0,
             edges_nonmanifold=0, edges_inconsistent=0)
    for fs in edge_faces.values():
        if len(fs) == 1:
            r["edges_boundary"] += 1
        elif len(fs) >= 3:
            r["edges_nonmanifold"] += 1
        elif fs[0][1] != fs[1][1]:
            r["edges_manifold"] += 1
        else:
            r["edges_inconsistent"] += 1
    return r


def _unit_rows(n):
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(ln > 0, n / ln, 0.0)


def face_normals64(corners):
    corners = np.asarray(corners, np.float64)
    return _unit_rows(np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]))


def corner_angles64(corners):
    """(T, 3): the angle at a, b, c: atan2(|e1 x e2|, e1 . e2)"""
    c = np.asarray(corners, np.float64)
    out = np.zeros((len(c), 3))
    for k in range(3):
        e1, e2 = c[:, (k + 1) % 3] - c[:, k], c[:, (k + 2) % 3] - c[:, k]
        out[:, k] = np.arctan2(np.linalg.norm(np.cross(e1, e2), axis=1), (e1 * e2).sum(axis=1))
    return out


def pseudonormals64(corners, idx, obj=None):
    """corners (T, 3, 3) positions, idx (T, 3), obj (T,) -> (T, 7, 3) float64: rows ab, bc, ca, a, b, c, face"""
    corners = np.asarray(corners, np.float64)
    edge_of, vert_of, _ = features(idx, obj)
    un, ang = face_normals64(corners), corner_angles64(corners)
    ne, nv = (int(x.max()) + 1 if x.size else 0 for x in (edge_of, vert_of))
    es, vs = np.zeros((ne, 3)), np.zeros((nv, 3))
    for k in range(3):
        np.add.at(es, edge_of[:, k], un)
        np.add.at(vs, vert_of[:, k], ang[:, k, None] * un)
    es, vs = _unit_rows(es), _unit_rows(vs)
    out = np.zeros((len(corners), 7, 3))
    out[:, 0:3], out[:, 3:6], out[:, 6] = es[edge_of], vs[vert_of], un
    return out


def pseudonormal_bounds(corners, idx, obj=None):
    """The rounding bound of DESIGN.md §20 for every row of the float32 table against `pseudonormals64`, as the Euclidean norm of the
    difference in units of u = 2^-24 -> (T, 7).  Conditioning comes from the float64 model alone.  With theta the angle at corner a
    (the face normal is cross(b - a, c - a)), alpha the corner angles, S the unnormalised sum of a feature and k its number of faces:
        face    A = 14 / sin(theta) + 4
        edge    2 (sum_i A_i + k^2) / |S| + 4
        vertex  2 (sum_i (43 + alpha_i (A_i + 1)) + k sum_i alpha_i) / |S| + 4
    A face without a normal contributes nothing and has the bound 0; so has a feature whose sum has no length (nan: not compared)."""
    corners = np.asarray(corners, np.float64)
    edge_of, vert_of, _ = features(idx, obj)
    e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    n = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        sin_t = np.linalg.norm(n, axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
        A = np.where(sin_t > 0, 14.0 / sin_t + 4.0, 0.0)
    has = (sin_t > 0).astype(np.float64)
    un, ang = face_normals64(corners), corner_angles64(corners)
    ne, nv = (int(x.max()) + 1 if x.size else 0 for x in (edge_of, vert_of))
    es, ea, ek = np.zeros((ne, 3)), np.zeros(ne), np.zeros(ne)
    vs, va, vk, vw = np.zeros((nv, 3)), np.zeros(nv), np.zeros(nv), np.zeros(nv)
    for k in range(3):
        np.add.at(es, edge_of[:, k], un), np.add.at(ea, edge_of[:, k], A * has), np.add.at(ek, edge_of[:, k], has)
        np.add.at(vs, vert_of[:, k], ang[:, k, None] * un), np.add.at(va, vert_of[:, k], has * (43.0 + ang[:, k] * (A + 1.0)))
        np.add.at(vk, vert_of[:, k], has), np.add.at(vw, vert_of[:, k], has * ang[:, k])
    with np.errstate(all="ignore"):
        be = 2.0 * (ea + ek * ek) / np.linalg.norm(es, axis=1) + 4.0
        bv = 2.0 * (va + vk * vw) / np.linalg.norm(vs, axis=1) + 4.0
    out = np.zeros((len(corners), 7))
    out[:, 0:3], out[:, 3:6], out[:, 6] = be[edge_of], bv[vert_of], A
    return out


# ------------------------------------------------------------------------------------------------ the float32 restatement
def _seg_feature(t, edge, v0, v1):
    return np.where(t > 0, np.where(t < 1, edge, v1), v0)


def tri_feature(p, a, b, c):
    """tests/_query_model.py::tri_nearest with the winning feature: -> (D2, u, v, q, feature).  The segments ab, bc, ca in that order, a
    strict < replaces; a clamped t of 0 or 1 names the vertex at that end; the plane term last."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    one = F(1)
    d2, t, q = QM.seg_dist2(p, a, b)
    u, v, feat = t, np.zeros_like(t), _seg_feature(t, FEAT_AB, FEAT_A, FEAT_B)
    for (x, y), uv, names in (((b, c), lambda t: (one - t, t), (FEAT_BC, FEAT_B, FEAT_C)), ((c, a), lambda t: (np.zeros_like(t), one - t), (FEAT_CA, FEAT_C, FEAT_A))):
        e2, t, qe = QM.seg_dist2(p, x, y)
        rep = e2 < d2
        ue, ve = uv(t)
        d2, u, v, q = np.where(rep, e2, d2), np.where(rep, ue, u), np.where(rep, ve, v), np.where(rep[..., None], qe, q)
        feat = np.where(rep, _seg_feature(t, *names), feat)
    n = QM.cross(b - a, c - a)
    nn = QM.dot(n, n)
    s_ab, s_bc, s_ca = QM.dot(QM.cross(b - a, p - a), n), QM.dot(QM.cross(c - b, p - b), n), QM.dot(QM.cross(a - c, p - c), n)
    inside = (nn > 0) & (s_ab >= 0) & (s_bc >= 0) & (s_ca >= 0)
    h = QM.dot(p - a, n)
    with np.errstate(all="ignore"):
        w = h / nn
        dp = w * h
        qp = p - w[..., None] * n
        up, vp = s_ca / nn, s_ab / nn
    rep = inside & (dp < d2)
    d2, u, v, q = np.where(rep, dp, d2), np.where(rep, up, u), np.where(rep, vp, v), np.where(rep[..., None], qp, q)
    feat = np.where(rep, FEAT_FACE, feat)
    L = QM.own_box_dist2(np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c), p)
    return np.where(d2 < L, L, d2).astype(F), u.astype(F), v.astype(F), q.astype(F), feat.astype(np.int64)


def signed_model(points, slots, shade, table):
    """The contract's answer per query: tests/_query_model.py's brute force for the winner, then the winner's feature, that feature's row
    of `table` ((slots, 7, >= 3) float32: the device's own, or a model's) and the sign.
    -> dict(ident, closest, sd (n, 4) float32, feature (n,), res = the brute force's dict)"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    slots, shade, table = np.asarray(slots, F), np.asarray(shade, np.uint32), np.asarray(table, F)
    res = QM.brute_force(pts, slots, shade)
    ident, closest = QM.expected_buffers(res)
    n = len(pts)
    sd, feature = np.zeros((n, 4), F), np.full(n, FEAT_CURVE, np.int64)
    k = np.nonzero(res["found"])[0]
    if len(k):
        sl = res["slot"][k].astype(np.int64)
        curve = ((shade[sl, 3] >> 24) & QM.SLOT_IS_CURVE) != 0
        p = pts[k, :3]
        d2, u, v, q, feat = tri_feature(p, slots[sl, 0, :3], slots[sl, 1, :3], slots[sl, 2, :3])
        tri = ~curve
        assert np.array_equal(d2[tri], res["d2"][k][tri]) and np.array_equal(q[tri], res["q"][k][tri])  # (the two restatements agree)
        feat = np.where(curve, FEAT_CURVE, feat)
        N = np.where(curve[:, None], F(0), table[sl, np.minimum(feat, 6), :3]).astype(F)
        s = QM.dot(p - res["q"][k], N)
        d = np.sqrt(res["d2"][k])
        sd[k, :3], sd[k, 3] = N, np.where(s < 0, -d, d)
        feature[k] = feat
    return dict(ident=ident, closest=closest, sd=sd, feature=feature, res=res)


def mesh_slots(v, f, obj=None):
    """a mesh as the slots and ShadeRecs of a committed scene would hold it (gid = face index) -> (slots (T, 4, 4), shade (T, 32))"""
    v, f = np.asarray(v, F), np.asarray(f, np.int64)
    slots, shade = np.zeros((len(f), 4, 4), F), np.zeros((len(f), 32), np.uint32)
    slots[:, :3, :3] = v[f]
    shade[:, 24] = np.arange(len(f))
    shade[:, 25] = 0 if obj is None else obj
    shade[:, 27] = np.arange(len(f))
    return slots, shade


# ------------------------------------------------------------------------------------------------ ground truth in float64
def winding_number(p, tri, chunk=512):
    """the generalized winding number of the triangles tri (T, 3, 3) about each point p (n, 3): the sum of the signed solid angles
    2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|) over 4 pi (Van Oosterom & Strackee 1983)"""
    p, tri = np.asarray(p, np.float64), np.asarray(tri, np.float64)
    out = np.zeros(len(p))
    for at in range(0, len(p), chunk):
        r = tri[None] - p[at:at + chunk, None, None, :]
        a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(axis=-1)
        den = la * lb * lc + (a * b).sum(axis=-1) * lc + (b * c).sum(axis=-1) * la + (c * a).sum(axis=-1) * lb
        out[at:at + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def dist64(p, tri, chunk=512):
    p, tri = np.asarray(p, np.float64), np.asarray(tri, np.float64)
    out = np.zeros(len(p))
    for at in range(0, len(p), chunk):
        out[at:at + chunk] = QM.tri_dist64(p[at:at + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).min(axis=1)
    return out


# ------------------------------------------------------------------------------------------------ points
def sample_points(v, f, seed, per_kind=42, n_box=1000):
    """About 2000 points for a mesh: `per_kind` vertices, edge midpoints and points on faces (all of a kind when the mesh has fewer,
    topped up with points on faces), each displaced along + and - its float64 pseudonormal by SCALES x the diameter; then n_box points
    uniform in twice the box.  -> (n, 4) float32 rows (p, inf)"""
    rng = np.random.RandomState(7100 + seed)
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    pn = pseudonormals64(v[f], f)
    edge_of, vert_of, _ = features(f)
    base, normal = [], []
    _, first = np.unique(vert_of.reshape(-1), return_index=True)
    for at in rng.permutation(first)[:per_kind]:
        t, k = divmod(int(at), 3)
        base.append(v[f[t, k]]), normal.append(pn[t, 3 + k])
    _, first = np.unique(edge_of.reshape(-1), return_index=True)
    for at in rng.permutation(first)[:per_kind]:
        t, k = divmod(int(at), 3)
        base.append(0.5 * (v[f[t, k]] + v[f[t, (k + 1) % 3]])), normal.append(pn[t, k])
    while len(base) < 3 * per_kind:
        t = rng.randint(len(f))
        w = rng.dirichlet((1.0, 1.0, 1.0))
        base.append(w @ v[f[t]]), normal.append(pn[t, 6])
    base, normal = np.array(base), np.array(normal)
    d = diameter(v)
    moved = [base + sign * s * d * normal for s in SCALES for sign in (1.0, -1.0)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, h = 0.5 * (lo + hi), hi - lo
    box = c + (rng.rand(n_box, 3) * 2 - 1) * h
    p = np.concatenate(moved + [box]).astype(F)
    return np.ascontiguousarray(np.concatenate([p, np.full((len(p), 1), np.inf, F)], axis=1), F)


@functools.lru_cache(maxsize=None)
def ground_truth(name):
    """-> (points (n, 4) float32, inside (n,) bool, distance (n,) float64, diameter) for a shape, computed once"""
    v, f = shape(name)
    pts = sample_points(v, f, sorted(SHAPES).index(name))
    p = pts[:, :3].astype(np.float64)
    w = winding_number(p, v[f])
    return pts, np.rint(w) == 1, dist64(p, v[f]), diameter(v)
