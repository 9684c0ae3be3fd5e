"""The signed-distance model of tests/_sdf_model.py against ground truth, without a GPU.

Six closed shapes -- a regular tetrahedron, a squat pyramid with base dihedrals of 21.8 degrees ("needle"), a cube of 12 triangles, an
L-shaped prism with a 293 degree reflex edge, an 80-triangle icosphere, a 16 x 8 torus -- and about 2000 points each: vertices, edge
midpoints and points on faces displaced along + and - their float64 pseudonormal by 1e-3, 1e-2, 1e-1 and 1 diameter, and uniform points
in twice the box.  The float32 model (nearest primitive, winning feature, float64 pseudonormals rounded to float32, the sign of
dot(p - q, N)) must agree with the float64 generalized winding number at every point farther than 1e-5 diameters from the surface; at
most 1 % of the points may be nearer than that.  The same points show why the table exists: with the nearest triangle's FACE normal in
place of the feature's pseudonormal the sign is wrong at some of them on the needle and on the L-prism.

Also here: the float32 feature choice against tests/_query_model.py::tri_nearest, and the topology report on a closed cube, an open
quad, a cube with one flipped face and three triangles sharing an edge."""
import numpy as np
import pytest

import _query_model as QM
import _sdf_model as SM

F = np.float32


@pytest.mark.parametrize("name", sorted(SM.SHAPES))
def test_shapes_are_closed_consistent_and_outward(name):
    v, f = SM.shape(name)
    r = SM.topology_report(f)
    print(name, r, "volume", SM.signed_volume(v, f))
    assert r["triangles"] == len(f) <= 300
    assert r["edges_boundary"] == r["edges_nonmanifold"] == r["edges_inconsistent"] == 0 and 2 * r["edges_manifold"] == 3 * len(f)
    assert SM.signed_volume(v, f) > 0
    want = {"tetrahedron": 4, "needle": 6, "cube": 12, "l_prism": 20, "icosphere": 80, "torus": 256}[name]
    assert len(f) == want
    if name == "cube":  # corner valences 4 and 5
        assert sorted(set(np.bincount(f.reshape(-1)))) == [4, 5]


def _signs(name, face_only=False):
    v, f = SM.shape(name)
    pts, inside, dist, diam = SM.ground_truth(name)
    slots, shade = SM.mesh_slots(v, f)
    table = SM.pseudonormals64(v[f], f).astype(F)
    if face_only:
        table = np.repeat(table[:, 6:7], 7, axis=1)
    m = SM.signed_model(pts, slots, shade, table)
    assert m["res"]["found"].all()
    return m, inside, dist > SM.NEAR * diam


@pytest.mark.parametrize("name", sorted(SM.SHAPES))
def test_model_sign_equals_the_winding_number(name):
    m, inside, held = _signs(name)
    n = len(inside)
    print(f"{name}: {n} points, {int(inside.sum())} inside, {int((~held).sum())} nearer than {SM.NEAR} diameters, winning features",
          np.bincount(m["feature"], minlength=8))
    assert 1900 <= n <= 2100 and (~held).sum() <= 0.01 * n
    assert inside.sum() > 100 and (~inside).sum() > 100
    got = m["sd"][:, 3] < 0
    bad = np.nonzero(held & (got != inside))[0]
    assert len(bad) == 0, (name, len(bad), bad[:5], m["sd"][bad[:5]], m["feature"][bad[:5]])
    # edges, vertices and faces all win somewhere
    count = np.bincount(m["feature"], minlength=8)
    assert count[0:3].sum() > 0 and count[3:6].sum() > 0 and count[6] > 0 and count[7] == 0


@pytest.mark.parametrize("name", ["needle", "l_prism"])
def test_the_face_normal_alone_gets_the_sign_wrong(name):
    m, inside, held = _signs(name, face_only=True)
    wrong = held & ((m["sd"][:, 3] < 0) != inside)
    print(f"{name}: the nearest triangle's face normal gives the wrong side at {int(wrong.sum())} of {int(held.sum())} points")
    assert wrong.sum() > 0
    assert (m["feature"][wrong] != SM.FEAT_FACE).all()  # ... and only where an edge or a vertex is the closest feature


def test_tri_feature_restates_tri_nearest_and_names_the_feature():
    rng = np.random.RandomState(5)
    tri = (rng.rand(400, 3, 3) * 2 - 1).astype(F)
    tri[:20, 2] = tri[:20, 1]                        # two equal corners
    tri[20:40, 1] = tri[20:40, 0]
    tri[40:60, 1:] = tri[40:60, :1]                  # a point
    tri[60:80, 2] = (tri[60:80, 0] + tri[60:80, 1]) / F(2)  # collinear
    p = (rng.rand(300, 1, 3) * 3 - 1.5).astype(F)
    p[:100, 0] = tri[rng.randint(400, size=100), rng.randint(3, size=100)]  # on corners
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    d2, u, v, q, feat = SM.tri_feature(p, a, b, c)
    w = QM.tri_nearest(p, a, b, c)
    for got, want in zip((d2, u, v, q), w):
        assert np.array_equal(got.view(np.uint32), np.asarray(want, F).view(np.uint32))
    assert set(np.unique(feat)) == set(range(7))
    # what the names mean: (u, v) of an edge winner lies strictly inside the edge, of a vertex winner on the corner
    for name, uv in ((SM.FEAT_A, (0, 0)), (SM.FEAT_B, (1, 0)), (SM.FEAT_C, (0, 1))):
        k = feat == name
        assert np.array_equal(u[k], np.full(k.sum(), uv[0], F)) and np.array_equal(v[k], np.full(k.sum(), uv[1], F))
    k = feat == SM.FEAT_AB
    assert (u[k] > 0).all() and (u[k] < 1).all() and (v[k] == 0).all()
    k = feat == SM.FEAT_BC
    assert (v[k] > 0).all() and (v[k] < 1).all()
    k = feat == SM.FEAT_CA
    assert (u[k] == 0).all() and (v[k] > 0).all() and (v[k] < 1).all()
    # a triangle without area never wins by its plane
    assert (feat[:, :80] != SM.FEAT_FACE).all()
    # constructed: above the middle of a right triangle, beside its hypotenuse, beyond a corner
    a, b, c = (np.array(x, F) for x in ([0, 0, 0], [1, 0, 0], [0, 1, 0]))
    for point, want in (([0.25, 0.25, 1], SM.FEAT_FACE), ([1, 1, 0], SM.FEAT_BC), ([-1, -1, 0.5], SM.FEAT_A), ([2, -0.5, 0], SM.FEAT_B), ([0.5, -1, 0], SM.FEAT_AB),
                        ([-1, 0.5, 0], SM.FEAT_CA), ([-0.5, 3, 0], SM.FEAT_C)):
        assert SM.tri_feature(np.array(point, F), a, b, c)[4] == want, point


def test_topology_report():
    v, f = SM.shape("cube")
    assert SM.topology_report(f) == dict(triangles=12, vertices=8, edges_manifold=18, edges_boundary=0, edges_nonmanifold=0, edges_inconsistent=0)
    quad = np.array([[0, 1, 2], [0, 2, 3]])
    assert SM.topology_report(quad) == dict(triangles=2, vertices=4, edges_manifold=1, edges_boundary=4, edges_nonmanifold=0, edges_inconsistent=0)
    flipped = f.copy()
    flipped[5] = flipped[5][[0, 2, 1]]
    assert SM.topology_report(flipped) == dict(triangles=12, vertices=8, edges_manifold=15, edges_boundary=0, edges_nonmanifold=0, edges_inconsistent=3)
    fan = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]])
    assert SM.topology_report(fan) == dict(triangles=3, vertices=5, edges_manifold=0, edges_boundary=6, edges_nonmanifold=1, edges_inconsistent=0)
    # the same indices in another object are other vertices
    two = SM.topology_report(np.concatenate([quad, quad]), np.array([0, 0, 1, 1]))
    assert two == dict(triangles=4, vertices=8, edges_manifold=2, edges_boundary=8, edges_nonmanifold=0, edges_inconsistent=0)


def test_pseudonormals_of_the_cube():
    """every pseudonormal of an axis-aligned box is what symmetry says: a face's its axis, an edge's the bisector of its two faces (the
    diagonal of a face: the face's), a corner's (1, 1, 1) / sqrt(3) by sign -- only with the ANGLE weights, since a corner has four or
    five triangles"""
    v, f = SM.shape("cube")
    pn = SM.pseudonormals64(v[f], f)
    un = SM.face_normals64(v[f])
    assert np.allclose(np.abs(un).max(axis=1), 1.0)
    corner = np.sign(v[f])  # (T, 3, 3)
    assert np.allclose(pn[:, 3:6], corner / np.sqrt(3.0), atol=1e-12)
    for t in range(len(f)):
        for k in range(3):
            a, b = v[f[t, k]], v[f[t, (k + 1) % 3]]
            shared = np.sign(a) == np.sign(b)
            want = np.where(shared, np.sign(a), 0.0)
            if shared.sum() == 1:  # a face's diagonal
                want = un[t]
            assert np.allclose(pn[t, k], want / np.linalg.norm(want), atol=1e-12), (t, k)
