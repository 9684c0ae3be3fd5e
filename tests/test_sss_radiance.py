"""The random-walk subsurface closure's radiance against float64 slab transport (tests/_sss_analytic.py), on both back
ends: the oracle leg runs on the CPU, the HIP leg is marked gpu.

Scene.  A box slab [-5, 5] x [-5, 5] x [-0.1, 0], alone, under the constant environment L = (1.0, 0.8, 0.6); a look-at camera straight
above sees only the central 0.4 x 0.3 of the top face, at 64 x 48.  The half-width is 50 thicknesses, so the transport is
one-dimensional (test_side_walls_do_not_matter).  Every material has specular = metallic = clearcoat = 0: subsurface is the only
closure and no selection weight enters.

Expectation, from the reference's text.  NEE at the entry evaluates a closure set without a subsurface term and adds 0.  The distance
sampling is a one-sample balance-heuristic estimator over the three channels and the roulette divides by its own probability, so the
walk's throughput is unbiased per channel: a walk leaves through the top face with expected weight thr0 R and through the bottom face
with thr0 T, (R, T) = slab(a, tau0) per channel.  The exit continues as a Lambert surface of weight thr: NEE in the exit frame, then a
cosine-distributed direction -- which CyclesPrincipledShader takes to world space with the ENTRY frame (cycles-principled-shader.cc:
468-470).  At the top face the two frames are equal and the exit returns thr L (the furnace property of
tests/_env_analytic.py).  At the bottom face they are opposite: the BSDF ray goes back into the slab, meets the top face from behind
and ends (a walk refuses a back face), so only the NEE part arrives, KAPPA = ln(17) / 16 = 0.1771 of thr L.  Hence
    E_c = L_c thr0_c (R + KAPPA T)(a_c, tau0_c)
and every case must REJECT the quirk-free L thr0 (R + T).  With a black plate of another instance inside the slab at depth 0.04 every
walk that meets it ends (random-walk-sss.h:371-378): E_c = L_c thr0_c R(a_c, 0.4 tau0_c), reflection alone, and R + T of the cut slab
must be rejected.  The plate cases run under PBRHIP_SSS_FOREIGN = 0 and the default (the walk's entry below the root, with and
without foreign references).

Statistics: test_analytic_radiance.py's protocol unchanged -- K = 64 batches, a fixed seed_seq, first_pass = spp * k; 8 x 8 cells plus
the whole receiver; Student-t bar at two-sided 1e-6 / n_tests.  spp per case is the smallest of 16, 32, 64 at which the oracle rejects
1.01 E for the whole-receiver mean (the power check, inside the test); the table CASES holds it with the z observed there."""
import numpy as np
import pytest

import _analytic as A
import _oracle as O
import _sss_analytic as S
from test_analytic_radiance import BACKENDS, CELL, K, _pa, group_stats

W, H = 64, 48
SEED_SEQ = 1618033988
THICKNESS = 0.1
HALF = 5.0
PLATE_DEPTH = 0.04
L_ENV = np.array([1.0, 0.8, 0.6])
EYE, FOV = (0.0, 0.0, 1.0), float(np.degrees(2.0 * np.arctan(0.15)))     # 0.4 x 0.3 of the plane z = 0


def _mat(colour, tau0, subsurface=1.0, **kw):
    """a one-closure subsurface material whose mixed colour is `colour` and whose optical thickness across the slab is tau0"""
    colour = np.broadcast_to(np.asarray(colour, np.float64), (3,))
    tau0 = np.broadcast_to(np.asarray(tau0, np.float64), (3,))
    base = kw.pop("base_color", tuple(colour))
    sc = (colour - np.asarray(base) * (1.0 - subsurface)) / subsurface
    r = S.radius_for_tau0(colour, tau0, THICKNESS, subsurface)
    return A.material(subsurface=subsurface, base_color=tuple(base), subsurface_color=tuple(sc), subsurface_radius=tuple(r), specular=0.0,
                      metallic=0.0, clearcoat=0.0, **kw)


# case -> (material, spp, z of 1.01 E for the whole-receiver mean on the oracle at that spp: the largest |z| of the three channels)
CASES = {
    "gray": (_mat(0.5, 2.0), 16, -23.1),
    "chromatic": (_mat((0.8, 0.5, 0.2), (0.7, 2.5, 8.0)), 16, -18.2),
    "thin_bright": (_mat(0.9, 0.5), 16, -19.1),
    "thick": (_mat((0.95, 0.6, 0.3), 10.0), 16, -43.3),
    "half": (_mat((0.65, 0.55, 0.55), 2.0, subsurface=0.5, base_color=(0.9, 0.3, 0.5)), 16, -23.6),
    "weighted": (_mat(0.5, 2.0, transmission=0.25), 16, -14.0),
}
PLATE_CASES = {"gray": (16, -14.7), "chromatic": (16, -12.9)}   # (spp, z of 1.01 E as above; the same under either PBRHIP_SSS_FOREIGN)


def slab_scene(mat, plate=False):
    parts = [A.quad((0, 0, 0), (HALF, 0, 0), (0, HALF, 0)),                                           # top, +z
             A.quad((0, 0, -THICKNESS), (0, HALF, 0), (HALF, 0, 0)),                                  # bottom, -z
             A.quad((HALF, 0, -0.5 * THICKNESS), (0, HALF, 0), (0, 0, 0.5 * THICKNESS)),              # +x
             A.quad((-HALF, 0, -0.5 * THICKNESS), (0, 0, 0.5 * THICKNESS), (0, HALF, 0)),             # -x
             A.quad((0, HALF, -0.5 * THICKNESS), (0, 0, 0.5 * THICKNESS), (HALF, 0, 0)),              # +y
             A.quad((0, -HALF, -0.5 * THICKNESS), (HALF, 0, 0), (0, 0, 0.5 * THICKNESS))]             # -y
    v = np.concatenate([p[0] for p in parts])
    f = np.concatenate([p[1] + 4 * k for k, p in enumerate(parts)])
    c = v[f].mean(1)
    n = np.cross(v[f][:, 1] - v[f][:, 0], v[f][:, 2] - v[f][:, 0])
    assert (np.sum(n * (c - np.array([0, 0, -0.5 * THICKNESS])), 1) > 0).all(), "every face of the slab looks outwards"
    meshes = [A.Mesh("slab", v, f, mat)]
    if plate:
        pv, pf = A.quad((0, 0, -PLATE_DEPTH), (4.95, 0, 0), (0, 4.95, 0))
        meshes.append(A.Mesh("plate", pv, pf, A.material(**A.BLACK)))
    return A.Scene(meshes)


def render_batches(backend, S_, spp, w=W, h=H):
    env = np.tile(L_ENV.astype(np.float32), (4, 8, 1))
    if backend == "oracle":
        so = A.build(O.OracleScene(), S_, O.make_principled)
        so.SetEnvironment(env, 1.0, None)
        so.SetCamera(EYE, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV)
        th = O.oracle_threads()
        out = [so.render(w, h, spp, first_pass=k * spp, seed_seq=SEED_SEQ, threads=th)[:2] for k in range(K)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    pa = _pa()
    sg = A.build(pa.Scene(), S_, pa.make_principled)
    sg.SetEnvironment(env, 1.0, None)
    sg.SetCamera(EYE, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV)
    rgba, count = [], []
    for k in range(K):
        layer = pa.RenderLayer()
        pa.Render(sg, w, h, spp, layer=layer, first_pass=k * spp, seed_seq=SEED_SEQ)
        rgba.append(np.array(layer.rgba, np.float32).reshape(h, w, 4))
        count.append(np.array(layer.count, np.uint32).reshape(h, w))
    sg.close()
    return np.stack(rgba), np.stack(count)


def stats(means, E):
    """z per (8 x 8 cell, channel) and for the whole image (the last row), and the bar: test_analytic_radiance.group_stats"""
    h, w = means.shape[1:3]
    groups = []
    for cy in range(0, h, CELL):
        for cx in range(0, w, CELL):
            g = np.zeros((h, w), bool)
            g[cy:cy + CELL, cx:cx + CELL] = True
            groups.append(g)
    groups.append(np.ones((h, w), bool))
    return group_stats(means, groups, np.broadcast_to(np.asarray(E, np.float64), (h, w, 3)))


_expect = {}


def expected(case, plate):
    if (case, plate) not in _expect:
        mat = CASES[case][0]
        kw = dict(plate_depth=PLATE_DEPTH) if plate else {}
        e = dict(E=S.slab_radiance(mat, THICKNESS, L_ENV, **kw))
        if plate:
            e["open_plate"] = S.slab_radiance(mat, THICKNESS, L_ENV, plate_open=True, **kw)
        else:
            e["no_quirk"] = S.slab_radiance(mat, THICKNESS, L_ENV, quirk=False)
            if case == "chromatic":
                e["gray_mean"] = S.slab_radiance(mat, THICKNESS, L_ENV, gray_mean=True)
        _expect[(case, plate)] = e
    return _expect[(case, plate)]


def check(name, backend, S_, e, spp, frame=(W, H)):
    rgba, count = render_batches(backend, S_, spp, *frame)
    assert (count == spp).all() and (rgba[..., 3] == count).all()
    means = rgba[..., :3] / count[..., None]
    E = e["E"]
    z, bar = stats(means, E)
    rel = means.mean((0, 1, 2)) / E - 1
    print(f"sss {name} [{backend}] spp {spp}: E {E}, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), whole-receiver z "
          f"{' '.join(f'{v:+.2f}' for v in z[-1])}, rel err {' '.join(f'{r:+.1e}' for r in rel)}")
    assert np.abs(z).max() < bar, (name, z[-1], bar)
    z1, _ = stats(means, 1.01 * E)
    print(f"sss {name} [{backend}]: whole-receiver z against 1.01 E {' '.join(f'{v:+.2f}' for v in z1[-1])}")
    assert np.abs(z1[-1]).max() >= bar, (name, "1.01 E is not rejected for the whole-receiver mean", z1[-1], bar)
    for alt in e:
        if alt != "E":
            za, _ = stats(means, e[alt])
            print(f"sss {name} [{backend}]: max |z| against {alt} ({e[alt]}): {np.abs(za).max():.1f}")
            assert np.abs(za).max() >= bar, (name, f"{alt} is not rejected", np.abs(za).max(), bar)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(CASES))
def test_slab_radiance(case, backend):
    mat, spp, _ = CASES[case]
    check(case, backend, slab_scene(mat), expected(case, False), spp)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("foreign", ["0", None])
@pytest.mark.parametrize("case", list(PLATE_CASES))
def test_slab_with_plate_radiance(case, foreign, backend, monkeypatch):
    if foreign is None:
        monkeypatch.delenv("PBRHIP_SSS_FOREIGN", raising=False)
    else:
        monkeypatch.setenv("PBRHIP_SSS_FOREIGN", foreign)
    check(f"{case}+plate(foreign={foreign})", backend, slab_scene(CASES[case][0], plate=True), expected(case, True), PLATE_CASES[case][0])


def test_side_walls_do_not_matter():
    """the numpy Monte Carlo with walls 50 thicknesses away: of 1e6 walks none reaches a wall (the lateral leakage decays like
    exp(-pi r / thickness) for a thick slab; in the thin one a single flight spans d thicknesses with probability exp(-tau0 d), 4e-11 for
    the 48 from the camera's field to a wall), so R + T with walls is R + T without; the widest walk stays within half the way"""
    for a, tau0 in ((0.95, 10.0), (0.9, 0.5)):
        free, walled = S.slab_mc(a, tau0, 1000000, seed=3), S.slab_mc(a, tau0, 1000000, seed=3, half_width=HALF / THICKNESS - 2.0)
        assert walled["wall"] == 0.0 and walled["reach"] < 0.5 * HALF / THICKNESS, walled
        assert abs((walled["R"] + walled["T"]) - (free["R"] + free["T"])) < 1e-6


def test_cases_are_what_the_table_says():
    """the materials give the optical thicknesses of the issue's table, one closure, and the thr0 they claim"""
    want = {"gray": 2.0, "chromatic": (0.7, 2.5, 8.0), "thin_bright": 0.5, "thick": 10.0, "half": 2.0, "weighted": 2.0}
    for case, (mat, _, _) in CASES.items():
        m = S.medium(mat)
        assert m["enable_subsurface"] and not m["enable_diffuse"]
        assert np.allclose(m["sigma_t"] * THICKNESS, want[case], rtol=1e-5), (case, m["sigma_t"] * THICKNESS)
        assert np.allclose(m["thr0"], 0.75 if case == "weighted" else 1.0, rtol=1e-6)
    assert CASES["half"][0]["base_color"] != CASES["half"][0]["subsurface_color"]
    assert abs(S.KAPPA - np.log(17.0) / 16.0) < 1e-15
    mu = (np.arange(200000) + 0.5) / 200000
    assert abs(np.mean(2.0 * mu / (1.0 + 16.0 * mu * mu)) - S.KAPPA) < 1e-9
