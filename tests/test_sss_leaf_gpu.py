"""GPU (-m gpu): the device's random-walk leaves (pbrhip_leaf_eval ops 11-13) against the float64 model of the reference's text
(tests/_sss_analytic.py), on the inputs and with the bounds of tests/test_sss_model_cpu.py.

Op 11 (ParamToBsdf + the medium as commit hoists it) and op 12 (SampleScatterDistance, its channel pdf computed with and without a
precomputed albedo: bit-equal) use that module's MEDIUM_BOUND and DISTANCE_BOUND.  Op 13 runs sss_scatter, the function k_sss_step
and k_sss_walk call, on 4096 seeded walk states against walk_event.  Its bounds, in float32 roundings (eps = 2^-24) along the longest
path, states chosen with sigma_t t <= 8 in every channel:
    channel pdf                                   5
    T = exp(-sigma_t t)                           8 + 2    (the product's rounding moves the exponent by <= 8 eps; exp's 1 ulp)
    pdf = dot(channel pdf, sigma_t T)             5 + 1 + 10 + 1, two sums of positives: 19
    thr sigma_s T / pdf                           2 + 10 + 19 + 1 = 32
    p = saturate(max thr), thr / p                32 + 1                                        -> SCATTER_BOUND = 65 eps = 3.9e-6
    t' = -log(1 - e1) / sigma_t[channel]          3 eps (DISTANCE's t), where the channel agrees: the next channel pdf's components differ
                                                  from the model's by <= 2 x 17 eps (thr sigma_s T and the pdf's own 5; the common factors
                                                  cancel), so items whose u0 lies within 34 eps of a boundary are left out of t' (<= 1 %)
    org' = org + t dir                            3 eps of |org| + |t dir|
Directions agree within 1e-6 per component, generator states are equal, and the alive flags are equal except where the roulette draw q
lies within 1e-6 (relative) of p (<= 1 % of the items).
Measured on an MI355X: medium 6.1 eps of 67; distance t 1.7 eps of 3, channel pdf 4.0 eps of 7; scatter event (3133 of 4096 alive): throughput
8.0 eps of 65, next distance 1.7 eps of 3, origin 1.1 eps of 3, direction 4.0e-7 of 1e-6; no draw within 1e-6 of p, no u0 near a boundary.

Materials committed through a scene: the hoisted coefficients a render reads (commit.cpp) are not reachable through a hook, so the
textured twin of a material -- the same colours from 1 x 1 textures, which takes the per-hit path of k_shade_principled<2> -- must
render the same frame bit for bit at 64 x 48 x 4 spp."""
import numpy as np
import pytest

import _analytic as A
import _sss_analytic as S
import test_sss_model_cpu as M
from test_sss_model_cpu import EPS

pytestmark = pytest.mark.gpu

SCATTER_BOUND = 65 * EPS
N_STATES = 4096


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def param_words(pa, mat):
    p = pa.make_principled(mat)
    return np.frombuffer(bytes(p), np.float32).copy()


def test_medium_matches_the_model(pa):
    mats = M.medium_inputs()
    x = np.stack([param_words(pa, m) for m in mats])
    assert x.shape[1] == 25
    got = pa.api.leaf_eval(pa.api.LEAF_SSS_MEDIUM, x, 23)
    worst = M.check_medium(got, mats, "gpu")
    print(f"gpu medium against the model: max relative error {worst:.2e} = {worst / EPS:.1f} eps (bound {M.MEDIUM_BOUND:.2e} = 67 eps)")


def test_scatter_distance_matches_the_model(pa):
    x = M.distance_inputs()
    got = pa.api.leaf_eval(pa.api.LEAF_SSS_DISTANCE, x, 8)
    assert np.array_equal(got[:, 0:4].view(np.uint32), got[:, 4:8].view(np.uint32)), "a precomputed albedo changes the distance or the channel pdf"
    rt, rp, near = M.check_distance(got[:, 0], got[:, 1:4], x, "gpu")
    print(f"gpu scatter distance against the model: t {rt:.2e} = {rt / EPS:.1f} eps (bound 3 eps), channel pdf {rp:.2e} = {rp / EPS:.1f} eps "
          f"(bound 7 eps); {near:.2%} of the items within {M.BOUNDARY} of a boundary")


def walk_states(n=N_STATES, seed=17):
    """seeded walk states as float32 words (n, 21) in op 13's layout: media of random materials, throughputs 0.03 .. 3, a distance drawn
    from one channel and cut to sigma_t t <= 8, step indices that include the last two, random generator states and odd increments"""
    rng = np.random.RandomState(seed)
    med = [S.medium(m) for m in M.medium_inputs(96, seed + 1) if M.i_ok(m)]
    x = np.zeros((n, 21), np.float32)
    w = x.view(np.uint32)
    for i in range(n):
        m = med[i % len(med)]
        d = rng.normal(size=3)
        x[i, 0:3], x[i, 3:6] = rng.uniform(-1.0, 1.0, 3), d / np.linalg.norm(d)
        x[i, 6:9], x[i, 9:12] = m["sigma_t"], m["sigma_s"]
        x[i, 12:15] = 10.0 ** rng.uniform(-1.5, 0.5, 3)
        st = x[i, 6:9].astype(np.float64)
        x[i, 15] = min(-np.log(1.0 - rng.random_sample()) / st[rng.randint(3)], 8.0 / st.max())
        w[i, 16] = (8191, 8192)[(i // 64) % 2] if i % 64 == 63 else rng.randint(0, 8000)
        w[i, 17:19] = rng.randint(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        w[i, 19] = rng.randint(0, 2 ** 32, dtype=np.uint64) | 1
        w[i, 20] = rng.randint(0, 2 ** 32, dtype=np.uint64)
    return x


def test_scatter_event_matches_the_model(pa):
    x = walk_states()
    w = x.view(np.uint32)
    got = pa.api.leaf_eval(pa.api.LEAF_SSS_SCATTER, x, 15)
    gw = got.view(np.uint32)
    assert (got[:, 14] == 1.0).all(), "k_sss_step's and k_sss_walk's way of calling sss_scatter disagree"
    u64 = lambda lo, hi: lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))      # noqa: E731
    with np.errstate(invalid="ignore"):                       # (the integer words are NaN patterns to a float cast; they are not read as floats)
        xd = x.astype(np.float64)
    state, inc = u64(w[:, 17], w[:, 18]), u64(w[:, 19], w[:, 20])
    ev = S.walk_event(xd[:, 0:3], xd[:, 3:6], xd[:, 6:9], xd[:, 9:12], xd[:, 12:15], xd[:, 15], w[:, 16], state, inc)
    assert (xd[:, 6:9] * xd[:, 15:16]).max() <= 8.0 * (1 + 1e-6)
    alive = got[:, 0] == 1.0
    close = np.abs(ev["q"] - ev["p"]) <= 1e-6 * ev["p"]
    assert close.mean() <= 0.01
    assert np.array_equal(alive[~close], ev["alive"][~close]), np.nonzero(alive != ev["alive"])[0][:8]
    last = w[:, 16] == 8192
    assert last.sum() >= 16 and not alive[last].any() and (w[:, 16] == 8191).sum() >= 16 and alive[w[:, 16] == 8191].any(), "the walk ends past 8192 steps, not before"
    assert 0.2 < alive.mean() < 0.9, alive.mean()
    # a walk that ends leaves its state as it came
    dead = ~alive
    assert np.array_equal(gw[dead][:, 1:14], np.concatenate([w[dead][:, 0:6], w[dead][:, 12:19]], 1))
    ok = alive & ev["alive"]
    assert np.array_equal(u64(gw[ok, 12], gw[ok, 13]), ev["rng_state"][ok]), "generator states differ"
    assert np.array_equal(gw[ok, 11], ev["bounce"][ok].astype(np.uint32))
    with np.errstate(invalid="ignore"):
        g = got[ok].astype(np.float64)
    d_dir = np.abs(g[:, 4:7] - ev["dir"][ok]).max()
    assert d_dir <= 1e-6, d_dir
    r_thr = np.abs(g[:, 7:10] / ev["thr"][ok] - 1.0).max()
    assert r_thr <= SCATTER_BOUND, r_thr / EPS
    scale = np.abs(xd[ok, 0:3]) + np.abs(xd[ok, 15:16] * xd[ok, 3:6])
    r_org = (np.abs(g[:, 1:4] - ev["org"][ok]) / scale).max()
    assert r_org <= 3 * EPS, r_org / EPS
    b = S.channel_boundaries(ev["next_pdf"][ok])
    near = (np.abs(ev["u0"][ok][:, None] - b) <= 34 * EPS).any(1)
    assert near.mean() <= 0.01
    r_t = np.abs(g[~near, 10] / ev["t_scatter"][ok][~near] - 1.0).max()
    assert r_t <= 3 * EPS, r_t / EPS
    assert sorted(set(ev["channel"][ok])) == [0, 1, 2]
    print(f"gpu scatter event against the model ({ok.sum()} alive of {len(x)}): throughput {r_thr:.2e} = {r_thr / EPS:.1f} eps (bound 65 eps), "
          f"distance {r_t / EPS:.1f} eps (bound 3), origin {r_org / EPS:.1f} eps (bound 3), direction {d_dir:.1e} (bound 1e-6); "
          f"{close.sum()} roulette draws within 1e-6 of p, {near.sum()} u0 within 34 eps of a boundary")


def _build_with_zero_texcoords(scene, S_, make_principled):
    """_analytic.build for a one-mesh scene, with texcoords (0, 0) at every vertex: a hit's uv is then exactly 0 and the bilinear fetch
    returns the 1 x 1 texture's texel itself (weights 1, 0, 0, 0)"""
    (m,) = S_.meshes
    mid = scene.AddMaterialParam(make_principled(m.material))
    v4 = np.concatenate([np.asarray(m.verts, np.float32), np.ones((len(m.verts), 1), np.float32)], 1)
    f = np.asarray(m.faces, np.uint32)
    mesh = scene.AddTriangleMesh(v4, None, np.zeros((len(v4), 2), np.float32), f, None, f, np.full(len(f), mid, np.uint32))
    ls = scene.CreateLocalScene()
    scene.AddMeshToLocalScene(ls, mesh)
    scene.CreateInstance(ls, None)
    scene.CommitScene()
    return scene


def test_committed_material_renders_like_its_textured_twin(pa):
    """the coefficients commit hoists (Material::sss_sigt / sss_sigs / sss_wthr, read by k_shade_principled<1>) against the per-hit
    path (k_shade_principled<2>: ParamToBsdf and medium_coefficients at every hit): the same frame, bit for bit"""
    import test_sss_radiance as R
    base, sc = (0.75, 0.5, 0.25), (0.5, 0.25, 0.75)
    mat = A.material(subsurface=0.5, base_color=base, subsurface_color=sc, subsurface_radius=(0.3, 0.2, 0.1), specular=0.0)
    frames = []
    for textured in (False, True):
        sg = pa.Scene()
        m = dict(mat)
        if textured:
            m["base_color_tex_id"] = sg.AddTexture(np.array(base, np.float32).reshape(1, 1, 3))
            m["subsurface_color_tex_id"] = sg.AddTexture(np.array(sc, np.float32).reshape(1, 1, 3))
            m["base_color"], m["subsurface_color"] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)       # (the textures alone carry the colours)
        _build_with_zero_texcoords(sg, R.slab_scene(m), pa.make_principled)
        sg.SetEnvironment(np.tile(R.L_ENV.astype(np.float32), (4, 8, 1)), 1.0, None)
        sg.SetCamera(R.EYE, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), R.FOV)
        layer = pa.RenderLayer()
        pa.Render(sg, 64, 48, 4, layer=layer, seed_seq=R.SEED_SEQ)
        frames.append((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)))
        sg.close()
    assert frames[0][0][..., :3].any() and np.array_equal(frames[0][1], frames[1][1])
    assert frames[0][0].tobytes() == frames[1][0].tobytes(), "the hoisted medium and the per-hit medium render different frames"
