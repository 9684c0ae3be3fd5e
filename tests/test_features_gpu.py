"""First-hit feature buffers (pbrhip_render_features) on the GPU.  Every expected value is built in numpy from the
existing hooks -- Scene.CameraRays, Scene.trace_closest, Scene.texture_fetch -- and the scene description, never from the function
under test: the hit count, the depth sum and the albedo sum bit for bit, the normal sum against float64 within 8 x 2^-24 per
component and sample, and the result's independence of the schedule."""
import ctypes as C

import numpy as np
import pytest

NONE = 0xFFFFFFFF
EPS = 2.0 ** -24
ESTATE, EINVAL = -6, -1
SEED = 1234567890

# name -> eye, lookat, up, fov, lens radius, focus distance (None: the reference's camera)
LENS_CAMERAS = {
    "cornell": ((0.6, 0.3, 5.2), (0.0, -0.1, 0.0), (0.0, 1.0, 0.0), 38.0, 0.05, 0.0),
    "hair": ((1.5, 0.8, 4.5), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 40.0, 0.04, 0.0),
    "instanced": ((0.4, 0.9, 6.0), (0.0, 0.0, 0.0), (0.1, 1.0, 0.0), 42.0, 0.06, 5.5),
    "textured": ((0.3, 0.6, 5.0), (0.0, -0.3, 0.0), (0.0, 1.0, 0.0), 40.0, 0.03, 0.0),
}


def _pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _desc(name):
    from pbrlab_amd import scenes
    if name == "cornell":
        return scenes.cornell_scene("ggx", monkey_subdiv=2, lucy_nu=64, lucy_nv=12)
    if name == "hair":  # hair coloured by RGB: its albedo is the parameter (melanin: test_melanin_albedo)
        d = scenes.hair_scene(n_strands=1500, n_segments=6, head_subdiv=2)
        d.curves[0].material = dict(d.curves[0].material, coloring_hair=0, base_color=(0.31, 0.17, 0.08))
        return d
    if name == "hair_melanin":
        return scenes.hair_scene(n_strands=1500, n_segments=6, head_subdiv=2)
    if name == "instanced":  # flat and smooth meshes under rotations, non-uniform scales and translations
        d = scenes.cornell_scene("ggx", monkey_subdiv=2, lucy_nu=64, lucy_nv=12)
        for sh in d.shapes:
            if sh.name == "monkey":
                sh.transform = scenes.instance_matrix((20.0, 35.0, -10.0), (1.3, 0.8, 1.1), (0.2, 0.25, 0.3))
            elif sh.name == "lucy":
                sh.transform = scenes.instance_matrix((0.0, 50.0, 15.0), (0.9, 1.2, 0.9), (-0.15, 0.1, 0.35))
            elif sh.name == "box":
                sh.transform = scenes.instance_matrix((10.0, 30.0, 25.0), (1.5, 2.0, 1.2), (0.1, 0.9, -0.5))
            elif sh.name == "back":
                sh.transform = scenes.instance_matrix((0.0, 0.0, 0.0), (0.8, 0.8, 1.0), (0.0, 0.0, 0.0))
        return d
    if name == "textured":
        return scenes.textured_cornell_scene(monkey_subdiv=2, lucy_nu=64, lucy_nv=12)
    raise KeyError(name)


_cache = {}


def _scene(name, builder=0):
    """(description, committed scene) -- one per name and builder for the module"""
    key = (name, builder)
    if key not in _cache:
        pa = _pa()
        d = _desc(name)
        _cache[key] = (d, pa.scene_from_desc(d, bvh_builder=builder))
    return _cache[key]


def _set_camera(s, cam):
    if cam is None:
        s.SetCamera(None)
    else:
        s.SetCamera(*cam)


def _hooks(s, W, H, first_pass, passes, seed=SEED):
    """rays and closest hits of every (pass, y, x) from the hooks: arrays shaped (passes, H, W)"""
    yy, xx = np.mgrid[0:H, 0:W]
    xyp = np.stack([np.broadcast_to(xx, (passes, H, W)), np.broadcast_to(yy, (passes, H, W)),
                    np.broadcast_to(np.arange(first_pass, first_pass + passes)[:, None, None], (passes, H, W))], -1)
    rays = s.CameraRays(W, H, xyp.reshape(-1, 3), seed_seq=seed)
    hits = s.trace_closest(rays)
    return rays.reshape(passes, H, W), hits.reshape(passes, H, W)


def _sum32(per_sample):
    """float32 sum over axis 0 in ascending order (one rounding per addition)"""
    acc = np.zeros(per_sample.shape[1:], np.float32)
    for p in range(per_sample.shape[0]):
        acc = (acc + per_sample[p].astype(np.float32)).astype(np.float32)
    return acc


def _materials_of_hits(desc, hits):
    """index into `colours`, per hit sample (-1: a miss), and the float32 colour table: a shape's faces carry their material id, a
    curve mesh its own hair material (build_scene's instance order: shapes, then curves)"""
    colours = [m["base_color"] for m in desc.materials] + [c.material["base_color"] for c in desc.curves]
    idx = np.full(hits.shape, -1, np.int64)
    inst, prim = hits["instance_id"], hits["prim_id"]
    for i, sh in enumerate(desc.shapes):
        m = inst == i
        idx[m] = sh.material_ids[prim[m]]
    for j, _ in enumerate(desc.curves):
        idx[inst == len(desc.shapes) + j] = len(desc.materials) + j
    assert ((idx >= 0) == (inst != NONE)).all()
    return idx, np.asarray(colours, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "hair", "instanced"])
def test_bit_exact_against_the_hooks(name):
    pa = _pa()
    desc, s = _scene(name)
    seen_hit = seen_miss = False
    for cam in (None, LENS_CAMERAS[name]):
        _set_camera(s, cam)
        for (W, H), first_pass, passes in (((61, 47), 0, 6), ((33, 75), 5, 4)):
            rays, hits = _hooks(s, W, H, first_pass, passes)
            hit = hits["instance_id"] != NONE
            if cam is not None:
                assert hit.any() and (~hit).any(), (name, "a user-camera case must see hits and misses")
            seen_hit, seen_miss = seen_hit or hit.any(), seen_miss or (~hit).any()
            f = pa.RenderFeatures(s, W, H, passes, first_pass=first_pass, seed_seq=SEED)
            assert (f.count == passes).all()
            assert np.array_equal(f.albedo[..., 3], hit.sum(0).astype(np.float32)), (name, cam is not None, W, H)
            want_t = _sum32(np.where(hit, hits["t"], np.float32(0)))
            assert np.array_equal(_bits(f.normal_depth[..., 3]), _bits(want_t)), (name, cam is not None, W, H)
            idx, colours = _materials_of_hits(desc, hits)
            col = np.where(hit[..., None], colours[np.maximum(idx, 0)], np.float32(0))
            want_a = np.stack([_sum32(col[..., k]) for k in range(3)], -1)
            assert np.array_equal(_bits(f.albedo[..., :3]), _bits(want_a)), (name, cam is not None, W, H)
    assert seen_hit and seen_miss, name
    s.SetCamera(None)


def _expected_normals(desc, rays, hits):
    """float64 feature normal per sample (zeros for a miss) and the mask of samples whose flip is well conditioned"""
    d = rays["dir"].astype(np.float64)
    n = np.zeros(hits.shape + (3,))
    inst, prim = hits["instance_id"], hits["prim_id"]
    u, v = hits["u"].astype(np.float64), hits["v"].astype(np.float64)
    curve = np.zeros(hits.shape, bool)
    for i, sh in enumerate(desc.shapes):
        m = inst == i
        if not m.any():
            continue
        if sh.normal_ids is None:  # CalcGeometryNormal of the mesh's own (local) corners
            p = desc.vertices[sh.vertex_ids[prim[m]]][..., :3].astype(np.float64)
            nn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])
        else:
            c = desc.normals[sh.normal_ids[prim[m]]][..., :3].astype(np.float64)
            nn = (1 - u[m] - v[m])[:, None] * c[:, 0] + u[m][:, None] * c[:, 1] + v[m][:, None] * c[:, 2]
        n[m] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    for j, cs in enumerate(desc.curves):
        m = inst == len(desc.shapes) + j
        if not m.any():
            continue
        assert cs.transform is None
        cp = cs.vertices[cs.indices[prim[m]][:, None] + np.arange(4)[None, :]][..., :3].astype(np.float64)
        uu = u[m][:, None]
        t = 3 * (1 - uu) ** 2 * (cp[:, 1] - cp[:, 0]) + 6 * uu * (1 - uu) * (cp[:, 2] - cp[:, 1]) + 3 * uu ** 2 * (cp[:, 3] - cp[:, 2])
        n[m] = t / np.linalg.norm(t, axis=1, keepdims=True)
        curve |= m
    dn = (d * n).sum(-1)
    flip = (dn > 0) & ~curve
    n[flip] = -n[flip]
    hit = inst != NONE
    good = ~hit | curve | (np.abs(dn) >= 1e-4)
    return n, good, curve


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "hair", "instanced"])
def test_normals_against_float64(name):
    pa = _pa()
    desc, s = _scene(name)
    for cam in (None, LENS_CAMERAS[name]):
        _set_camera(s, cam)
        W, H, passes = 61, 47, 6
        rays, hits = _hooks(s, W, H, 0, passes)
        hit = hits["instance_id"] != NONE
        n, good, curve = _expected_normals(desc, rays, hits)
        assert (~good).sum() <= 1e-3 * hit.sum(), (name, int((~good).sum()), int(hit.sum()))
        f = pa.RenderFeatures(s, W, H, passes, seed_seq=SEED)
        pix_ok = good.all(0)
        # 8 x 2^-24 per component and hit sample; a cubic's derivative: x 4
        bound = EPS * 8 * (hit & ~curve).sum(0) + EPS * 32 * curve.sum(0)
        err = np.abs(f.normal_depth[..., :3].astype(np.float64) - n.sum(0)).max(-1)
        print(f"{name} cam={'lens' if cam else 'ref'}: max normal-sum error / bound = {np.max(err[pix_ok] / np.maximum(bound[pix_ok], EPS)):.3f}")
        assert (err[pix_ok] <= bound[pix_ok]).all(), (name, float((err[pix_ok] - bound[pix_ok]).max() / EPS))
    s.SetCamera(None)


@pytest.mark.gpu
def test_textured_albedo_is_the_shading_kernels_fetch():
    pa = _pa()
    desc, s = _scene("textured")
    f32 = np.float32
    for cam in (None, LENS_CAMERAS["textured"]):
        _set_camera(s, cam)
        W, H, passes = 61, 47, 5
        rays, hits = _hooks(s, W, H, 0, passes)
        hit = hits["instance_id"] != NONE
        idx, colours = _materials_of_hits(desc, hits)
        col = np.where(hit[..., None], colours[np.maximum(idx, 0)], f32(0)).astype(f32)
        inst, prim, u, v = hits["instance_id"], hits["prim_id"], hits["u"], hits["v"]
        textured = 0
        for i, sh in enumerate(desc.shapes):
            for mat in np.unique(sh.material_ids):
                tex = desc.materials[int(mat)]["base_color_tex_id"]
                if tex == NONE:
                    continue
                m = (inst == i) & hit
                m[m] = sh.material_ids[prim[m]] == mat
                if not m.any():
                    continue
                uu, vv = u[m].astype(f32), v[m].astype(f32)
                if sh.texcoord_ids is None:  # no texcoords: the barycentrics
                    tu, tv = uu, vv
                else:  # make_surface: w0 = 1 - u - v; w0 t0 + u t1 + v t2, one float32 rounding per operation
                    tc = desc.texcoords[sh.texcoord_ids[prim[m]]].astype(f32)
                    w0 = ((f32(1) - uu).astype(f32) - vv).astype(f32)
                    tu = (((w0 * tc[:, 0, 0]).astype(f32) + (uu * tc[:, 1, 0]).astype(f32)).astype(f32) + (vv * tc[:, 2, 0]).astype(f32)).astype(f32)
                    tv = (((w0 * tc[:, 0, 1]).astype(f32) + (uu * tc[:, 1, 1]).astype(f32)).astype(f32) + (vv * tc[:, 2, 1]).astype(f32)).astype(f32)
                col[m] = s.texture_fetch(int(tex), np.stack([tu, tv], 1))
                textured += int(m.sum())
        assert textured > 100, "the camera must see the textured floor and walls"
        f = pa.RenderFeatures(s, W, H, passes, seed_seq=SEED)
        want = np.stack([_sum32(col[..., k]) for k in range(3)], -1)
        assert np.array_equal(_bits(f.albedo[..., :3]), _bits(want)), ("lens" if cam else "ref")
    s.SetCamera(None)


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in ((a.albedo, b.albedo), (a.normal_depth, b.normal_depth), (a.count, b.count)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "hair"])
def test_schedule_independence(name):
    pa = _pa()
    desc, s = _scene(name)
    _set_camera(s, LENS_CAMERAS[name])
    W, H, passes = 83, 59, 8
    ref = pa.RenderFeatures(s, W, H, passes, first_pass=3, seed_seq=SEED)
    assert ref.albedo[..., 3].max() > 0
    # chunks of two passes (four launches), two shard block sizes, the other tree builder
    assert _same(ref, pa.RenderFeatures(s, W, H, passes, first_pass=3, seed_seq=SEED, max_paths_in_flight=2 * W * H))
    assert _same(ref, pa.RenderFeatures(s, W, H, passes, first_pass=3, seed_seq=SEED, max_paths_in_flight=1))
    for block in (16, 64):
        assert _same(ref, pa.RenderFeatures(s, W, H, passes, first_pass=3, seed_seq=SEED, shard_block=block))
    _, s2 = _scene(name, builder=1)
    _set_camera(s2, LENS_CAMERAS[name])
    assert _same(ref, pa.RenderFeatures(s2, W, H, passes, first_pass=3, seed_seq=SEED))
    s2.SetCamera(None)
    # three ranks: disjoint pixels, everything else left as it is (zero): their sum is the frame
    parts = [pa.RenderFeatures(s, W, H, passes, first_pass=3, seed_seq=SEED, tile_rank=r, tile_world=3, shard_block=16) for r in range(3)]
    assert sum((p.count > 0).astype(int) for p in parts).max() == 1
    tot = pa.FeatureLayer(W, H)
    for p in parts:
        tot.albedo += p.albedo
        tot.normal_depth += p.normal_depth
        tot.count += p.count
    assert _same(ref, tot)
    # progressive: [3, 7) then [7, 11) on top == [3, 11) at once
    prog = pa.RenderFeatures(s, W, H, 4, first_pass=3, seed_seq=SEED)
    pa.RenderFeatures(s, W, H, 4, prog, first_pass=7, seed_seq=SEED, no_clear=True)
    assert _same(ref, prog)
    s.SetCamera(None)


@pytest.mark.gpu
def test_rendering_is_not_disturbed():
    pa = _pa()
    _, s = _scene("cornell")
    s.SetCamera(None)
    a, b = pa.RenderLayer(), pa.RenderLayer()
    pa.Render(s, 64, 48, 4, layer=a)
    pa.RenderFeatures(s, 50, 70, 3)
    pa.Render(s, 64, 48, 4, layer=b)
    assert np.array_equal(a.rgba.view(np.uint32), b.rgba.view(np.uint32)) and np.array_equal(a.count, b.count)


@pytest.mark.gpu
def test_melanin_albedo():
    """the colour whose sigma_a under the RGB mapping is the melanin material's: exp(-sqrt(sigma_a) poly(beta_n)); sigma_a restated
    in float32 as hair_param_to_bsdf computes it, the closed form in float64; within 4 x 2^-24 relative"""
    pa = _pa()
    desc, s = _scene("hair_melanin")
    s.SetCamera(None)
    m = desc.curves[0].material
    assert m["coloring_hair"] == 1
    f32 = np.float32
    mel = f32(min(max(m["melanin"], 0.0), 1.0)) * f32(1.0)
    red = f32(min(max(m["melanin_redness"], 0.0), 1.0))
    # the material's log is the fast-math one (fastm::flog): taken from the device's leaf hook, the same single-precision arithmetic
    arg = np.array([[0, max(f32(1) - mel, f32(0.0001)), 0]], f32)
    arg.view(np.uint32)[0, 0] = 3
    mel = -f32(pa.api.leaf_eval(pa.api.LEAF_FASTMATH, arg, 1)[0, 0])
    eu, pheo = f32(mel * f32(f32(1) - red)), f32(mel * red)
    sig = np.array([f32(f32(eu * f32(0.506)) + f32(pheo * f32(0.343))), f32(f32(eu * f32(0.841)) + f32(pheo * f32(0.733))),
                    f32(f32(eu * f32(1.653)) + f32(pheo * f32(1.924)))], np.float64)
    bn = np.float64(f32(m["azimuthal_roughness"]))
    poly = 5.969 - 0.215 * bn + 2.532 * bn ** 2 - 10.73 * bn ** 3 + 5.574 * bn ** 4 + 0.245 * bn ** 5
    want = np.exp(-np.sqrt(sig) * poly)
    W, H = 61, 47
    rays, hits = _hooks(s, W, H, 0, 1)
    on_hair = hits["instance_id"][0] == len(desc.shapes)
    assert on_hair.sum() > 50
    f = pa.RenderFeatures(s, W, H, 1, seed_seq=SEED)
    got = f.albedo[on_hair][:, :3].astype(np.float64)
    rel = np.abs(got - want) / want
    print("melanin albedo", want, "max relative error / 2^-24:", rel.max() / EPS)
    assert (rel <= 4 * EPS).all(), rel.max() / EPS


@pytest.mark.gpu
def test_abi_checks():
    pa = _pa()
    from pbrlab_amd import api
    s = pa.Scene()
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderFeatures(s, 8, 8, 1)
    assert e.value.code == ESTATE
    s.close()
    _, s = _scene("cornell")
    s.SetCamera(None)
    for w, h, n in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
        with pytest.raises(pa.PbrHipError) as e:
            pa.RenderFeatures(s, w, h, n)
        assert e.value.code == EINVAL, (w, h, n)
    # one float buffer not wanted: the others are what they are with it, and nothing else is written
    W, H = 40, 30
    full = pa.RenderFeatures(s, W, H, 3)
    desc = api.RenderDesc(W, H, 3, 0, SEED, 0, 1, 0, 0, 0, 0, 0)
    nd = np.full((H, W, 4), 7.0, np.float32)
    cnt = np.zeros((H, W), np.uint32)
    api._chk(s.L.pbrhip_render_features(s.h, C.byref(desc), None, nd.ctypes.data, cnt.ctypes.data))
    assert np.array_equal(_bits(nd), _bits(full.normal_depth)) and np.array_equal(cnt, full.count)
    al = np.zeros((H, W, 4), np.float32)
    api._chk(s.L.pbrhip_render_features(s.h, C.byref(desc), al.ctypes.data, None, None))
    assert np.array_equal(_bits(al), _bits(full.albedo))


@pytest.mark.gpu
def test_device_variant_gives_the_host_variants_bits():
    import torch
    pa = _pa()
    _, s = _scene("cornell")
    _set_camera(s, LENS_CAMERAS["cornell"])
    W, H = 70, 45
    host = pa.RenderFeatures(s, W, H, 5, first_pass=2)
    a = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
    n = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
    c = torch.full((H, W), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pa.RenderFeatures(s, W, H, 5, first_pass=2, device_out=(a.data_ptr(), n.data_ptr(), c.data_ptr()))
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(host.albedo)) and np.array_equal(_bits(n.cpu().numpy()), _bits(host.normal_depth))
    assert np.array_equal(c.cpu().numpy().astype(np.uint32), host.count)
    s.SetCamera(None)


@pytest.mark.gpu
def test_shim_caller_runs():
    """tests/cpp/shim_features.cc: pbrlab::RenderFeatures (twice, the second call on top) and pbrlab::Denoise through the C++ shim"""
    import os
    import subprocess
    _pa()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib, exe = os.path.join(root, "pbrlab_amd"), os.path.join(root, "tests", "cpp", "shim_features")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_features.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "features ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
