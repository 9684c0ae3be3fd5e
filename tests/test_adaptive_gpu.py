"""Adaptive sampling (pbrhip_render_adaptive) on the GPU.  The decision kernels are held to the numpy model of
tests/_adaptive_model.py as bits; a rendered layer is held to the contract -- pixel p holds, bit for bit, what a plain render of
count[p] passes holds at p -- and its count map, tile errors, sample total and round count to the model's run over plain frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _adaptive_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -6
W, H = 60, 44  # 8 x 6 tiles: a clipped column (4 wide) and a clipped row (4 high)
LENS_CAMERA = ((0.6, 0.3, 5.2), (0.0, -0.1, 0.0), (0.0, 1.0, 0.0), 38.0, 0.05, 0.0)  # a thin lens
INSIDE_CAMERA = ((0.0, 0.0, 0.9), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0)           # inside the box: every pixel sees a lit wall
AWAY_CAMERA = ((0.0, 0.0, 5.0), (0.0, 0.0, 10.0), (0.0, 1.0, 0.0), 40.0)             # looks away from the box: misses only
FAR_CAMERA = ((0.0, 0.0, 5.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0)               # the box covers under half of the frame


def _pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _desc(name):
    from pbrlab_amd import scenes
    if name == "hair":
        return scenes.hair_scene(n_strands=1500, n_segments=6, head_subdiv=2)
    return scenes.cornell_scene("ggx", monkey_subdiv=2, lucy_nu=64, lucy_nv=12)


_scenes, _plain = {}, {}


def _scene(name="cornell", builder=0):
    key = (name, builder)
    if key not in _scenes:
        _scenes[key] = _pa().scene_from_desc(_desc(name), bvh_builder=builder)
    return _scenes[key]


def _frames(tag, s, w, h, **kw):
    """frame_at(n) -> (rgba, count) of a plain Render of n passes; rendered once per (tag, size, n) for the module and never changed"""
    pa = _pa()

    def frame_at(n):
        key = (tag, w, h, n, tuple(sorted(kw.items())))
        if key not in _plain:
            layer = pa.RenderLayer()
            pa.Render(s, w, h, n, layer=layer, **kw)
            _plain[key] = (layer.rgba.copy(), layer.count.copy())
        return _plain[key]
    return frame_at


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _assert_result(r, m):
    """an adaptive layer against the model's run"""
    assert np.array_equal(r.count, m["count"])
    assert _same(r.tile_error, m["tile_error"]), np.abs(r.tile_error - m["tile_error"]).max()
    assert r.samples == m["samples"] == int(r.count.sum(dtype=np.int64)) and r.rounds == m["rounds"]
    assert _same(r.rgba, m["rgba"])


# ---------------------------------------------------------------------------------------------------- 1. the decision kernels
def _crafted(h, w, seed, n_prev, n_now):
    rng = np.random.RandomState(seed)
    A = np.zeros((h, w, 4), np.float32)
    A[..., :3] = (rng.uniform(0, 2, (h, w, 3)) ** 3) * n_prev
    A[..., 3] = n_prev
    I = A.copy()
    noise = rng.uniform(0, 2, (h, w, 3)) ** 3
    calm = rng.uniform(size=(h, w)) < 0.5  # about half the pixels: nearly equal halves
    noise[calm] = A[..., :3][calm] / n_prev * rng.uniform(0.98, 1.02, (int(calm.sum()), 3))
    I[..., :3] += (noise * (n_now - n_prev)).astype(np.float32)
    I[..., 3] = n_now
    # special values, each in a tile of its own where the image has that many tiles
    ty, tx = AM.tiles_across(h), AM.tiles_across(w)
    spots = [(min(h - 1, 8 * (k // tx % ty) + 1), min(w - 1, 8 * (k % tx) + 2)) for k in range(6)]
    I[spots[0]] = A[spots[0]] = 0.0                                    # a black pixel: e = 0 / sqrt(1e-3)
    I[spots[1]][:3], A[spots[1]][:3] = (3e-39, 1e-40, 0.0), (1e-39, 1e-41, 0.0)  # denormals
    if ty * tx >= 6:
        I[spots[2]][:3], A[spots[2]][:3] = (1e30, 2e30, 3e30), (1e30, 1e29, 0.0)
        I[spots[3]][0] = np.inf
        I[spots[4]][1] = np.nan
        I[spots[5]][:3], A[spots[5]][:3] = (3e38, 3e38, 3e38), (1e38, 0.0, 0.0)  # near the top of the range
    return I, A


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n_prev,n_now", [(8, 8, 4, 8), (5, 3, 2, 4), (57, 20, 16, 24), (64, 48, 8, 16)])
def test_decision_kernels_equal_the_model_as_bits(w, h, n_prev, n_now):
    _pa()
    from pbrlab_amd import api
    I, A = _crafted(h, w, 11 + w, n_prev, n_now)
    ntiles = AM.tiles_across(h) * AM.tiles_across(w)
    rng = np.random.RandomState(w)
    tiles = np.arange(ntiles, dtype=np.uint32)
    if (w, h) == (64, 48):  # a subset in scrambled order
        tiles = rng.permutation(ntiles)[:31].astype(np.uint32)
        assert list(tiles) != sorted(tiles)
    err0 = rng.uniform(1, 2, ntiles).astype(np.float32)  # entries of tiles that are not listed stay
    e = AM.pixel_error(I, A, n_prev, n_now)
    Es = np.array([AM.tile_error(e, t, w, h) for t in tiles])
    finite = np.sort(Es[np.isfinite(Es)])
    thresholds = [0.0, float(np.float32(finite[len(finite) // 2])) if len(finite) else 1.0, 1e30]
    for thr in thresholds:
        want = AM.step(I, A, n_prev, n_now, thr, tiles, err0)
        got = api.adaptive_step(I, A, n_prev, n_now, thr, tiles, err0)
        for name, g, m in zip(("tiles_out", "pixels_out", "tile_error", "snapshot"), got, want):
            assert g.shape == m.shape and _same(g, m), (name, thr, g, m)
    if ntiles > 1:  # the middle threshold splits the list
        kept = len(AM.step(I, A, n_prev, n_now, thresholds[1], tiles)[0])
        assert 0 < kept < len(tiles)
    got = api.adaptive_step(I, A, n_prev, n_now, 0.5, np.zeros(0, np.uint32), err0)  # an empty list: nothing happens
    assert len(got[0]) == 0 and len(got[1]) == 0 and _same(got[2].reshape(-1), err0) and _same(got[3], A)


# ---------------------------------------------------------------------------------------------------- 2. the contract
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "hair", "lens"])
def test_every_pixel_is_a_plain_render_of_its_count(name):
    pa = _pa()
    s = _scene("hair" if name == "hair" else "cornell")
    if name == "lens":
        s.SetCamera(*LENS_CAMERA)
    try:
        frame_at = _frames(name, s, W, H)
        threshold = 0.1  # chosen on the model over the oracle's frames: the model stops a good half of the tiles
        m = AM.run(frame_at, W, H, 32, threshold, first_level=2)
        stopped = float((m["count"] < 32).mean())
        print(f"{name}: the model stops {stopped:.3f} of the pixels before the maximum; levels {np.unique(m['count'])}")
        assert 0.1 < stopped < 0.9
        r = pa.RenderAdaptive(s, W, H, 32, threshold=threshold, first_level=2)
        F = {n: frame_at(n)[0] for n in (4, 8, 16, 32)}
        assert set(np.unique(r.count)) <= set(F)
        for n, fn in F.items():
            at = r.count == n
            assert _same(r.rgba[at], fn[at]), (name, n)
        _assert_result(r, m)
        assert r.rounds == 5 and (r.rgba[..., 3] == r.count).all()
    finally:
        s.SetCamera(None)


# ---------------------------------------------------------------------------------------------------- 3. limits
@pytest.mark.gpu
def test_limits():
    pa = _pa()
    s = _scene()
    npix = W * H
    try:
        s.SetCamera(*INSIDE_CAMERA)
        frame_at = _frames("inside", s, W, H)
        r = pa.RenderAdaptive(s, W, H, 16, threshold=0.0, first_level=4)  # no tile of a lit, noisy view has E == 0
        assert _same(r.rgba, frame_at(16)[0]) and (r.count == 16).all() and r.samples == npix * 16 and r.rounds == 3
        assert (r.tile_error > 0).all()
        r = pa.RenderAdaptive(s, W, H, 64, threshold=1e30, first_level=4)  # everything stops at the first decision
        assert (r.count == 8).all() and _same(r.rgba, frame_at(8)[0]) and r.rounds == 2 and r.samples == npix * 8
        r = pa.RenderAdaptive(s, W, H, 6, threshold=1e30, first_level=4)   # min(2 first_level, max)
        assert (r.count == 6).all() and _same(r.rgba, frame_at(6)[0]) and r.rounds == 2
        for first in (16, 100):  # first_level >= max: one plain round, no decision
            r = pa.RenderAdaptive(s, W, H, 16, threshold=1e30, first_level=first)
            assert r.rounds == 1 and _same(r.rgba, frame_at(16)[0]) and not r.tile_error.any()
        fin = C.c_size_t(99)
        r = pa.RenderAdaptive(s, W, H, 24, threshold=0.0, first_level=4, finish_pass=fin)  # levels 4, 8, 16, 24
        assert r.rounds == 4 and (r.count == 24).all() and _same(r.rgba, frame_at(24)[0]) and fin.value == 24
        _assert_result(r, AM.run(frame_at, W, H, 24, 0.0, first_level=4))
        r = pa.RenderAdaptive(s, W, H, 64, threshold=0.05)  # first_level 0 = 8
        assert r.count.min() >= 16 and _same(r.rgba[r.count == 16], frame_at(16)[0][r.count == 16])
        s.SetCamera(*AWAY_CAMERA)
        r = pa.RenderAdaptive(s, W, H, 64, threshold=0.0, first_level=4)  # misses only: E == 0 <= 0
        assert (r.count == 8).all() and not r.rgba[..., :3].any() and not r.tile_error.any() and r.rounds == 2
    finally:
        s.SetCamera(None)


# ---------------------------------------------------------------------------------------------------- 4. schedule independence
@pytest.mark.gpu
def test_schedule_independence():
    pa = _pa()
    base = None
    for name in ("cornell", "hair"):
        s = _scene(name)
        kw = dict(threshold=0.1, first_level=2)
        base = pa.RenderAdaptive(s, W, H, 32, **kw)
        assert 0.1 < (base.count < 32).mean() < 0.9
        variants = [dict(max_paths_in_flight=3 * W * H), dict(max_paths_in_flight=700), dict(num_streams=2), dict(tail_paths=0xFFFFFFFF)]
        for v in variants:
            r = pa.RenderAdaptive(s, W, H, 32, **kw, **v)
            assert _same(r.rgba, base.rgba) and _same(r.count, base.count) and _same(r.tile_error, base.tile_error), (name, v)
            assert (r.samples, r.rounds) == (base.samples, base.rounds)
    from pbrlab_amd import api
    for builder in (api.BVH_HOST_SAH, api.BVH_GPU_LBVH_WIDE):  # (hair: `base` is the host-built scene's)
        r = pa.RenderAdaptive(_scene("hair", builder), W, H, 32, threshold=0.1, first_level=2)
        assert _same(r.rgba, base.rgba) and _same(r.count, base.count) and _same(r.tile_error, base.tile_error), builder


# ---------------------------------------------------------------------------------------------------- 5. shards
@pytest.mark.gpu
def test_shards():
    pa = _pa()
    s = _scene()
    kw = dict(threshold=0.1, first_level=2)
    one = pa.RenderAdaptive(s, W, H, 32, **kw)
    rgba, count, err = np.zeros_like(one.rgba), np.zeros_like(one.count), np.zeros_like(one.tile_error)
    samples = 0
    for rank in range(3):
        r = pa.RenderAdaptive(s, W, H, 32, tile_rank=rank, tile_world=3, shard_block=8, **kw)
        mine = AM.rank_tiles(W, H, rank, 3, 8)
        other = np.ones(err.size, bool)
        other[mine] = False
        assert not r.tile_error.reshape(-1)[other].any() and (r.count > 0).sum() == sum(len(AM.tile_pixels(t, W, H)) for t in mine)
        assert not (count[r.count > 0]).any()  # disjoint
        rgba += r.rgba  # (x + 0 is x: disjoint shards add up exactly)
        count += r.count
        err += r.tile_error
        samples += r.samples
    assert _same(rgba, one.rgba) and _same(count, one.count) and _same(err, one.tile_error) and samples == one.samples
    r = pa.RenderAdaptive(s, W, H, 32, tile_rank=50, tile_world=64, shard_block=8, **kw)  # 48 blocks: rank 50 has none
    assert not r.rgba.any() and not r.count.any() and not r.tile_error.any() and r.samples == 0 and r.rounds == 0
    r = pa.RenderAdaptive(s, W, H, 32, shard_block=16, **kw)
    assert _same(r.rgba, one.rgba) and _same(r.count, one.count)
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderAdaptive(s, W, H, 32, shard_block=12, **kw)
    assert e.value.code == EINVAL


# ---------------------------------------------------------------------------------------------------- 6. refusals and state
@pytest.mark.gpu
def test_refusals_and_state(oracle):
    pa = _pa()
    from pbrlab_amd import api
    desc = _desc("cornell")
    s = pa.scene_from_desc(desc)
    for kw in (dict(flags=api.RENDER_NO_CLEAR), dict(threshold=-0.5), dict(threshold=float("nan"))):
        with pytest.raises(pa.PbrHipError) as e:
            pa.RenderAdaptive(s, W, H, 8, **kw)
        assert e.value.code == EINVAL, kw
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderAdaptive(s, W, H, 0)
    assert e.value.code == EINVAL
    fresh = pa.Scene()
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderAdaptive(fresh, W, H, 8)
    assert e.value.code == ESTATE
    before = pa.RenderAdaptive(s, W, H, 16, threshold=0.1, first_level=2)
    # a stale scene is refused and works again after the refit (the same vertices: the same frame)
    s.UpdateTriangleMesh(0, desc.vertices)
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderAdaptive(s, W, H, 16, threshold=0.1, first_level=2)
    assert e.value.code == ESTATE
    s.RefitScene()
    after = pa.RenderAdaptive(s, W, H, 16, threshold=0.1, first_level=2)
    assert _same(after.rgba, before.rgba) and _same(after.count, before.count)
    # the pixel cache is intact: plain renders after an adaptive call still equal the oracle's
    so = oracle.oracle_scene_from_desc(desc)
    rgba, count, _ = so.render(W, H, 2, threads=oracle.oracle_threads(), math_mode=oracle.MATH_DEVICE)
    for render in (lambda layer: pa.Render(s, W, H, 2, layer=layer), lambda layer: pa.RenderMulti([s], W, H, 2, layer=layer)):
        layer = pa.RenderLayer()
        render(layer)
        assert np.array_equal(layer.count, count)
        diff = np.abs(layer.rgba - rgba).max(axis=2) > 0
        rel = np.linalg.norm(layer.rgba[..., :3] - rgba[..., :3]) / np.linalg.norm(rgba[..., :3])
        assert diff.mean() < 1e-3 and rel < 1e-4, (int(diff.sum()), float(rel))  # (smoke()'s bound: rare last-ulp libm events)
    # a cancel flag set before the call: OK, nothing rendered
    flag, fin = C.c_ubyte(1), C.c_size_t(7)
    r = pa.RenderAdaptive(s, W, H, 16, cancel_render_flag=flag, finish_pass=fin)
    assert not r.count.any() and not r.rgba.any() and r.samples == 0 and r.rounds == 0 and fin.value == 0 and not r.tile_error.any()


@pytest.mark.gpu
def test_device_variant_gives_the_host_variants_bits():
    pa = _pa()
    import torch
    s = _scene()
    host = pa.RenderAdaptive(s, W, H, 32, threshold=0.1, first_level=2)
    rgba = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
    count = torch.full((H, W), 7, dtype=torch.int32, device="cuda:0")
    err = torch.full(host.tile_error.shape, 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    samples, rounds = pa.api.RenderAdaptive(s, W, H, 32, threshold=0.1, first_level=2, device_out=(rgba.data_ptr(), count.data_ptr(), err.data_ptr()))
    assert (samples, rounds) == (host.samples, host.rounds)
    assert _same(rgba.cpu().numpy(), host.rgba) and _same(count.cpu().numpy().view(np.uint32), host.count) and _same(err.cpu().numpy(), host.tile_error)


# ---------------------------------------------------------------------------------------------------- 7. it pays
@pytest.mark.gpu
def test_it_pays_on_a_sparse_view():
    """the open-fronted box from far away: most of the frame is background, which stops at the first decision.  The adaptive frame's
    mean squared error against a reference of 16 x the maximum level, in passes of its own, is below that of the uniform frame that
    took at least as many samples."""
    pa = _pa()
    from pbrlab_amd import api
    s = _scene()
    n = 64
    npix = n * n
    try:
        s.SetCamera(*FAR_CAMERA)
        feat = pa.RenderFeatures(s, n, n, 4)
        covered = float((feat.albedo[..., 3] > 0).mean())
        print(f"covered share of the frame {covered:.3f}")
        assert 0.2 < covered < 0.5
        ref = pa.RenderLayer()
        pa.Render(s, n, n, 16 * 64, layer=ref, first_pass=64)  # disjoint from the passes [0, 64) both frames draw from
        ref_mean = ref.rgba[..., :3].astype(np.float64) / (16 * 64)
        a = pa.RenderAdaptive(s, n, n, 64, threshold=api.ADAPTIVE_THRESHOLD, first_level=4)
        spp = -(-a.samples // npix)  # never fewer samples than the adaptive frame took
        u = pa.RenderLayer()
        pa.Render(s, n, n, spp, layer=u)
        assert int(u.count.sum(dtype=np.int64)) >= a.samples
        mse_a = float(((a.rgba[..., :3].astype(np.float64) / a.count[..., None] - ref_mean) ** 2).mean())
        mse_u = float(((u.rgba[..., :3].astype(np.float64) / spp - ref_mean) ** 2).mean())
        print(f"adaptive: {a.samples} samples ({a.samples / npix:.2f} per pixel, {a.rounds} rounds), uniform: {spp} spp; "
              f"MSE adaptive {mse_a:.4e}, uniform {mse_u:.4e}, ratio {mse_a / mse_u:.3f}")
        assert mse_a / mse_u < 1.0
        out = pa.Denoise(a, feat)  # the filter divides by every pixel's own count
        assert out.shape == (n, n, 4) and np.isfinite(out).all() and (out[..., 3] == 1).all()
    finally:
        s.SetCamera(None)


@pytest.mark.gpu
def test_shim_caller_runs():
    _pa()
    exe = os.path.join(ROOT, "tests", "cpp", "shim_adaptive")
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_adaptive.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "adaptive ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_cli_adaptive(tmp_path):
    """pbrlab-hip-cli --adaptive: --spp is the maximum, the PNG is rgba / count with every pixel's own count (alpha = count / count), and
    --denoise takes the result"""
    _pa()
    import re
    from pbrlab_amd import io_api
    d = str(tmp_path)
    with open(os.path.join(d, "m.mtl"), "w") as f:
        f.write("newmtl white\nbase_color 0.7 0.7 0.7\nspecular 0\n")
    with open(os.path.join(d, "q.obj"), "w") as f:
        f.write("mtllib m.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 1\nv 0.3 -0.3 1\nv 0.3 0.3 1\nv -0.3 0.3 1\n"
                "usemtl white\no floor\nf 1 2 3 4\no light_top\nf 8 7 6 5\n")
    w, h = 72, 40
    for extra in ([], ["--denoise"]):
        r = subprocess.run([io_api.CLI_PATH, "q.obj", "--width", str(w), "--height", str(h), "--spp", "16", "--adaptive", "0.05", "--min-spp", "2",
                            "--out", "a.png"] + extra, cwd=d, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"adaptive: (\d+) samples .* in (\d+) rounds", r.stderr)
        assert m and 4 * w * h <= int(m.group(1)) <= 16 * w * h and 2 <= int(m.group(2)) <= 4, r.stderr
        img = io_api.png_decode(open(os.path.join(d, "a.png"), "rb").read())
        assert img.shape == (h, w, 4) and img[..., 3].min() == 255 and img[..., :3].max() > 0
