"""pbrhip_denoise on the GPU: against the float64 model of tests/_denoise_model.py within a derived rounding bound,
exact properties of the filter, and that it denoises -- measured against the renderer's own convergence.

Measured on an MI355X (profiles/README.md has the table): see the figures the tests print."""
import os
import subprocess

import numpy as np
import pytest

import _denoise_model as DM
from test_features_gpu import _hooks, _pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _synthetic(W, H, seed):
    """random colours over a few planes of distinct normals and depths, background regions and count == 0 holes"""
    import pbrlab_amd as pa
    rng = np.random.RandomState(seed)
    layer, feat = pa.RenderLayer(W, H), pa.FeatureLayer(W, H)
    spp = rng.randint(1, 9, (H, W)).astype(np.uint32)
    yy, xx = np.mgrid[0:H, 0:W]
    region = ((xx * 5) // W + 2 * ((yy * 3) // H)) % 5  # five regions: 0 = background, 1..4 = planes
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [0.48, 0.6, 0.64], [-0.6, 0.64, 0.48]], np.float64)
    hits = np.where(region == 0, 0, spp)
    hits = np.where((region == 3) & (rng.rand(H, W) < 0.3), np.maximum(hits // 2, 1), hits)  # partly covered pixels
    nrm = normals[region] + 0.02 * rng.normal(size=(H, W, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    depth = 2.0 + region + 0.01 * xx + 0.02 * yy * (region % 2)
    alb = rng.uniform(0.05, 0.95, (H, W, 3))
    alb[region == 4] = 0.0  # a black albedo
    feat.albedo[..., :3] = alb * hits[..., None]
    feat.albedo[..., 3] = hits
    feat.normal_depth[..., :3] = nrm * hits[..., None]
    feat.normal_depth[..., 3] = depth * hits
    feat.count[...] = spp
    hole = rng.rand(H, W) < 0.03
    spp_l = np.where(hole, 0, spp).astype(np.uint32)
    layer.rgba[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3)) * spp_l[..., None]
    layer.rgba[..., 3] = spp_l
    layer.count[...] = spp_l
    return layer, feat


@pytest.mark.gpu
@pytest.mark.parametrize("normal_squarings", [7, 0])
def test_against_the_float64_model(normal_squarings):
    """|gpu - model| <= B = iterations (64 + 16 x 2^normal_squarings) 2^-24 max|e0| max(a): an iteration is a convex combination
    (rounding costs <= 64 x 2^-24 of the range and is not amplified), exp(-x) moves a weight by x e^-x O(2^-24), and every squaring
    doubles the relative error of N_p . N_q (~16 x 2^-24)"""
    pa = _pa()
    for (W, H, seed) in ((67, 45, 1), (531, 40, 2)):
        layer, feat = _synthetic(W, H, seed)
        for iterations, sc, sd, albedo in ((5, 0.8, 0.5, True), (3, 0.0, 1.0, True), (5, 0.5, 0.0, False), (1, 2.0, 0.2, True)):
            got = pa.Denoise(layer, feat, iterations=iterations, sigma_color=sc, sigma_depth=sd, normal_squarings=normal_squarings, albedo=albedo)
            want = DM.denoise(layer.rgba, layer.count, feat.albedo, feat.normal_depth, feat.count, iterations, sc, sd, normal_squarings, albedo)
            e0, a = DM.prepare(layer.rgba, layer.count, feat.albedo, feat.normal_depth, feat.count, albedo)[:2]
            B = iterations * (64 + 16 * 2 ** normal_squarings) * EPS * np.abs(e0).max() * a.max()
            err = np.abs(got - want).max()
            print(f"{W}x{H} it={iterations} sc={sc} sd={sd} albedo={albedo} squarings={normal_squarings}: max error {err:.3e}, bound {B:.3e}")
            assert err <= B, (W, H, iterations, sc, sd, albedo, err, B)
        # no features at all: a colour-guided A-trous
        got = pa.Denoise(layer, None, iterations=4, sigma_color=0.7, sigma_depth=0.3, normal_squarings=normal_squarings)
        want = DM.denoise(layer.rgba, layer.count, None, None, None, 4, 0.7, 0.3, normal_squarings)
        mean = np.where(layer.count[..., None] > 0, layer.rgba[..., :3] / np.maximum(layer.count, 1)[..., None], 0)
        assert np.abs(got - want).max() <= 4 * 80 * EPS * np.abs(mean).max()


def _ulp_close(a, b, ulps=2):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (np.abs(a.astype(np.float64) - b) <= ulps * np.spacing(np.abs(b).astype(np.float32))).all()


@pytest.mark.gpu
def test_exact_properties():
    pa = _pa()
    W, H = 67, 45
    layer, feat = _synthetic(W, H, 4)
    valid = layer.count > 0
    # a constant colour comes back constant under any features (no albedo: the colour itself is what is filtered)
    const = pa.RenderLayer(W, H)
    const.count[...] = layer.count
    const.rgba[..., :3] = np.array([0.3, 0.6, 0.9], np.float32) * layer.count[..., None].astype(np.float32)
    out = pa.Denoise(const, feat, albedo=False)
    mean = np.where(valid[..., None], const.rgba[..., :3] / np.maximum(const.count, 1)[..., None].astype(np.float32), 0).astype(np.float32)
    assert _ulp_close(out[valid][:, :3], mean[valid]) and (out[valid][:, 3] == 1).all()
    # holes are (0, 0, 0, 0) and influence nobody
    assert (out[~valid] == 0).all() and (~valid).any()
    base = pa.Denoise(layer, feat)
    loud = pa.RenderLayer(W, H)
    loud.rgba[...], loud.count[...] = layer.rgba, layer.count
    loud.rgba[~valid] = 1e6
    assert np.array_equal(pa.Denoise(loud, feat).view(np.uint32), base.view(np.uint32))
    # two faces with perpendicular normals painted 1 and 0: nothing bleeds
    two, f2 = pa.RenderLayer(W, H), pa.FeatureLayer(W, H)
    left = np.broadcast_to(np.arange(W)[None, :] < W // 2, (H, W))
    two.count[...] = 4
    two.rgba[..., :3] = np.where(left, 4.0, 0.0)[..., None]
    f2.count[...] = 4
    f2.albedo[...] = (4.0, 4.0, 4.0, 4.0)
    f2.normal_depth[..., :3] = np.where(left[..., None], (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))
    f2.normal_depth[..., 3] = 4 * 3.0
    out = pa.Denoise(two, f2)
    assert _ulp_close(out[left][:, :3], 1.0) and (out[~left][:, :3] == 0).all()
    # background pixels only mix with background pixels: surface colours 5, background colours 1 -> the background stays 1
    bg = pa.RenderLayer(W, H)
    is_bg = feat.albedo[..., 3] == 0
    assert is_bg.any() and (~is_bg).any()
    bg.count[...] = 2
    bg.rgba[..., :3] = np.where(is_bg, 2.0, 10.0)[..., None]
    out = pa.Denoise(bg, feat, albedo=False)
    assert _ulp_close(out[is_bg][:, :3], 1.0) and _ulp_close(out[~is_bg][:, :3], 5.0)


def _highpass_energy(img):
    d = img[1:-1, 1:-1] - 0.25 * (img[:-2, 1:-1] + img[2:, 1:-1] + img[1:-1, :-2] + img[1:-1, 2:])
    return float((d * d).sum())


@pytest.mark.gpu
def test_albedo_demodulation_keeps_the_texture():
    """colour = albedo texture x smooth irradiance on one plane: NO_ALBEDO blurs the texture, the default keeps it"""
    pa = _pa()
    W, H = 96, 64
    rng = np.random.RandomState(9)
    yy, xx = np.mgrid[0:H, 0:W]
    tex = (0.2 + 0.6 * (((xx // 3) + (yy // 3)) % 2))[..., None] * np.array([1.0, 0.8, 0.6])
    irr = (0.5 + 0.4 * np.sin(xx / 40.0) * np.cos(yy / 30.0))[..., None]
    layer, feat = pa.RenderLayer(W, H), pa.FeatureLayer(W, H)
    layer.count[...] = 4
    layer.rgba[..., :3] = 4 * tex * irr
    feat.count[...] = 4
    feat.albedo[..., :3] = 4 * tex
    feat.albedo[..., 3] = 4
    feat.normal_depth[...] = (0.0, 0.0, 4.0, 8.0)
    e_in = _highpass_energy(tex * irr)
    e_keep = _highpass_energy(pa.Denoise(layer, feat, sigma_color=0.0)[..., :3])
    e_blur = _highpass_energy(pa.Denoise(layer, feat, sigma_color=0.0, albedo=False)[..., :3])
    print(f"high-frequency energy: input {e_in:.4f}, default {e_keep:.4f}, NO_ALBEDO {e_blur:.4f}")
    assert e_blur < e_in and e_blur < e_keep and abs(e_keep - e_in) < e_in - e_blur


def _rel_mse(img, truth, mask=None):
    d = ((img - truth) ** 2).sum(-1) / ((truth ** 2).sum(-1) + 1e-2)
    return float(d[mask].mean() if mask is not None else d.mean())


def _wall_interiors(s, desc, W, H, passes):
    """pixels whose `passes` samples all hit one and the same wall primitive and that lie >= 8 pixels from any pixel of which that is
    not true (the image border counts as such), from the hooks"""
    rays, hits = _hooks(s, W, H, 0, passes)
    walls = [i for i, sh in enumerate(desc.shapes) if sh.name in ("floor", "ceiling", "back", "left", "right")]
    same = (hits["instance_id"] == hits["instance_id"][0]).all(0) & (hits["prim_id"] == hits["prim_id"][0]).all(0) & np.isin(hits["instance_id"][0], walls)
    interior = same.copy()
    for _ in range(8):
        p = np.pad(interior, 1, constant_values=False)
        interior = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:] & p[:-2, :-2] & p[:-2, 2:] & p[2:, :-2] & p[2:, 2:]
    return interior


@pytest.mark.gpu
def test_it_denoises():
    """Cornell GGX, 256 x 256.  Truth: 4096 spp of passes disjoint from everything else.  Yardsticks: the relative MSE of plain frames at
    8, 16, 32 and 64 spp.  The denoised 8-spp frame (features of the same 8 passes, default parameters) must beat the 8-spp yardstick
    over the frame and the 16-spp yardstick over wall interiors (pixels whose 8 samples all hit one and the same untextured wall
    primitive, >= 8 pixels from any pixel of which that is not true; selected from the hooks)."""
    pa = _pa()
    from pbrlab_amd import scenes
    desc = scenes.cornell_scene("ggx", monkey_subdiv=3, lucy_nu=256, lucy_nv=32)
    s = pa.scene_from_desc(desc)
    W = H = 256

    def mean(first_pass, spp):
        layer = pa.RenderLayer()
        pa.Render(s, W, H, spp, layer=layer, first_pass=first_pass)
        return layer, (layer.rgba[..., :3] / layer.count[..., None]).astype(np.float64)

    truth = mean(1000, 4096)[1]
    yard = {spp: _rel_mse(mean(0, spp)[1], truth) for spp in (8, 16, 32, 64)}
    layer8, noisy = mean(0, 8)
    feat = pa.RenderFeatures(s, W, H, 8)
    out = pa.Denoise(layer8, feat)[..., :3].astype(np.float64)
    interior = _wall_interiors(s, desc, W, H, 8)
    assert interior.sum() > 2000, int(interior.sum())
    yard_w = {spp: _rel_mse(mean(0, spp)[1], truth, interior) for spp in (8, 16, 32, 64)}
    got, got_w = _rel_mse(out, truth), _rel_mse(out, truth, interior)
    print(f"relative MSE, frame: denoised 8 spp {got:.5f}; plain {yard}")
    print(f"relative MSE, wall interiors ({int(interior.sum())} pixels): denoised 8 spp {got_w:.5f}; plain {yard_w}")
    assert got < yard[8], (got, yard)
    assert got_w < yard_w[16], (got_w, yard_w)
    s.close()


@pytest.mark.gpu
def test_device_variant_gives_the_host_variants_bits():
    import torch
    pa = _pa()
    W, H = 67, 45
    layer, feat = _synthetic(W, H, 6)
    host = pa.Denoise(layer, feat, iterations=3)
    t = [torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")
         for a in (layer.rgba, layer.count, feat.albedo, feat.normal_depth, feat.count)]
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pa.DenoiseDevice(0, W, H, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), (t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr()), iterations=3)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32))
    out.zero_()
    torch.cuda.synchronize()
    pa.DenoiseDevice(0, W, H, t[0].data_ptr(), t[1].data_ptr(), out.data_ptr(), None, iterations=2, sigma_depth=0.0)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pa.Denoise(layer, None, iterations=2, sigma_depth=0.0).view(np.uint32))


@pytest.mark.gpu
def test_abi_checks():
    pa = _pa()
    layer, feat = _synthetic(16, 12, 8)
    for kw in (dict(iterations=9), dict(normal_squarings=17), dict(sigma_color=float("nan")), dict(sigma_depth=float("nan"))):
        with pytest.raises(pa.PbrHipError) as e:
            pa.Denoise(layer, feat, **kw)
        assert e.value.code == -1, kw
    assert pa.Denoise(layer, feat, iterations=8, normal_squarings=16).shape == (12, 16, 4)


@pytest.mark.gpu
def test_cli_aov_and_denoise(tmp_path):
    """--aov writes three decodable PNGs of the image's size, --denoise an image that differs from the plain one (the plain one is what
    tests/test_io_gpu.py pins byte for byte)"""
    _pa()
    from pbrlab_amd import io_api
    from test_io_gpu import _write_scene_files
    d = str(tmp_path)
    files = _write_scene_files(d, "textured", False)
    W, H = 96, 64
    common = [io_api.CLI_PATH] + files + ["--width", str(W), "--height", str(H), "--spp", "8"]
    plain, den, aov = os.path.join(d, "plain.png"), os.path.join(d, "den.png"), os.path.join(d, "aov")
    for extra in (["--out", plain], ["--out", den, "--denoise", "--aov", aov, "--feature-spp", "4"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = (io_api.png_decode(open(f, "rb").read()) for f in (plain, den))
    assert a.shape == b.shape == (H, W, 4) and not np.array_equal(a, b)
    imgs = {kind: io_api.png_decode(open(f"{aov}.{kind}.png", "rb").read()) for kind in ("albedo", "normal", "depth")}
    for kind, img in imgs.items():
        assert img.shape[:2] == (H, W) and img[..., :3].std() > 1, (kind, img.shape)
    # --gpus 2 with the flags: features and filter run on the first GPU over the gathered layer -- the same files
    den2 = os.path.join(d, "den2.png")
    r = subprocess.run(common + ["--out", den2, "--denoise", "--feature-spp", "4", "--gpus", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(io_api.png_decode(open(den2, "rb").read()), b)
