"""Rendering along caller-supplied rays and the three projections without a GPU: the symbols and names exist and refuse
bad arguments before any device work, the new kernels keep their budgets and stay out of the render kernels' code object, the C++ shim
caller compiles, and the float64 projection model of tests/_projection_model.py keeps its own invariants."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _codeobj as CO
import _projection_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shim_rays")
SYMBOLS = ("pbrhip_render_rays", "pbrhip_render_rays_device", "pbrhip_render_features_rays_device", "pbrhip_projection_rays_device")
EINVAL, ENODEVICE = -1, -3
RAY_KERNELS = ("k_generate_rays", "k_project_rays", "k_features_rays<true, false>", "k_features_rays<true, true>", "k_features_rays<false, true>")


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert L.pbrhip_abi_version() == 6 and "#define PBRHIP_ABI_VERSION 6u" in hdr
    for name in ("RenderRays", "RenderFeaturesRays", "RenderProjection"):
        assert hasattr(pa, name) and hasattr(api, name), name
    assert hasattr(api.Scene, "ProjectionRays")
    enum = dict(re.findall(r"PBRHIP_PROJECTION_(\w+) = (\d)", hdr))
    assert (int(enum["LATLONG"]), int(enum["FISHEYE"]), int(enum["ORTHO"])) == (api.PROJECTION_LATLONG, api.PROJECTION_FISHEYE, api.PROJECTION_ORTHO) \
        == (PM.LATLONG, PM.FISHEYE, PM.ORTHO)
    shim = open(os.path.join(ROOT, "include", "pbrlab_hip.hpp")).read()
    for name in ("RenderRays", "RenderFeaturesRays", "ProjectionRays", "RenderProjection"):
        assert re.search(r"\b" + name + r"\(const Scene&", shim), name
    assert api.RAY_BUFFER_BYTES == 256 << 20 and "kRayBufferBytes = size_t(256) << 20" in shim


def test_null_and_bad_arguments_are_refused_before_any_device_work():
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    desc = api._desc(8, 4, 4)
    rays = np.zeros((4, 4, 8), api.RAY_DT)
    rgba, count = np.zeros((4, 8, 4), np.float32), np.zeros((4, 8), np.uint32)
    out = (rgba.ctypes.data, count.ctypes.data, None, None)
    fake = C.c_void_p(16)  # never dereferenced: the checks below come before the scene is touched

    def refused(rc, word):
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())

    # a NULL scene, NULL rays, a NULL layer
    refused(L.pbrhip_render_rays(None, C.byref(desc), rays.ctypes.data, 4, 2, None, *out), b"NULL")
    refused(L.pbrhip_render_rays_device(None, C.byref(desc), rays.ctypes.data, 4, 2, None, None, *out), b"NULL")
    refused(L.pbrhip_render_rays(fake, C.byref(desc), None, 4, 2, None, *out), b"NULL")
    refused(L.pbrhip_render_rays_device(fake, C.byref(desc), None, 4, 2, None, None, *out), b"NULL")
    refused(L.pbrhip_render_rays(fake, None, rays.ctypes.data, 4, 2, None, *out), b"NULL")
    refused(L.pbrhip_render_rays(fake, C.byref(desc), rays.ctypes.data, 4, 2, None, None, count.ctypes.data, None, None), b"NULL")
    refused(L.pbrhip_render_features_rays_device(None, C.byref(desc), rays.ctypes.data, 4, None, None, None, None), b"NULL")
    refused(L.pbrhip_render_features_rays_device(fake, C.byref(desc), None, 4, None, None, None, None), b"NULL")
    refused(L.pbrhip_projection_rays_device(None, 0, 0.0, 8, 4, 0, 1, 1, rays.ctypes.data, None), b"NULL")
    refused(L.pbrhip_projection_rays_device(fake, 0, 0.0, 8, 4, 0, 1, 1, None, None), b"NULL")
    # the shape of the ray buffer and the draws: neither 1 nor num_sample planes, more than 16 draws
    for planes in (0, 2, 3, 5):
        refused(L.pbrhip_render_rays(fake, C.byref(desc), rays.ctypes.data, planes, 2, None, *out), b"ray_passes")
        refused(L.pbrhip_render_rays_device(fake, C.byref(desc), rays.ctypes.data, planes, 2, None, None, *out), b"ray_passes")
        refused(L.pbrhip_render_features_rays_device(fake, C.byref(desc), rays.ctypes.data, planes, None, None, None, None), b"ray_passes")
    refused(L.pbrhip_render_rays(fake, C.byref(desc), rays.ctypes.data, 4, 17, None, *out), b"camera_draws")
    refused(L.pbrhip_render_rays_device(fake, C.byref(desc), rays.ctypes.data, 1, 17, None, None, *out), b"camera_draws")
    # the projection's own arguments
    for args in ((3, 0.0, 8, 4, 0, 1), (0, 0.0, 0, 4, 0, 1), (1, 361.0, 8, 4, 0, 1), (1, -1.0, 8, 4, 0, 1), (2, 0.0, 8, 4, 0, 1),
                 (2, float("nan"), 8, 4, 0, 1), (0, 0.0, 8, 4, 0xFFFFFFFF, 2)):
        assert L.pbrhip_projection_rays_device(fake, *args, 1, rays.ctypes.data, None) == EINVAL, args


def test_python_refuses_bad_rays_before_any_c_call():
    from pbrlab_amd import api
    ok = np.zeros((4, 6, 8, 8), np.float32)

    class Tensor:  # what _ray_source reads of a torch tensor
        def __init__(self, shape=(4, 6, 8, 8), dtype="torch.float32", dev="cuda", index=0, contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous
            self.device = type("D", (), dict(type=dev, index=index))()

        def data_ptr(self):
            return 4096

        def is_contiguous(self):
            return self._c

    scene = type("S", (), dict(device=0, h=None))()
    for bad, err in ((ok.astype(np.float64), TypeError), (ok[..., :7], ValueError), (ok[0, 0], ValueError), (np.zeros((2, 6, 8), api.RAY_DT), ValueError),
                     (np.zeros((4, 6, 8, 8), np.int32), TypeError), ("rays", TypeError), ((4096, 6, 8), TypeError), ((0, (4, 6, 8)), ValueError),
                     ((4096, (3, 6, 8)), ValueError), ((4096, (6,)), ValueError), (Tensor(dtype="torch.float16"), TypeError),
                     (Tensor(shape=(4, 6, 8, 7)), ValueError), (Tensor(dev="cpu"), ValueError), (Tensor(index=1), ValueError),
                     (Tensor(contiguous=False), ValueError), (Tensor(shape=(3, 6, 8, 8)), ValueError), (np.zeros((4, 0, 8), api.RAY_DT), ValueError)):
        for fn in (api.RenderRays, api.RenderFeaturesRays):
            with pytest.raises(err):
                fn(scene, bad, 4)
    with pytest.raises(ValueError):
        api.RenderRays(scene, ok, 4, camera_draws=17)
    with pytest.raises(ValueError):
        api.RenderRays(scene, ok, 4, device_out=(1, 2))  # host rays cannot go into device buffers
    # what passes: the grid comes from the shape
    assert api._ray_source(ok, scene, 4)[2] == (4, 6, 8) and api._ray_source(ok[0], scene, 4)[2] == (1, 6, 8)
    assert api._ray_source(np.zeros((6, 8), api.RAY_DT), scene, 9)[2] == (1, 6, 8)
    assert api._ray_source(Tensor(), scene, 4)[:3] == ("device", 4096, (4, 6, 8)) and api._ray_source((4096, (6, 8)), scene, 4)[2] == (1, 6, 8)
    with pytest.raises(ValueError):
        api.Scene.ProjectionRays(scene, "cylinder", 8, 4, 0, 1)
    # a NULL scene reaches the library, which says so
    for fn in (api.RenderRays, api.RenderFeaturesRays):
        with pytest.raises(api.PbrHipError) as e:
            fn(None, ok, 4)
        assert e.value.code == EINVAL and "NULL" in str(e.value)


def test_fails_loudly_without_device():
    import pbrlab_amd as pa
    if pa.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderProjection(pa.Scene(), "latlong", 8, 4, 2)
    assert e.value.code == ENODEVICE
    with pytest.raises(pa.PbrHipError):
        pa.api.DeviceRays((1, 4, 8), 0)  # no device memory without a device, and no host stand-in for it


def test_ray_kernels_stay_within_their_budgets():
    if not CO.available():
        pytest.skip("libpbrhip.so or the LLVM tools are missing")
    import _codeobj_tus as T
    table = T.kernel_table()
    assert sorted(k for k in table if "_rays" in k and "k_camera_rays" not in k) == sorted(RAY_KERNELS)
    for name in ("k_generate_rays", "k_project_rays"):  # streaming kernels of k_generate_camera's class
        got = table[name]
        assert got["private_segment_fixed_size"] == 0 and got["group_segment_fixed_size"] == 0, (name, got)
        assert got["vgpr_count"] <= 64 and CO.waves_per_simd(got["vgpr_count"]) >= 8, (name, got)
    for name in RAY_KERNELS[2:]:  # k_features' class: the LDS part of the traversal stack, four blocks per CU
        got = table[name]
        assert got["private_segment_fixed_size"] == 0 and got["group_segment_fixed_size"] == 40 * 256 * 4 and got["vgpr_count"] <= 128, (name, got)
    # the render kernels' translation unit is still the library's first code object, without any of these
    first = CO.kernel_table()
    assert not any(k in first for k in RAY_KERNELS) and all(k in table for k in first)
    assert any(k.startswith("k_trace") for k in first) and all(k in first for k in ("k_accumulate", "k_generate", "k_generate_camera", "k_camera_rays"))
    assert sum("k_features<" in k for k in table) == 3


def test_rays_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_rays.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3, r.stderr


def test_cli_rejects_bad_projection_flags():
    cli = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
    if not os.path.exists(cli):
        pytest.skip("pbrlab-hip-cli not built")
    cam = ["--eye", "0,0,1", "--lookat", "0,0,0"]
    for args, msg in ((["--projection"], "missing value for --projection"), (["--projection", "cube"], "--projection needs latlong, fisheye or ortho"),
                      (["--projection", "latlong"], "--projection needs --eye and --lookat"),
                      (cam + ["--projection", "ortho"], "--projection ortho needs --ortho-height"),
                      (cam + ["--projection", "fisheye", "--ortho-height", "2"], "--ortho-height needs --projection ortho"),
                      (cam + ["--projection", "ortho", "--ortho-height", "0"], "--ortho-height needs a finite number > 0"),
                      (cam + ["--projection", "fisheye", "--fov", "400"], "--projection fisheye needs --fov in (0, 360]"),
                      (cam + ["--projection", "latlong", "--gpus", "2"], "--projection renders on one GPU"),
                      (cam + ["--projection", "latlong", "--denoise"], "--projection renders on one GPU")):
        r = subprocess.run([cli, "scene.obj"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.returncode, r.stderr)


# ---------------------------------------------------------------------------------------------------- the projection model
CAM = PM.frame((1.2, -1.6, 1.4), (0.0, 0.0, 0.1), (0.0, 0.0, 1.0))


def test_model_frame_and_jitter():
    eye, r, u, f = CAM
    for a in (r, u, f):
        assert abs(np.linalg.norm(a) - 1) < 1e-15
    assert abs(r @ u) < 1e-15 and abs(r @ f) < 1e-15 and abs(u @ f) < 1e-15 and np.allclose(np.cross(r, u), -f)  # r, u, -f right-handed
    assert u[2] > 0  # up is up
    # PCG32's published first output for state 42, sequence 54 (the generator every sample owns)
    inc = (54 << 1) | 1
    state, _ = PM._pcg32(0, inc)
    state, _ = PM._pcg32((state + 42) & PM.MASK, inc)
    assert PM._pcg32(state, inc)[1] == 0xA15C02B7
    jx, jy = PM.jitters(5, 3, 17)
    assert jx.shape == (3, 5) and (jx >= 0).all() and (jx < 1).all() and (jy >= 0).all() and (jy < 1).all()
    assert len(np.unique(np.concatenate([jx.ravel(), jy.ravel()]))) == 30 and not np.array_equal(jx, PM.jitters(5, 3, 18)[0])


@pytest.mark.parametrize("size", [(64, 32), (37, 91)])
def test_model_invariants(size):
    W, H = size
    eye, r, u, f = CAM
    half = np.full((H, W), 0.5)
    for proj, param in ((PM.LATLONG, 0.0), (PM.FISHEYE, 180.0), (PM.FISHEYE, 360.0), (PM.ORTHO, 2.5)):
        org, d, active, rho = PM.rays(proj, CAM, W, H, *PM.jitters(W, H, 0), param=param)
        assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-14, proj
        assert active.all() == (proj != PM.FISHEYE)
    # lat-long: the image centre looks along f, the top row along u, the left and right edges along -f
    zero = np.zeros((H, W))
    _, d, _, _ = PM.rays(PM.LATLONG, CAM, W, H, zero + (W / 2 - W // 2), zero + (H / 2 - H // 2))
    assert np.abs(d[H // 2, W // 2] - f).max() < 1e-14
    _, d, _, _ = PM.rays(PM.LATLONG, CAM, W, H, zero, zero)
    assert np.abs(d[0] - u).max() < 1e-14 and np.abs(d[H // 2 if H % 2 == 0 else 0, 0] - (-f if H % 2 == 0 else u)).max() < 1e-14
    # ... and a quarter turn to the right of the centre along r
    if W % 4 == 0 and H % 2 == 0:
        assert np.abs(d[H // 2, 3 * W // 4] - r).max() < 1e-14
    # fisheye of 180 degrees: rho = 1 (the top of the image circle: sx = 0, sy = 1) is perpendicular to f; the centre is f
    _, d, active, rho = PM.rays(PM.FISHEYE, CAM, W, H, zero + (W / 2 - W // 2), zero, param=180.0)
    assert rho[0, W // 2] == 1.0 and active[0, W // 2] and abs(d[0, W // 2] @ f) < 1e-15 and np.abs(d[0, W // 2] - u).max() < 1e-15
    _, d, _, rho = PM.rays(PM.FISHEYE, CAM, W, H, zero + (W / 2 - W // 2), zero + (H / 2 - H // 2), param=180.0)
    assert rho[H // 2, W // 2] == 0 and np.array_equal(d[H // 2, W // 2], f)
    # ... the corners of the frame lie outside the image circle, whatever the aspect
    _, _, active, _ = PM.rays(PM.FISHEYE, CAM, W, H, half, half, param=180.0)
    assert not active[0, 0] and not active[-1, -1] and not active[0, -1] and not active[-1, 0] and active[H // 2, W // 2]
    # ... param 0 means the camera's field of view
    assert np.array_equal(PM.rays(PM.FISHEYE, CAM, W, H, half, half, param=0.0, fov=70.0)[1], PM.rays(PM.FISHEYE, CAM, W, H, half, half, param=70.0)[1])
    # ortho: the origins span +-half vertically and +-half x aspect horizontally, every direction is f
    org, d, _, _ = PM.rays(PM.ORTHO, CAM, W, H, zero, zero, param=2.5)
    assert (d == f).all()
    assert np.abs(org[0, 0] - (eye - 2.5 * W / H * r + 2.5 * u)).max() < 1e-14
    org1, _, _, _ = PM.rays(PM.ORTHO, CAM, W, H, zero + 1, zero + 1, param=2.5)
    assert np.abs(org1[-1, -1] - (eye + 2.5 * W / H * r - 2.5 * u)).max() < 1e-14
    assert np.abs((org - eye) @ f).max() < 1e-14
