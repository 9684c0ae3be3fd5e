"""tests/cpp/shim_knearest.cc: pbrlab::Scene::KNearest and KNearestDevice through the C++ shim (include/pbrlab_hip.hpp).  Without a device
the caller compiles, links and fails loudly, like shim_allhits; on the GPU its answers, printed as words, equal the Python binding's on
the same scene and points."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shim_knearest")
F = np.float32
INF = np.inf
POINTS = [(0.25, 0.5, 1.0, INF), (0.25, 0.5, 1.0, 1.5), (3.0, 0.5, 1.0, 3.5), (0.25, np.nan, 1.0, INF), (0.0, 0.0, -5.0, 1.0), (3.0, 0.5, -2.0, 0.0)]
K = 2


def test_knearest_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_knearest.cc"),
                           "-L" + lib, "-lpbrhip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3 and "shim:" in r.stderr, (r.returncode, r.stderr)


def _python_lines():
    """the shim's scene and points through the Python binding, formatted as the shim prints them"""
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    quad = lambda r, z: [[-r, -r, z, 1], [r, -r, z, 1], [r, r, z, 1], [-r, r, z, 1]]
    verts = np.array(quad(1.0, 0.0) + quad(8.0, -2.0), F)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="grey", base_color=(0.25, 0.25, 0.25))
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    desc = scenes.SceneDesc(verts, np.zeros((0, 4), F), [mat], [scenes.Shape("quad", faces, None, np.zeros(2, np.uint32)),
                                                                scenes.Shape("wall", faces + 4, None, np.zeros(2, np.uint32)),
                                                                scenes.Shape("wall", faces + 4, None, np.zeros(2, np.uint32))])
    s = pa.scene_from_desc(desc)
    pts = np.array(POINTS, F)
    count, ident, closest = s.KNearestDevice(torch.from_numpy(pts.copy()).to("cuda:0"), K, closest=True)
    count, ident, closest = count.cpu().numpy().view(np.uint32), ident.cpu().numpy().view(np.uint32), closest.cpu().numpy().view(np.uint32)
    hcount, hident, hclosest = s.KNearest(pts, K)
    assert np.array_equal(hcount, count) and np.array_equal(hident, ident) and np.array_equal(hclosest.view(np.uint32), closest)
    assert count.tolist() == [6, 2, 6, 0, 0, 2]
    word = lambda a: " ".join(f"{int(x):08x}" for x in a)
    return [f"K {i} {int(count[i]):08x} | {word(ident[i].reshape(-1))} | {word(closest[i].reshape(-1))}" for i in range(len(pts))]


@pytest.mark.gpu
def test_knearest_shim_caller_runs_and_matches_python():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    test_knearest_shim_caller_compiles()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    got = [ln for ln in r.stdout.splitlines() if ln[:2] == "K "]
    assert got == _python_lines()
