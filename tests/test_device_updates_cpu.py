"""CPU: mesh updates from device memory and the refit staged on the GPU (pbrlab_amd/csrc/geom_gpu.hip; pbrhip_scene_update_*_mesh_device,
pbrhip_scene_read_slots) -- what can be held without a device: the symbols and names, the NULL-scene refusals, the new kernels' table and
the Python wrappers' argument checks.  tests/test_device_updates_gpu.py holds the feature itself to a fresh commit."""
import numpy as np
import pytest

import _codeobj as CO

EINVAL = -1
KERNELS = ["k_dg_check", "k_dg_init", "k_dg_stage"]
SYMBOLS = ("pbrhip_scene_update_triangle_mesh_device", "pbrhip_scene_update_curve_mesh_device", "pbrhip_scene_read_slots")


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("UpdateTriangleMeshDevice", "UpdateCurveMeshDevice", "read_slots"):
        assert hasattr(pa.Scene, name), name
    assert L.pbrhip_abi_version() == 6


def test_a_null_scene_is_refused():
    from pbrlab_amd import _lib
    L = _lib.lib()
    v = np.zeros((3, 4), np.float32)
    n = np.zeros(1, np.uint32)
    assert L.pbrhip_scene_update_triangle_mesh_device(None, 0, v.ctypes.data, 3, None, 0, None) == EINVAL
    assert b"NULL" in L.pbrhip_last_error()
    assert L.pbrhip_scene_update_curve_mesh_device(None, 0, v.ctypes.data, 3, None) == EINVAL
    assert L.pbrhip_scene_read_slots(None, None, None, n.ctypes.data) == EINVAL and b"NULL" in L.pbrhip_last_error()


def test_every_staging_kernel_is_listed_and_uses_no_scratch():
    assert CO.available(), "libpbrhip.so or the LLVM tools are missing"
    import _codeobj_tus as T
    table = T.kernel_table()
    mine = {k.split("::")[-1].split("(")[0]: v for k, v in table.items() if "k_dg_" in k}
    print({k: (v["vgpr_count"], v["private_segment_fixed_size"], v["group_segment_fixed_size"]) for k, v in mine.items()})
    assert sorted(mine) == KERNELS
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the names other tests pin to complete lists stay out of the new translation unit: its kernels are exactly the ones above
    for k in mine:
        assert not any(p in k for p in ("k_rf_", "k_qc_", "k_features", "k_denoise")), k
    # ... and it is linked behind the render kernels' unit: the library's first code object holds none of them
    assert not any("k_dg_" in k for k in CO.kernel_table())


class _Tensor:
    """what the wrappers look at of a torch tensor"""

    def __init__(self, shape=(8, 4), dtype="torch.float32", contiguous=True, device_type="cuda", index=0):
        self.shape, self.dtype, self._c = shape, dtype, contiguous
        self.device = type("device", (), {"type": device_type, "index": index})()
        self.asked = 0

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        self.asked += 1
        return 0x1000


class _NoCalls:
    """stands in for the library: any C call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


@pytest.fixture()
def scene():
    from pbrlab_amd import api
    s = api.Scene.__new__(api.Scene)                                      # (no device here: a scene object that cannot reach the library)
    s.L, s.h, s.device = _NoCalls(), None, 0
    return s


@pytest.mark.parametrize("bad,exc", [
    (dict(dtype="torch.float64"), TypeError), (dict(contiguous=False), ValueError), (dict(shape=(8, 3)), ValueError), (dict(shape=(32,)), ValueError),
    (dict(device_type="cpu"), ValueError), (dict(index=1), ValueError)])
def test_wrappers_refuse_bad_tensors_before_any_c_call(scene, bad, exc):
    good = _Tensor()
    for call in (lambda t: scene.UpdateTriangleMeshDevice(0, t, stream=0), lambda t: scene.UpdateTriangleMeshDevice(0, good, t, stream=0),
                 lambda t: scene.UpdateCurveMeshDevice(0, t, stream=0)):
        t = _Tensor(**bad)
        with pytest.raises(exc):
            call(t)
        assert t.asked == 0
    with pytest.raises(TypeError):
        scene.UpdateCurveMeshDevice(0, np.zeros((8, 4), np.float32), stream=0)  # host memory is not a device array
    with pytest.raises(TypeError):
        scene.UpdateCurveMeshDevice(0, (1, 2, 3), stream=0)


def test_wrappers_pass_good_arguments_on(scene):
    """a well-formed tensor-like object and a (pointer, count) pair both reach the C call, with the stream as given"""
    seen = []

    class Lib:
        def pbrhip_scene_update_triangle_mesh_device(self, *a):
            seen.append(a)
            return 0
    scene.L = Lib()
    scene.UpdateTriangleMeshDevice(3, _Tensor(shape=(5, 4)), stream=7)
    scene.UpdateTriangleMeshDevice(3, (0x2000, 9), (0x3000, 2))
    (h, mesh, vp, nv, np_, nn, st), second = seen
    assert (mesh, vp.value, nv, np_, nn, st.value) == (3, 0x1000, 5, None, 0, 7)
    assert (second[2].value, second[3], second[4].value, second[5], second[6]) == (0x2000, 9, 0x3000, 2, None)


def test_api_does_not_import_torch_at_load():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "import sys; import pbrlab_amd.api; print('torch' in sys.modules)"], cwd=root, check=True,
                         capture_output=True, text=True).stdout
    assert out.strip() == "False"


def test_shim_has_the_device_calls(tmp_path):
    """include/pbrlab_hip.hpp: the two names compile against the header with the argument types a caller holds"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "shim_device.cc"
    src.write_text('#include "pbrlab_hip.hpp"\n'
                   "void edit(pbrlab::Scene& s, const pbrlab::MeshPtr& tri, const pbrlab::MeshPtr& hair, const void* d, void* stream) {\n"
                   "  s.UpdateTriangleMeshDevice(tri, d, 8u);\n  s.UpdateTriangleMeshDevice(tri, d, 8u, d, 8u, stream);\n"
                   "  s.UpdateCurveMeshDevice(hair, d, 16u);\n  s.UpdateCurveMeshDevice(hair, d, 16u, stream);\n  s.RefitScene();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "include"), str(src)])
