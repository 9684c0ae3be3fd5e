"""GPU (-m gpu): the per-light shaft grid changes no image (pbrlab_amd/csrc/shaft_grid.h, kernels.hip::shaft_unoccluded).

Frames of 64 x 64 x 4 rendered with PBRHIP_SHADOW_GRID=0 (every shadow ray traced) and with the default grid are compared byte for byte,
rgba and count: the reduced Cornell box with the wavefront kernels alone (tail_paths = 0xFFFFFFFF: k_shade_principled, the kernel that
uses the grid) and with the default hand-over to k_tail, a scene with two lights, one with a transformed instance, one with nine lights
(no grid), one with media (its kernels do not use the grid).  After a vertex edit that moves an occluder into shafts that were clear, on
the host and from device memory, the refitted scene's frame equals that of a fresh commit of the edited model.  A statistics render
counts the rays the grid answers (culled_shadow_rays of shadow_grid_info) and traces them all the same, so that shadow_rays +
tail_shadow_rays stays the oracle's count."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _oracle as O  # noqa: E402
from pbrlab_amd import scenes  # noqa: E402

W = H = 64
SPP = 4
NEVER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


class grid_knob:
    """PBRHIP_SHADOW_GRID for the renders inside (the library reads its knobs at every call); None: unset, the default"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("PBRHIP_SHADOW_GRID", None)
        if self.value is not None:
            os.environ["PBRHIP_SHADOW_GRID"] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop("PBRHIP_SHADOW_GRID", None)
        if self.old is not None:
            os.environ["PBRHIP_SHADOW_GRID"] = self.old


def small_cornell(variant="ggx"):
    return scenes.cornell_scene(variant, seed=1, monkey_subdiv=3, lucy_nu=256, lucy_nv=32)


def add_quad(desc, name, corners, material_id, transform=None):
    """one more shape of two triangles (a name that starts with "light" makes it an area light)"""
    first = len(desc.vertices)
    v = np.concatenate([np.asarray(corners, np.float32).reshape(4, 3), np.ones((4, 1), np.float32)], 1)
    desc.vertices = np.concatenate([desc.vertices, v])
    ids = (np.array([[0, 1, 2], [0, 2, 3]], np.uint32) + np.uint32(first)).astype(np.uint32)
    desc.shapes.append(scenes.Shape(name, ids, None, np.full(2, material_id, np.uint32), transform=transform))
    return desc


def frame(pa, sg, tail_paths, grid):
    lay = pa.RenderLayer()
    with grid_knob(grid):
        ok, _ = pa.Render(sg, W, H, SPP, layer=lay, tail_paths=tail_paths)
    assert ok is True and (lay.count == SPP).all()
    return lay.rgba.tobytes(), lay.count.tobytes()


def counted(pa, sg, tail_paths):
    """a statistics render under the default grid -> (its statistics, the grid's report)"""
    lay = pa.RenderLayer()
    with grid_knob(None):
        ok, st = pa.Render(sg, W, H, SPP, layer=lay, tail_paths=tail_paths, flags=pa.api.RENDER_STATS)
        gi = sg.shadow_grid_info()
    assert ok is True
    return st, gi, (lay.rgba.tobytes(), lay.count.tobytes())


def two_lights():
    return add_quad(small_cornell(), "light2", [(-0.99, -0.2, -0.3), (-0.99, -0.2, 0.3), (-0.99, 0.4, 0.3), (-0.99, 0.4, -0.3)], 1)


def transformed():
    # a screen that its instance transform lifts from below the floor into the room: some floor shafts are clear only without it
    return add_quad(small_cornell(), "screen", [(-0.2, -3.0, -0.6), (0.5, -3.0, -0.6), (0.5, -3.0, -0.1), (-0.2, -3.0, -0.1)], 7,
                    transform=scenes.instance_matrix(rotate_deg=(0.0, 20.0, 0.0), translate=(0.0, 3.2, 0.0)))


def nine_lights():
    d = small_cornell()
    for i in range(8):
        x = -0.9 + 0.22 * i
        add_quad(d, f"light{i + 2}", [(x, 0.99, -0.9), (x + 0.1, 0.99, -0.9), (x + 0.1, 0.99, -0.8), (x, 0.99, -0.8)], 1)
    return d


@pytest.mark.parametrize("name,make,tail,has_grid,culls", [
    ("cornell_wavefront", small_cornell, NEVER, True, True),
    ("cornell_default_tail", small_cornell, 0, True, None),
    ("two_lights", two_lights, NEVER, True, True),
    ("transformed_instance", transformed, NEVER, True, True),
    ("nine_lights", nine_lights, NEVER, False, False),
    ("media", lambda: small_cornell("sss"), NEVER, True, False),
])
def test_frames_do_not_depend_on_the_grid(pa, name, make, tail, has_grid, culls):
    desc = make()
    sg = pa.scene_from_desc(desc)
    off, on = frame(pa, sg, tail, 0), frame(pa, sg, tail, None)
    assert off == on, name
    st, gi, stats_frame = counted(pa, sg, tail)
    assert stats_frame == off
    print(name, {k: gi[k] for k in ("resolution", "num_lights", "bytes", "clear_cells", "unknown_cells", "culled_shadow_rays", "clear_cell_rays", "leaf_tests")},
          "shadow rays", st["shadow_rays"], "+", st["tail_shadow_rays"])
    assert (gi["resolution"] > 0) == has_grid
    if has_grid:
        assert gi["num_lights"] == sum(s.name[:5] == "light" for s in desc.shapes) and gi["bytes"] == gi["num_lights"] * gi["resolution"] ** 3 * 32
        assert gi["clear_cells"] > 0 and gi["clear_cells"] + gi["unknown_cells"] == gi["num_lights"] * gi["resolution"] ** 3
        assert sg.info()["device_bytes"] >= gi["bytes"]
    else:
        assert gi["bytes"] == 0
    if culls is True:
        assert 0 < gi["culled_shadow_rays"] <= gi["clear_cell_rays"] <= st["shadow_rays"]
    if culls is False:
        assert gi["culled_shadow_rays"] == 0
    # the rays the grid answers are still the integrator's shadow rays
    ost = O.oracle_scene_from_desc(desc).render(W, H, SPP, threads=O.oracle_threads(), math_mode=O.MATH_DEVICE)[2]
    assert st["shadow_rays"] + st["tail_shadow_rays"] == ost["shadow_rays"]


def test_culled_rays_on_the_cornell_box(pa):
    sg = pa.scene_from_desc(small_cornell())
    st, gi, _ = counted(pa, sg, NEVER)
    assert 0 < gi["culled_shadow_rays"] <= st["shadow_rays"]
    with grid_knob(0):
        assert sg.shadow_grid_info()["resolution"] == 0 and sg.shadow_grid_info()["bytes"] == 0
    with grid_knob(16):
        cells = sg.read_shadow_grid()
    assert cells.shape == (1, 16, 16, 16, 8)
    counts = cells[..., 0]
    assert ((counts <= 7) | (counts == 0xFFFFFFFF)).all() and (counts <= 7).any() and (counts == 0xFFFFFFFF).any()


def _lifted_box(desc):
    """the small box moved up under the light: it now shadows floor cells whose shafts were clear"""
    box = [i for i, s in enumerate(desc.shapes) if s.name == "box"][0]
    ids = np.unique(desc.shapes[box].vertex_ids)
    v = desc.vertices.copy()
    v[ids, 1] += 1.2
    v[ids, 0] -= 0.05
    v[ids, 2] -= 0.55
    return box, v


@pytest.mark.parametrize("device_update", [False, True])
def test_refit_after_an_occluder_moves_into_clear_shafts(pa, device_update):
    desc = small_cornell()
    sg = pa.scene_from_desc(desc)
    before = frame(pa, sg, NEVER, None)
    box, v = _lifted_box(desc)
    if device_update:
        import torch
        sg.UpdateTriangleMeshDevice(box, torch.from_numpy(v).to("cuda:0"))
    else:
        sg.UpdateTriangleMesh(box, v)
    sg.RefitScene()
    refitted = frame(pa, sg, NEVER, None)
    desc.vertices = v
    fresh = pa.scene_from_desc(desc)
    assert refitted == frame(pa, fresh, NEVER, 0) == frame(pa, fresh, NEVER, None)
    assert refitted != before
