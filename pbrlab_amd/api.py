"""Host-side mirror of pbrlab's drop-in boundary over the C ABI of libpbrhip.so (include/pbrhip.h).

`Scene` keeps the builder method names of `pbrlab::Scene` (src/scene.h:19-91), `RenderLayer` the
fields of `pbrlab::RenderLayer` (src/render-layer.h:11-26) and `Render` the argument list of
`pbrlab::Render` (src/render.h:14-17).  Python is only the binding layer here: all work happens in
the HIP library; nothing in this module computes pixels and nothing falls back to the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib

NONE = 0xFFFFFFFF
fp = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)

RENDER_STATS, RENDER_TIMING, RENDER_NO_CLEAR, RENDER_TIMING_TRACE = 1, 2, 4, 8


class PrincipledParam(C.Structure):
    """pbrhip_principled_param == CyclesPrincipledBsdfParameter (src/material-param.h:24-49)."""
    _fields_ = [("base_color", C.c_float * 3), ("subsurface", C.c_float),
                ("subsurface_radius", C.c_float * 3), ("subsurface_color", C.c_float * 3),
                ("metallic", C.c_float), ("specular", C.c_float), ("specular_tint", C.c_float),
                ("roughness", C.c_float), ("anisotropic", C.c_float), ("anisotropic_rotation", C.c_float),
                ("sheen", C.c_float), ("sheen_tint", C.c_float), ("clearcoat", C.c_float),
                ("clearcoat_roughness", C.c_float), ("ior", C.c_float), ("transmission", C.c_float),
                ("transmission_roughness", C.c_float), ("base_color_tex_id", C.c_uint32),
                ("subsurface_color_tex_id", C.c_uint32)]


class HairParam(C.Structure):
    """pbrhip_hair_param == HairBsdfParameter (src/material-param.h:51-72)."""
    _fields_ = [("coloring_hair", C.c_uint32), ("base_color", C.c_float * 3), ("melanin", C.c_float),
                ("melanin_redness", C.c_float), ("melanin_randomize", C.c_float), ("roughness", C.c_float),
                ("azimuthal_roughness", C.c_float), ("ior", C.c_float), ("shift", C.c_float),
                ("specular_tint", C.c_float * 3), ("second_specular_tint", C.c_float * 3),
                ("transmission_tint", C.c_float * 3)]


class RenderDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("num_sample", C.c_uint32),
                ("first_pass", C.c_uint32), ("seed_seq", C.c_uint64), ("tile_rank", C.c_uint32),
                ("tile_world", C.c_uint32), ("max_paths_in_flight", C.c_uint32), ("flags", C.c_uint32),
                ("num_streams", C.c_uint32), ("tail_paths", C.c_uint32), ("shard_block", C.c_uint32)]


BVH_HOST_SAH, BVH_GPU_LBVH, BVH_GPU_LBVH_WIDE = 0, 1, 2


class ShadowGridInfo(C.Structure):  # pbrhip_shadow_grid_info
    _fields_ = ([(n, C.c_uint32) for n in ("resolution", "num_lights", "max_list", "pad")] +
                [(n, C.c_uint64) for n in ("bytes", "clear_cells", "unknown_cells", "empty_cells", "listed_leaves", "culled_shadow_rays",
                                           "clear_cell_rays", "leaf_tests")] + [("build_ms", C.c_double)])


class RenderStats(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("samples", "iterations", "chunks", "closest_rays", "closest_nodes",
                                           "closest_tris", "closest_curves", "shadow_rays", "shadow_nodes",
                                           "shadow_tris", "shadow_curves")] +
                [(n, C.c_double) for n in ("ms_generate", "ms_trace_closest", "ms_surface", "ms_shade_principled",
                                           "ms_shade_hair", "ms_sss_step", "ms_tail", "ms_accumulate", "ms_compact")] +
                [(n, C.c_uint64) for n in ("n_trace_closest", "n_tail", "n_surface", "n_shade_principled",
                                           "n_shade_hair", "n_sss_step")] + [("ms_total", C.c_double)] +
                [(n, C.c_uint64) for n in ("tail_closest_rays", "tail_shadow_rays", "pruned_rays", "passes_done", "node_bytes", "curve_bytes", "suspended_rays")] +
                [("ms_host_idle", C.c_double)])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SdInfo(C.Structure):  # pbrhip_sd_info
    _fields_ = ([(n, C.c_uint32) for n in ("triangles", "vertices", "edges_manifold", "edges_boundary", "edges_nonmanifold", "edges_inconsistent")] +
                [("table_bytes", C.c_uint64), ("topology_ms", C.c_double), ("table_ms", C.c_double)])


RAY_DT = np.dtype([("org", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT_DT = np.dtype([("normal_g", "<f4", 3), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"),
                   ("instance_id", "<u4"), ("geom_id", "<u4"), ("prim_id", "<u4")])
POINT_DT = np.dtype([("p", "<f4", 3), ("max_dist", "<f4")])  # pbrhip_point: a nearest-point query (max_dist inf: no bound)


class PbrHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pbrhip error {code}: {msg}")
        self.code = code


def _chk(rc):
    if rc != 0:
        msg = _lib.lib().pbrhip_last_error()
        raise PbrHipError(rc, msg.decode() if msg else "")


def _ptr(a, t=fp):
    return None if a is None else a.ctypes.data_as(t)


def _device_array(a, scene):
    """An argument of the *Device update calls -> (pointer, count): None, a (pointer, count) pair, or an object with data_ptr() as a
    torch tensor has -- float32, contiguous, (n, 4), on the scene's device, else TypeError / ValueError here, before any C call."""
    if a is None:
        return None, 0
    if isinstance(a, (tuple, list)):
        if len(a) != 2:
            raise TypeError("a device array is a tensor or a (pointer, count) pair")
        return C.c_void_p(None if a[0] is None else int(a[0])), int(a[1])
    if not hasattr(a, "data_ptr"):
        raise TypeError(f"{type(a).__name__} is no device array: pass a tensor on the scene's device (data_ptr()) or a (pointer, count) pair")
    if not str(getattr(a, "dtype", "")).endswith("float32"):
        raise TypeError(f"a device array must be float32, not {getattr(a, 'dtype', None)}")
    shape = tuple(getattr(a, "shape", ()))
    if len(shape) != 2 or shape[1] != 4:
        raise ValueError(f"a device array must have the shape (n, 4), not {shape}")
    if not a.is_contiguous():
        raise ValueError("a device array must be contiguous")
    dev = getattr(a, "device", None)
    if getattr(dev, "type", None) != "cuda":
        raise ValueError(f"a device array must be in GPU memory, not on {dev}")
    want = getattr(scene, "device", None)
    if want is not None and dev.index is not None and dev.index != want:
        raise ValueError(f"the array is on device {dev.index}, the scene on device {want}")
    return C.c_void_p(int(a.data_ptr())), int(shape[0])


def _query_array(a, scene, words, what):
    """The input of a *Device query -> (pointer, n): a (pointer, n) pair, or a float32, contiguous (n, words) tensor on the scene's
    device.  TypeError / ValueError here, before any C call."""
    if isinstance(a, (tuple, list)):
        if len(a) != 2:
            raise TypeError(f"{what}: a tensor or a (pointer, n) pair")
        return C.c_void_p(None if a[0] is None else int(a[0])), int(a[1])
    if not hasattr(a, "data_ptr"):
        raise TypeError(f"{what}: {type(a).__name__} is no device array: pass a tensor on the scene's device or a (pointer, n) pair")
    shape = tuple(getattr(a, "shape", ()))
    n = int(shape[0]) if shape else 0
    return C.c_void_p(_image_arg(a, (n, words), "float32", what, getattr(scene, "device", None))[0]), n


def _query_out(a, scene, shape, dtype, what):
    """An output of a *Device query -> pointer: None (not wanted), a device pointer (an int), or a contiguous tensor of that shape and
    dtype on the scene's device"""
    if a is None or isinstance(a, int):
        return C.c_void_p(a or None)
    if not hasattr(a, "data_ptr"):
        raise TypeError(f"{what}: {type(a).__name__} is no device array: pass a tensor on the scene's device or a device pointer")
    return C.c_void_p(_image_arg(a, shape, dtype, what, getattr(scene, "device", None))[0])


ALL_HITS_MAX = 32  # PBRHIP_ALL_HITS_MAX


def _all_hits_k(max_hits):
    """max_hits of an all-hits query as an int in [0, ALL_HITS_MAX]; ValueError here, before any C call"""
    if isinstance(max_hits, bool) or int(max_hits) != max_hits or not 0 <= int(max_hits) <= ALL_HITS_MAX:
        raise ValueError(f"max_hits must be an integer in [0, {ALL_HITS_MAX}], not {max_hits!r}")
    return int(max_hits)


K_NEAREST_MAX = 32  # PBRHIP_K_NEAREST_MAX


def _k_nearest_k(max_k):
    """max_k of a k-nearest query as an int in [0, K_NEAREST_MAX]; ValueError here, before any C call"""
    if isinstance(max_k, bool) or int(max_k) != max_k or not 0 <= int(max_k) <= K_NEAREST_MAX:
        raise ValueError(f"max_k must be an integer in [0, {K_NEAREST_MAX}], not {max_k!r}")
    return int(max_k)


def _device_stream(stream, *arrays):
    """The hipStream_t of a *Device update call: as given (an integer, or an object with cuda_stream); None: torch's current stream when
    an argument is a tensor (torch is then the caller's: this module does not import it otherwise), else the null stream."""
    if stream is None:
        if any(type(a).__module__.partition(".")[0] == "torch" for a in arrays):
            import torch
            stream = torch.cuda.current_stream()
        else:
            return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


def _fill(struct, d):
    for k, _ in struct._fields_:
        v = d[k]
        if isinstance(v, (tuple, list, np.ndarray)):
            setattr(struct, k, (C.c_float * 3)(*[float(x) for x in v]))
        else:
            setattr(struct, k, v)
    return struct


def make_principled(d):
    return _fill(PrincipledParam(), d)


def make_hair(d):
    return _fill(HairParam(), d)


LEAF_RNG, LEAF_FASTMATH, LEAF_FRESNEL, LEAF_MIS, LEAF_LAMBERT, LEAF_SPHERE, LEAF_TRIANGLE, LEAF_GGX_EVAL, LEAF_GGX_SAMPLE, LEAF_HAIR_EVAL, LEAF_HAIR_SAMPLE = range(11)
LEAF_SSS_MEDIUM, LEAF_SSS_DISTANCE, LEAF_SSS_SCATTER = 11, 12, 13


def leaf_eval(op, inputs, out_words):
    """pbrhip_leaf_eval (include/pbrhip.h): the device's leaf functions on an (n, in_words) array of float32 inputs (integers as their
    bits) -> (n, out_words) float32.  A test hook."""
    a = np.ascontiguousarray(inputs, np.float32)
    if a.ndim != 2:
        raise ValueError("inputs: (n, in_words)")
    out = np.zeros((a.shape[0], out_words), np.float32)
    _chk(_lib.lib().pbrhip_leaf_eval(C.c_uint32(op), C.c_void_p(a.ctypes.data), C.c_size_t(a.shape[0]), C.c_uint32(a.shape[1]),
                                     C.c_void_p(out.ctypes.data), C.c_uint32(out_words)))
    return out


# BvhNode (csrc/dscene.h): both children's boxes interleaved [axis][child], two child references
BVHNODE_DT = np.dtype([("lo", "<f4", (3, 2)), ("hi", "<f4", (3, 2)), ("c0", "<u4"), ("c1", "<u4"), ("pad", "<u4", 2)])


def lbvh_build(lo, hi, kinds, device=None):
    """pbrhip_lbvh_build (include/pbrhip.h): the GPU builder on (n, 3) float32 boxes lo / hi of kinds (n,) uint8 -> (nodes, order, depth):
    max(n - 1, 1) BVHNODE_DT nodes, the primitive of every leaf slot, the stack depth the tree needs -- whatever that is.  A test hook."""
    lo, hi = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (lo, hi))
    kinds = np.ascontiguousarray(kinds, np.uint8).reshape(-1)
    n = len(kinds)
    if len(lo) != n or len(hi) != n:
        raise ValueError("lo, hi and kinds differ in length")
    nodes = np.zeros(max(n - 1, 1) if n else 0, BVHNODE_DT)
    order = np.zeros(n, np.uint32)
    depth = C.c_uint32(0)
    _chk(_lib.lib().pbrhip_lbvh_build(_device if device is None else int(device), lo.ctypes.data, hi.ctypes.data, kinds.ctypes.data, n,
                                      nodes.ctypes.data, order.ctypes.data, C.addressof(depth)))
    return nodes, order, depth.value


# QNode (csrc/dscene.h): per axis an origin and a step, 8-bit bounds of four children (byte i of a word = child i), four references
QNODE_DT = np.dtype([("org", "<f4", 3), ("sx", "<f4"), ("sy", "<f4"), ("sz", "<f4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("c", "<u4", 4)])


def qtree_collapse(lo, hi, kinds, slots, device=None):
    """pbrhip_qtree_collapse (include/pbrhip.h): builder BVH_GPU_LBVH_WIDE on bare boxes and per-primitive slot records (n, 4, 4) float32
    -> dict(nodes, order, depth, qnodes (QNODE_DT), tri (words, 4), pts (points, 4), hit (points,) uint32, stack_need, fits, quantised).
    No fallback: whatever the collapse made.  A test hook."""
    lo, hi = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (lo, hi))
    kinds = np.ascontiguousarray(kinds, np.uint8).reshape(-1)
    slots = np.ascontiguousarray(slots, np.float32).reshape(-1, 4, 4)
    n = len(kinds)
    if len(lo) != n or len(hi) != n or len(slots) != n:
        raise ValueError("lo, hi, kinds and slots differ in length")
    dev = _device if device is None else int(device)
    sizes = np.zeros(6, np.uint32)
    head = (dev, lo.ctypes.data, hi.ctypes.data, kinds.ctypes.data, slots.ctypes.data, n)
    _chk(_lib.lib().pbrhip_qtree_collapse(*head, None, None, None, None, None, None, sizes.ctypes.data))
    nodes, order = np.zeros(max(n - 1, 1) if n else 0, BVHNODE_DT), np.zeros(n, np.uint32)
    qnodes, tri = np.zeros(int(sizes[0]), QNODE_DT), np.zeros((int(sizes[1]), 4), np.float32)
    pts, hit = np.zeros((int(sizes[2]), 4), np.float32), np.zeros(int(sizes[2]), np.uint32)
    if n and sizes[4] & 1:
        _chk(_lib.lib().pbrhip_qtree_collapse(*head, nodes.ctypes.data, order.ctypes.data, qnodes.ctypes.data, tri.ctypes.data,
                                              pts.ctypes.data, hit.ctypes.data, sizes.ctypes.data))
    return dict(nodes=nodes, order=order, depth=int(sizes[5]), qnodes=qnodes, tri=tri, pts=pts, hit=hit, stack_need=int(sizes[3]),
                fits=bool(sizes[4] & 1), quantised=bool(sizes[4] & 2))


def tree_refit(slots, nodes, qtree=None, device=None):
    """pbrhip_tree_refit (include/pbrhip.h): pbrhip_scene_refit's kernels on a bare tree.  slots: the NEW (n, 4, 4) float32 slots in leaf
    order; nodes: the max(n - 1, 1) BVHNODE_DT nodes; qtree: dict(qnodes, tri, pts, hit) as qtree_collapse returns it, or None for the
    binary tree alone -> (nodes, dict(qnodes, tri, pts, hit) or None), refitted copies.  A test hook."""
    slots = np.ascontiguousarray(slots, np.float32).reshape(-1, 4, 4)
    n = len(slots)
    nodes = np.array(nodes, BVHNODE_DT)
    if len(nodes) != (max(n - 1, 1) if n else 0):
        raise ValueError("nodes: max(n - 1, 1) of them")
    dev = _device if device is None else int(device)
    if qtree is None:
        _chk(_lib.lib().pbrhip_tree_refit(dev, n, slots.ctypes.data, nodes.ctypes.data, None, 0, None, 0, 0, None, None, 0))
        return nodes, None
    qn, tri = np.array(qtree["qnodes"], QNODE_DT), np.array(qtree["tri"], np.float32).reshape(-1, 4)
    pts, hit = np.array(qtree["pts"], np.float32).reshape(-1, 4), np.ascontiguousarray(qtree["hit"], np.uint32)
    if len(hit) != len(pts):
        raise ValueError("one hit code per point")
    tri_pairs = int(len(pts) == 8)  # (no curve record at all: a triangle-only tree, whose triangle leaves are TriPairs)
    _chk(_lib.lib().pbrhip_tree_refit(dev, n, slots.ctypes.data, nodes.ctypes.data, qn.ctypes.data, len(qn), tri.ctypes.data if len(tri) else None,
                                      len(tri), tri_pairs, pts.ctypes.data, hit.ctypes.data, len(pts)))
    return nodes, dict(qtree, qnodes=qn, tri=tri, pts=pts, hit=hit)


def math_mode():
    """'glibcf' (glibc's float functions restated bit for bit: the default) or 'f64r' (correctly rounded): pbrhip_math_mode()"""
    return {1: "f64r", 2: "glibcf"}[int(_lib.lib().pbrhip_math_mode())]


def device_count():
    n = C.c_int(0)
    _lib.lib().pbrhip_device_count(C.byref(n))
    return n.value


_device = 0  # what set_device selected (Denoise runs there)


def set_device(i):
    global _device
    _chk(_lib.lib().pbrhip_set_device(int(i)))
    _device = int(i)


def create_tiles(width, height):
    """CreateTiles (src/render-tile.cc:29-41): (n,4) array of sx,tx,sy,ty."""
    L = _lib.lib()
    n = C.c_uint32(0)
    _chk(L.pbrhip_create_tiles(width, height, None, C.byref(n)))
    out = np.zeros((n.value, 4), np.uint32)
    _chk(L.pbrhip_create_tiles(width, height, _ptr(out, u32p), C.byref(n)))
    return out


class RenderLayer:
    """pbrlab::RenderLayer (src/render-layer.h:11-26): rgba = sum of radiance (A = sample count), count."""

    def __init__(self, w=0, h=0):
        self.Resize(w, h)
        self.Clear()

    def Resize(self, w, h):
        self.width, self.height = int(w), int(h)
        self.rgba = np.zeros((self.height, self.width, 4), np.float32)
        self.count = np.zeros((self.height, self.width), np.uint32)

    def Clear(self):
        self.rgba[...] = 0
        self.count[...] = 0


ID_PRIMITIVE, ID_INSTANCE, ID_GEOM = 0, 1, 2  # PBRHIP_ID_*: which ShadeRec word Scene.ObjectIds gathers


class Scene:
    """pbrlab::Scene (src/scene.h:14-111) over libpbrhip."""

    def __init__(self):
        self.L = _lib.lib()
        h = C.c_void_p()
        _chk(self.L.pbrhip_scene_create(C.byref(h)))
        self.h = h
        self.device = _device

    def close(self):
        if getattr(self, "h", None):
            self.L.pbrhip_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def AddTriangleMesh(self, vertices, normals, texcoords, vertex_ids, normal_ids=None, texcoord_ids=None,
                        material_ids=None):
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        n = np.ascontiguousarray(normals if normals is not None else np.zeros((0, 4)), np.float32).reshape(-1, 4)
        t = np.ascontiguousarray(texcoords if texcoords is not None else np.zeros((0, 2)), np.float32).reshape(-1, 2)
        vid = np.ascontiguousarray(vertex_ids, np.uint32).reshape(-1, 3)
        nid = None if normal_ids is None else np.ascontiguousarray(normal_ids, np.uint32).reshape(-1, 3)
        tid = None if texcoord_ids is None else np.ascontiguousarray(texcoord_ids, np.uint32).reshape(-1, 3)
        mid = None if material_ids is None else np.ascontiguousarray(material_ids, np.uint32).reshape(-1)
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_add_triangle_mesh(self.h, _ptr(v), len(v), _ptr(n), len(n), _ptr(t), len(t),
                                                   _ptr(vid, u32p), _ptr(nid, u32p), _ptr(tid, u32p),
                                                   _ptr(mid, u32p), len(vid), C.byref(out)))
        return out.value

    def AddCubicBezierCurveMesh(self, vertices_xyzr, indices, material_ids=None):
        v = np.ascontiguousarray(vertices_xyzr, np.float32).reshape(-1, 4)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        mid = None if material_ids is None else np.ascontiguousarray(material_ids, np.uint32).reshape(-1)
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_add_curve_mesh(self.h, _ptr(v), len(v), _ptr(idx, u32p), _ptr(mid, u32p), len(idx),
                                                C.byref(out)))
        return out.value

    def AddMaterialParam(self, p):
        out = C.c_uint32()
        if isinstance(p, PrincipledParam):
            _chk(self.L.pbrhip_scene_add_principled_material(self.h, C.byref(p), C.byref(out)))
        elif isinstance(p, HairParam):
            _chk(self.L.pbrhip_scene_add_hair_material(self.h, C.byref(p), C.byref(out)))
        else:
            raise TypeError("material must be PrincipledParam or HairParam")
        return out.value

    def UpdateMaterialParam(self, material_id, p):
        """what EditQueue::EditAndPopAll does between renders (pc/pc-common.cc:57-84)."""
        if isinstance(p, PrincipledParam):
            _chk(self.L.pbrhip_scene_update_principled_material(self.h, material_id, C.byref(p)))
        else:
            _chk(self.L.pbrhip_scene_update_hair_material(self.h, material_id, C.byref(p)))

    def UpdateTriangleMesh(self, mesh_id, vertices, normals=None):
        """pbrhip_scene_update_triangle_mesh: new vertices (and normals; None: kept) of a triangle mesh, counts as it was added.  On a
        committed scene the scene is stale until RefitScene (or CommitScene)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
        n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        _chk(self.L.pbrhip_scene_update_triangle_mesh(self.h, mesh_id, v.ctypes.data, len(v), None if n is None else n.ctypes.data,
                                                      0 if n is None else len(n)))

    def UpdateCurveMesh(self, mesh_id, vertices_xyzr):
        """pbrhip_scene_update_curve_mesh: new control points xyz + radius of a curve mesh, as many as it was added with"""
        v = np.ascontiguousarray(vertices_xyzr, np.float32).reshape(-1, 4)
        _chk(self.L.pbrhip_scene_update_curve_mesh(self.h, mesh_id, v.ctypes.data, len(v)))

    def UpdateInstanceTransform(self, instance_id, transform=None):
        """pbrhip_scene_update_instance_transform: a new 4x4 transform of an instance (None: identity), as CreateInstance takes it"""
        t = None if transform is None else np.ascontiguousarray(transform, np.float32).reshape(16)
        _chk(self.L.pbrhip_scene_update_instance_transform(self.h, instance_id, None if t is None else t.ctypes.data))

    def UpdateTriangleMeshDevice(self, mesh_id, vertices, normals=None, stream=None):
        """pbrhip_scene_update_triangle_mesh_device: UpdateTriangleMesh from device memory of the scene's GPU.  vertices / normals: a
        float32, contiguous (n, 4) tensor on that device (anything with data_ptr(), as a torch tensor has), or a (pointer, count) pair;
        normals None: kept.  stream: the hipStream_t the arrays are produced on (None: with tensors torch's current stream, else the
        null stream); they are read after the work already enqueued there, and the library has its own copy when the call returns.
        From the first such call on a committed scene RefitScene stages on the GPU as well."""
        (vp, vn), (np_, nn), stream = _device_array(vertices, self), _device_array(normals, self), _device_stream(stream, vertices, normals)
        _chk(self.L.pbrhip_scene_update_triangle_mesh_device(self.h, mesh_id, vp, vn, np_, nn, stream))

    def UpdateCurveMeshDevice(self, mesh_id, vertices_xyzr, stream=None):
        """pbrhip_scene_update_curve_mesh_device: UpdateCurveMesh from device memory; arguments as UpdateTriangleMeshDevice's"""
        (vp, vn), stream = _device_array(vertices_xyzr, self), _device_stream(stream, vertices_xyzr)
        _chk(self.L.pbrhip_scene_update_curve_mesh_device(self.h, mesh_id, vp, vn, stream))

    def read_slots(self):
        """pbrhip_scene_read_slots, a test hook: the committed scene's slots (n, 4, 4) float32 in leaf order and its ShadeRecs (n, 32)
        uint32 as the device holds them"""
        n = C.c_uint32()
        _chk(self.L.pbrhip_scene_read_slots(self.h, None, None, C.byref(n)))
        slots, shade = np.zeros((n.value, 4, 4), np.float32), np.zeros((n.value, 32), np.uint32)
        _chk(self.L.pbrhip_scene_read_slots(self.h, slots.ctypes.data, shade.ctypes.data, C.byref(n)))
        return slots, shade

    def RefitScene(self):
        """pbrhip_scene_refit: the committed trees refitted on the GPU to the edited geometry; afterwards every observable equals that of
        a fresh scene built from the edited model and committed with the same builder"""
        _chk(self.L.pbrhip_scene_refit(self.h))

    def SnapshotPose(self):
        """pbrhip_scene_snapshot_pose: keeps the committed scene's slots and camera state on the device as the pose
        RenderMotion measures from.  Call it before the frame's edits; a second call replaces the first, CommitScene drops it."""
        _chk(self.L.pbrhip_scene_snapshot_pose(self.h))

    def ObjectIds(self, motion_layer, what=ID_INSTANCE, device_out=None, stream=None):
        """pbrhip_scene_object_ids: per pixel of RenderMotion's ident buffer (a MotionLayer, or the (H, W, 4) buffer itself)
        the primitive, instance or geometry id of the slot seen there, NONE for a miss -> (H, W) uint32.  A numpy ident travels through
        the host; an int32 tensor on the scene's GPU is read in place behind `stream` (None: torch's current one) and the result is an
        int32 tensor: device_out when given, else a new one."""
        ident = getattr(motion_layer, "ident", motion_layer)
        if what not in (ID_PRIMITIVE, ID_INSTANCE, ID_GEOM):
            raise ValueError(f"ObjectIds: what = {what} is none of ID_PRIMITIVE, ID_INSTANCE, ID_GEOM")
        h, w = (int(n) for n in tuple(ident.shape)[:2])
        if hasattr(ident, "data_ptr"):
            import torch
            src = _image_arg(ident, (h, w, 4), "int32", "ident", getattr(self, "device", None))[0]
            out = torch.empty((h, w), dtype=torch.int32, device=ident.device) if device_out is None else device_out
            dst = _image_arg(out, (h, w), "int32", "device_out", getattr(self, "device", None))[0]
            _chk(self.L.pbrhip_scene_object_ids_device(self.h, src, h * w, int(what), dst, _device_stream(stream, ident)))
            return out
        if device_out is not None:
            raise TypeError("ObjectIds: device_out goes with an ident tensor")
        src = _image_arg(ident, (h, w, 4), "uint32", "ident")[2]
        out = np.zeros((h, w), np.uint32)
        _chk(self.L.pbrhip_scene_object_ids(self.h, src.ctypes.data, h * w, int(what), out.ctypes.data))
        return out

    def AddTexture(self, pixels):
        """Scene::AddTexture: pixels (H, W, C) float32."""
        px = np.ascontiguousarray(pixels, np.float32)
        if px.ndim == 2:
            px = px[..., None]
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_add_texture(self.h, _ptr(px), px.shape[1], px.shape[0], px.shape[2], C.byref(out)))
        return out.value

    def SetEnvironment(self, rgb_hw3, scale=1.0, world_to_env=None):
        """A lat-long environment light: rgb_hw3 (H, W, 3) float radiance, row 0 = the top, times `scale`;
        world_to_env a 3x3 rotation (None: identity).  None removes it; an all-black map is none.  Takes effect at the next render."""
        if rgb_hw3 is None:
            _chk(self.L.pbrhip_scene_set_environment(self.h, None, 0, 0, C.c_float(1.0), None))
            return
        px = np.ascontiguousarray(rgb_hw3, np.float32)
        if px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("environment map must be (H, W, 3)")
        m = None if world_to_env is None else np.ascontiguousarray(world_to_env, np.float32).reshape(9)
        _chk(self.L.pbrhip_scene_set_environment(self.h, _ptr(px), px.shape[1], px.shape[0], C.c_float(scale), _ptr(m)))

    def SetCamera(self, eye, lookat=None, up=(0.0, 1.0, 0.0), fov=30.0, lens_radius=0.0, focus_distance=0.0):
        """A look-at camera: eye, lookat, up 3-vectors, fov = vertical field of view in degrees; lens_radius > 0 makes it
        a thin lens focused at focus_distance along the view direction (0: |lookat - eye|).  SetCamera(None) restores the reference's
        camera.  Takes effect at the next render; invalid values raise and leave the camera as it was."""
        if eye is None:
            _chk(self.L.pbrhip_scene_set_camera(self.h, None, None, None, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)))
            return
        if lookat is None:
            raise ValueError("SetCamera needs lookat")
        e, l, u = (np.ascontiguousarray(v, np.float32).reshape(3) for v in (eye, lookat, up))
        _chk(self.L.pbrhip_scene_set_camera(self.h, _ptr(e), _ptr(l), _ptr(u), C.c_float(fov), C.c_float(lens_radius),
                                            C.c_float(focus_distance)))

    def CameraRays(self, width, height, x_y_pass, seed_seq=1234567890):
        """pbrhip_camera_rays: the camera ray the renderer traces for each (x, y, pass) row of x_y_pass (n, 3) -> RAY_DT array.  The user
        camera when one is set, else the reference's (a committed scene)."""
        xyp = np.ascontiguousarray(x_y_pass, np.uint32).reshape(-1, 3)
        rays = np.zeros(len(xyp), RAY_DT)
        _chk(self.L.pbrhip_camera_rays(self.h, C.c_uint32(width), C.c_uint32(height), C.c_uint64(seed_seq), C.c_void_p(xyp.ctypes.data),
                                       C.c_size_t(len(xyp)), C.c_void_p(rays.ctypes.data)))
        return rays

    def ProjectionRays(self, projection, width, height, first_pass, num_pass, param=0.0, out=None, *, seed_seq=1234567890, stream=None):
        """pbrhip_projection_rays_device: the rays of passes [first_pass, first_pass + num_pass) of a width x height frame through
        `projection` -- "latlong" (a 360 degree panorama, param ignored), "fisheye" (equidistant; param = field of view in degrees up to
        360, 0 = the camera's fov) or "ortho" (param = half the height in world units) -- about SetCamera's frame, written on the
        device.  out: None (a new DeviceRays), a DeviceRays of that shape, or a float32 (num_pass, H, W, 8) tensor on the scene's
        device.  Returns out; RenderRays takes it with camera_draws = 2 and first_pass."""
        if isinstance(projection, str):
            if projection not in _PROJECTIONS:
                raise ValueError(f"unknown projection {projection!r}: one of {sorted(_PROJECTIONS)}")
            projection = _PROJECTIONS[projection]
        shape = (int(num_pass), int(height), int(width))
        if out is None:
            out = DeviceRays(shape, self.device)
        if isinstance(out, DeviceRays):
            if out.shape != shape:
                raise ValueError(f"out has the shape {out.shape}, the rays {shape}")
            ptr = out.ptr
        else:
            where, ptr, grid, _ = _ray_source(out, self, num_pass)
            if where != "device" or grid != shape:
                raise ValueError(f"out: a float32 tensor of shape {shape + (8,)} on the scene's device")
        _chk(self.L.pbrhip_projection_rays_device(self.h, int(projection), float(param), int(width), int(height), int(first_pass), int(num_pass),
                                                  C.c_uint64(seed_seq), C.c_void_p(ptr), _device_stream(stream, out)))
        return out

    def AddLightParam(self, emission):
        e = np.ascontiguousarray(emission, np.float32).reshape(3)
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_add_area_light(self.h, _ptr(e), C.byref(out)))
        return out.value

    def CreateLocalScene(self):
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_create_local_scene(self.h, C.byref(out)))
        return out.value

    def AddMeshToLocalScene(self, local_id, mesh_id):
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_add_mesh_to_local_scene(self.h, local_id, mesh_id, C.byref(out)))
        return out.value

    def CreateInstance(self, local_id, transform=None):
        t = None if transform is None else np.ascontiguousarray(transform, np.float32).reshape(16)
        out = C.c_uint32()
        _chk(self.L.pbrhip_scene_create_instance(self.h, local_id, _ptr(t), C.byref(out)))
        return out.value

    def AttachLightParamIdsToInstance(self, instance_id, ids_per_geom):
        for g, ids in enumerate(ids_per_geom):
            a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
            _chk(self.L.pbrhip_scene_attach_light_ids(self.h, instance_id, g, _ptr(a, u32p), len(a)))

    def AttachMaterialParamIdsToInstance(self, instance_id, ids_per_geom):
        for g, ids in enumerate(ids_per_geom):
            a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
            _chk(self.L.pbrhip_scene_attach_material_ids(self.h, instance_id, g, _ptr(a, u32p), len(a)))

    def CommitScene(self):
        _chk(self.L.pbrhip_scene_commit(self.h))

    def SetBvhBuilder(self, builder):
        """BVH_HOST_SAH (default), BVH_GPU_LBVH or BVH_GPU_LBVH_WIDE; before CommitScene (pbrhip_scene_set_bvh_builder)"""
        _chk(self.L.pbrhip_scene_set_bvh_builder(self.h, int(builder)))

    def FetchSceneAABB(self):
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        _chk(self.L.pbrhip_scene_aabb(self.h, _ptr(lo), _ptr(hi)))
        return lo, hi

    def info(self):
        nn, ns, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        dp = C.c_uint32()
        _chk(self.L.pbrhip_scene_info(self.h, C.byref(nn), C.byref(ns), C.byref(dp), C.byref(nb)))
        return dict(num_nodes=nn.value, num_slots=ns.value, depth=dp.value, device_bytes=nb.value)

    def shadow_grid_info(self):
        """pbrhip_scene_shadow_grid_info: the per-light shaft grid of the committed scene (resolution 0: none) and what it did in the
        scene's last statistics render (culled_shadow_rays: the shadow rays it answers)"""
        gi = ShadowGridInfo()
        _chk(self.L.pbrhip_scene_shadow_grid_info(self.h, C.byref(gi)))
        return {n: getattr(gi, n) for n, _ in gi._fields_ if n != "pad"}

    def read_shadow_grid(self):
        """pbrhip_scene_read_shadow_grid: the cells, (lights, n, n, n, 8) uint32: count or 0xFFFFFFFF, then the listed leaf indices"""
        gi = self.shadow_grid_info()
        n, nl = gi["resolution"], gi["num_lights"]
        cells = np.zeros((nl, n, n, n, 8), np.uint32)
        _chk(self.L.pbrhip_scene_read_shadow_grid(self.h, _ptr(cells), C.c_size_t(cells.size)))
        return cells

    def wide_info(self):
        """pbrhip_scene_wide_info: the 4-wide quantised tree of the committed scene (wide_nodes 0: none)"""
        nn, need, gpu = C.c_uint64(), C.c_uint32(), C.c_int()
        _chk(self.L.pbrhip_scene_wide_info(self.h, C.byref(nn), C.byref(need), C.byref(gpu)))
        return dict(wide_nodes=nn.value, stack_need=need.value, built_on_gpu=bool(gpu.value))

    # Raytracer::FirstHitTrace1 / AnyHit1 over ray arrays
    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, RAY_DT)
        hits = np.zeros(len(rays), HIT_DT)
        _chk(self.L.pbrhip_trace_closest(self.h, C.c_void_p(rays.ctypes.data), C.c_size_t(len(rays)),
                                         C.c_void_p(hits.ctypes.data)))
        return hits

    def texture_fetch(self, texture_id, uv):
        """pbrhip_texture_fetch: Texture::FetchFloat3 of a texture of this committed scene at (n, 2) coordinates -> (n, 3).  A test hook."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        rgb = np.zeros((len(uv), 3), np.float32)
        _chk(self.L.pbrhip_texture_fetch(self.h, C.c_uint32(texture_id), C.c_void_p(uv.ctypes.data), C.c_size_t(len(uv)), C.c_void_p(rgb.ctypes.data)))
        return rgb

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, RAY_DT)
        occ = np.zeros(len(rays), np.uint8)
        _chk(self.L.pbrhip_trace_any(self.h, C.c_void_p(rays.ctypes.data), C.c_size_t(len(rays)),
                                     C.c_void_p(occ.ctypes.data)))
        return occ

    # ray and nearest-point queries from device memory
    def TraceClosestDevice(self, rays, ident=None, hits=None, stream=None):
        """pbrhip_trace_closest_device: the closest hit of n rays held in memory of the scene's GPU -> (ident, hits).  rays: a float32,
        contiguous (n, 8) tensor (org, tmin, dir, tmax per row: RAY_DT) or a (pointer, n) pair.  ident: (n, 4) int32 = slot (NONE: a miss),
        bits of u, v, t -- RenderMotion's identity format, ObjectIds takes it; hits: (n, 9) int32 holding trace_closest's HIT_DT records
        bit for bit.  Each is a tensor or a device pointer (an int) and is written in place; with tensor rays and neither given both are
        allocated; one that is not given otherwise is not computed (None).  stream: the stream the rays are produced on (None: with
        tensors torch's current one): they are read after the work already enqueued there; the outputs are written when the call returns.
        Device pointers of rays and ident must be 16-byte aligned (the library refuses others); a tensor that starts its allocation is."""
        ptr, n = _query_array(rays, self, 8, "rays")
        if ident is None and hits is None and hasattr(rays, "data_ptr"):
            import torch
            ident, hits = (torch.empty((n, w), dtype=torch.int32, device=rays.device) for w in (4, 9))
        pi, ph = _query_out(ident, self, (n, 4), "int32", "ident"), _query_out(hits, self, (n, 9), "int32", "hits")
        _chk(self.L.pbrhip_trace_closest_device(self.h, ptr, n, _device_stream(stream, rays), pi, ph))
        return ident, hits

    def TraceAnyDevice(self, rays, out=None, stream=None):
        """pbrhip_trace_any_device: whether each of n rays in memory of the scene's GPU is blocked -> out, (n,) uint8 (a tensor or a device
        pointer; allocated when rays is a tensor and none is given).  rays and stream as TraceClosestDevice's."""
        ptr, n = _query_array(rays, self, 8, "rays")
        if out is None and hasattr(rays, "data_ptr"):
            import torch
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        _chk(self.L.pbrhip_trace_any_device(self.h, ptr, n, _device_stream(stream, rays), _query_out(out, self, (n,), "uint8", "out")))
        return out

    def NearestPoint(self, points):
        """pbrhip_nearest_point: per query point the nearest primitive within max_dist -> (ident, closest).  points: POINT_DT records,
        or (n, 4) float32 rows x, y, z, max_dist (inf: no bound).  ident: (n, 4) uint32 = slot (NONE: a miss), bits of u, v,
        sqrt(D2); closest: (n, 4) float32 = the closest point | D2 (zeros for a miss).  The definition of D2 is exact.
        Anything else than records or (n, 4) rows: ValueError, before any C call."""
        points = np.asarray(points)
        if points.dtype.names:
            pts = np.ascontiguousarray(points, POINT_DT).reshape(-1)
        elif points.ndim == 2 and points.shape[1] == 4:
            pts = np.ascontiguousarray(points, np.float32)
        else:
            raise ValueError(f"points must be POINT_DT records or have the shape (n, 4), not {points.shape}")
        n = len(pts)
        ident, closest = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.float32)
        _chk(self.L.pbrhip_nearest_point(self.h, C.c_void_p(pts.ctypes.data), n, C.c_void_p(ident.ctypes.data), C.c_void_p(closest.ctypes.data)))
        return ident, closest

    def NearestPointDevice(self, points, ident=None, closest=None, stream=None):
        """pbrhip_nearest_point_device: NearestPoint for n points in memory of the scene's GPU -> (ident, closest).  points: a float32,
        contiguous (n, 4) tensor or a (pointer, n) pair; ident: (n, 4) int32, closest: (n, 4) float32, tensors or device pointers written
        in place; outputs and stream as TraceClosestDevice's.  Device pointers must be 16-byte aligned (the library refuses others)."""
        ptr, n = _query_array(points, self, 4, "points")
        if ident is None and closest is None and hasattr(points, "data_ptr"):
            import torch
            ident = torch.empty((n, 4), dtype=torch.int32, device=points.device)
            closest = torch.empty((n, 4), dtype=torch.float32, device=points.device)
        pi, pc = _query_out(ident, self, (n, 4), "int32", "ident"), _query_out(closest, self, (n, 4), "float32", "closest")
        _chk(self.L.pbrhip_nearest_point_device(self.h, ptr, n, _device_stream(stream, points), pi, pc))
        return ident, closest

    # all-hits ray queries
    def TraceAll(self, rays, max_hits):
        """pbrhip_trace_all: per ray the number of accepted hits in (tmin, tmax] and the max_hits nearest of them -> (count, ident).
        rays: RAY_DT records or (n, 8) float32 rows org, tmin, dir, tmax (host memory).  count: (n,) uint32, every accepted hit, not
        capped by max_hits; ident: (n, max_hits, 4) uint32, per ray the hits ordered by (t, canonical primitive id, u) as slot, bits of
        u, v, t -- TraceClosestDevice's identity format, and ident[:, 0] equals its ident --, the entries past count (NONE, 0, 0, 0).
        max_hits in [0, ALL_HITS_MAX].  Anything else than records or (n, 8) rows, or a max_hits outside that: ValueError, before any C
        call."""
        max_hits = _all_hits_k(max_hits)
        rays = np.asarray(rays)
        if rays.dtype.names:
            r = np.ascontiguousarray(rays, RAY_DT).reshape(-1)
        elif rays.ndim == 2 and rays.shape[1] == 8:
            r = np.ascontiguousarray(rays, np.float32)
        else:
            raise ValueError(f"rays must be RAY_DT records or have the shape (n, 8), not {rays.shape}")
        n = len(r)
        count, ident = np.zeros(n, np.uint32), np.zeros((n, max_hits, 4), np.uint32)
        _chk(self.L.pbrhip_trace_all(self.h, C.c_void_p(r.ctypes.data), n, max_hits, C.c_void_p(count.ctypes.data), C.c_void_p(ident.ctypes.data)))
        return count, ident

    def TraceAllDevice(self, rays, max_hits, count=True, ident=True, stream=None):
        """pbrhip_trace_all_device: TraceAll for n rays in memory of the scene's GPU -> (count, ident).  rays and stream as
        TraceClosestDevice's.  count: (n,) int32, ident: (n, max_hits, 4) int32 -- ObjectIds takes its (1, n * max_hits, 4) view --, each
        True (allocated with torch; rays must be a tensor), a tensor or a device pointer (an int) written in place, or False / None: not
        computed (returned as None).  With max_hits == 0 there is no ident.  Not both may be left out.  Without count the traversal stops
        at the max_hits-th hit; with it every box the ray crosses is entered.  Device pointers of rays and ident must be 16-byte aligned."""
        max_hits = _all_hits_k(max_hits)
        ptr, n = _query_array(rays, self, 8, "rays")
        count, ident = (None if a is False else a for a in (count, ident))
        if max_hits == 0:
            ident = None
        if count is None and ident is None:
            raise ValueError("TraceAllDevice: neither count nor ident is wanted" + (" (max_hits == 0 leaves the count)" if max_hits == 0 else ""))
        if count is True or ident is True:
            if not hasattr(rays, "data_ptr"):
                raise TypeError("TraceAllDevice: outputs are allocated only beside tensor rays: pass tensors or device pointers")
            import torch
            if count is True:
                count = torch.empty((n,), dtype=torch.int32, device=rays.device)
            if ident is True:
                ident = torch.empty((n, max_hits, 4), dtype=torch.int32, device=rays.device)
        pc, pi = _query_out(count, self, (n,), "int32", "count"), _query_out(ident, self, (n, max_hits, 4), "int32", "ident")
        _chk(self.L.pbrhip_trace_all_device(self.h, ptr, n, max_hits, _device_stream(stream, rays), pc, pi))
        return count, ident

    # k-nearest queries
    def KNearest(self, points, max_k):
        """pbrhip_k_nearest: per query point the number of primitives within max_dist and the max_k nearest of them -> (count, ident,
        closest).  points: POINT_DT records or (n, 4) float32 rows x, y, z, max_dist (inf: no bound; host memory).  count: (n,) uint32,
        every unit with D2 <= max_dist^2, not capped by max_k; ident: (n, max_k, 4) uint32, per query the units ordered by (D2, canonical
        primitive id, piece index) as slot, bits of u, v, sqrt(D2) -- NearestPoint's format, and ident[:, 0] is its answer --, the
        entries past count (NONE, 0, 0, 0); closest: (n, max_k, 4) float32 = the closest point | D2 of each listed entry, zeros past
        them.  The order is D2's: sqrt merges distinct D2, closest[..., 3] has the strict order.  max_k in [0, K_NEAREST_MAX].
        Anything else than records or (n, 4) rows, or a max_k outside that: ValueError, before any C call."""
        max_k = _k_nearest_k(max_k)
        points = np.asarray(points)
        if points.dtype.names:
            pts = np.ascontiguousarray(points, POINT_DT).reshape(-1)
        elif points.ndim == 2 and points.shape[1] == 4:
            pts = np.ascontiguousarray(points, np.float32)
        else:
            raise ValueError(f"points must be POINT_DT records or have the shape (n, 4), not {points.shape}")
        n = len(pts)
        count, ident, closest = np.zeros(n, np.uint32), np.zeros((n, max_k, 4), np.uint32), np.zeros((n, max_k, 4), np.float32)
        _chk(self.L.pbrhip_k_nearest(self.h, C.c_void_p(pts.ctypes.data), n, max_k, C.c_void_p(count.ctypes.data), C.c_void_p(ident.ctypes.data),
                                     C.c_void_p(closest.ctypes.data)))
        return count, ident, closest

    def KNearestDevice(self, points, max_k, count=True, ident=True, closest=False, stream=None):
        """pbrhip_k_nearest_device: KNearest for n points in memory of the scene's GPU -> (count, ident, closest).  points and stream as
        NearestPointDevice's.  count: (n,) int32, ident: (n, max_k, 4) int32 -- ObjectIds takes its (1, n * max_k, 4) view --, closest:
        (n, max_k, 4) float32, each True (allocated with torch; points must be a tensor), a tensor or a device pointer (an int) written
        in place, or False / None: not computed (returned as None).  With max_k == 0 there is neither ident nor closest; closest needs
        ident (the list lives in its rows); count and ident may not both be left out.  Without count the traversal's bound shrinks to
        the max_k-th entry once the list is full; with it every box within max_dist is entered (max_dist = inf: the whole tree).
        Device pointers of points, ident and closest must be 16-byte aligned."""
        max_k = _k_nearest_k(max_k)
        ptr, n = _query_array(points, self, 4, "points")
        count, ident, closest = (None if a is False else a for a in (count, ident, closest))
        if max_k == 0:
            ident = closest = None
        if count is None and ident is None:
            raise ValueError("KNearestDevice: neither count nor ident is wanted" + (" (max_k == 0 leaves the count)" if max_k == 0 else ""))
        if closest is not None and ident is None:
            raise ValueError("KNearestDevice: closest needs ident: the list lives in the ident rows")
        if count is True or ident is True or closest is True:
            if not hasattr(points, "data_ptr"):
                raise TypeError("KNearestDevice: outputs are allocated only beside tensor points: pass tensors or device pointers")
            import torch
            if count is True:
                count = torch.empty((n,), dtype=torch.int32, device=points.device)
            if ident is True:
                ident = torch.empty((n, max_k, 4), dtype=torch.int32, device=points.device)
            if closest is True:
                closest = torch.empty((n, max_k, 4), dtype=torch.float32, device=points.device)
        pc, pi = _query_out(count, self, (n,), "int32", "count"), _query_out(ident, self, (n, max_k, 4), "int32", "ident")
        pq = _query_out(closest, self, (n, max_k, 4), "float32", "closest")
        _chk(self.L.pbrhip_k_nearest_device(self.h, ptr, n, max_k, _device_stream(stream, points), pc, pi, pq))
        return count, ident, closest

    # signed distance
    def SignedDistance(self, points):
        """pbrhip_signed_distance: NearestPoint with a sign -> (ident, closest, sd).  points, ident and closest as NearestPoint's (and
        equal to them); sd: (n, 4) float32 = the pseudonormal N of the feature of the nearest triangle the closest point lies on, then the
        signed distance: sqrt(D2) outside (dot(p - q, N) >= 0), -sqrt(D2) inside; a curve piece: N = 0 and a positive distance; a miss:
        zeros.  Anything else than records or (n, 4) rows: ValueError, before any C call."""
        points = np.asarray(points)
        if points.dtype.names:
            pts = np.ascontiguousarray(points, POINT_DT).reshape(-1)
        elif points.ndim == 2 and points.shape[1] == 4:
            pts = np.ascontiguousarray(points, np.float32)
        else:
            raise ValueError(f"points must be POINT_DT records or have the shape (n, 4), not {points.shape}")
        n = len(pts)
        ident, closest, sd = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        _chk(self.L.pbrhip_signed_distance(self.h, C.c_void_p(pts.ctypes.data), n, C.c_void_p(ident.ctypes.data), C.c_void_p(closest.ctypes.data),
                                           C.c_void_p(sd.ctypes.data)))
        return ident, closest, sd

    def SignedDistanceDevice(self, points, ident=None, closest=None, sd=None, stream=None):
        """pbrhip_signed_distance_device: SignedDistance for n points in memory of the scene's GPU -> (ident, closest, sd).  points: a
        float32, contiguous (n, 4) tensor or a (pointer, n) pair; ident: (n, 4) int32, closest and sd: (n, 4) float32, tensors or device
        pointers written in place; with tensor points and none given all three are allocated; one that is not given otherwise is not
        computed (None).  stream as NearestPointDevice's.  Device pointers must be 16-byte aligned (the library refuses others)."""
        ptr, n = _query_array(points, self, 4, "points")
        if ident is None and closest is None and sd is None and hasattr(points, "data_ptr"):
            import torch
            ident = torch.empty((n, 4), dtype=torch.int32, device=points.device)
            closest, sd = (torch.empty((n, 4), dtype=torch.float32, device=points.device) for _ in range(2))
        pi, pc = _query_out(ident, self, (n, 4), "int32", "ident"), _query_out(closest, self, (n, 4), "float32", "closest")
        ps = _query_out(sd, self, (n, 4), "float32", "sd")
        _chk(self.L.pbrhip_signed_distance_device(self.h, ptr, n, _device_stream(stream, points), pi, pc, ps))
        return ident, closest, sd

    def SignedDistanceGridDevice(self, origin, spacing, dims, max_dist=float("inf"), out=None, stream=None):
        """pbrhip_signed_distance_grid_device: the signed distance at origin + (i, j, k) * spacing for i < dims[0], j < dims[1],
        k < dims[2] -> out, a float32 (dims[2], dims[1], dims[0]) tensor on the scene's GPU (x fastest: what
        torch.nn.functional.grid_sample takes as a volume) or a device pointer, written in place; allocated with torch when none is given.
        0 where nothing lies within max_dist.  origin, spacing: three floats; dims: three integers >= 0, fewer than 2^31 points in all --
        checked here, before any C call."""
        o, sp = np.ascontiguousarray(origin, np.float32).reshape(-1), np.ascontiguousarray(spacing, np.float32).reshape(-1)
        if o.shape != (3,) or sp.shape != (3,) or len(dims) != 3:
            raise ValueError("origin, spacing and dims have three components each")
        if any(int(d) != d or d < 0 for d in dims):
            raise ValueError(f"dims must be three integers >= 0, not {tuple(dims)}")
        dm = np.array([int(d) for d in dims], np.uint64)
        if int(dm[0]) * int(dm[1]) * int(dm[2]) >= 1 << 31:
            raise ValueError("a grid has fewer than 2^31 points")
        dm = dm.astype(np.uint32)
        shape = (int(dm[2]), int(dm[1]), int(dm[0]))
        if out is None:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.device}")
        po = _query_out(out, self, shape, "float32", "out")
        _chk(self.L.pbrhip_signed_distance_grid_device(self.h, C.c_void_p(o.ctypes.data), C.c_void_p(sp.ctypes.data), C.c_void_p(dm.ctypes.data),
                                                       float(max_dist), _device_stream(stream, out), po))
        return out

    def SignedDistanceInfo(self):
        """pbrhip_scene_signed_distance_info: builds the pseudonormal table if it has to -> dict(triangles, vertices, edges_manifold,
        edges_boundary, edges_nonmanifold, edges_inconsistent, table_bytes, topology_ms, table_ms).  The sign is a guarantee only where the
        nearest object has no boundary, non-manifold or inconsistently oriented edge."""
        info = SdInfo()
        _chk(self.L.pbrhip_scene_signed_distance_info(self.h, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_}

    def read_pseudonormals(self):
        """pbrhip_scene_read_pseudonormals, a test hook: the pseudonormal table as the device holds it, (n, 7, 4) float32 in slot order:
        rows ab, bc, ca, a, b, c, face (xyz, 0); zeros for a curve slot"""
        n = C.c_uint32()
        _chk(self.L.pbrhip_scene_read_pseudonormals(self.h, None, C.byref(n)))
        out = np.zeros((n.value, 7, 4), np.float32)
        _chk(self.L.pbrhip_scene_read_pseudonormals(self.h, out.ctypes.data, C.byref(n)))
        return out


def Render(scene, width, height, num_sample, cancel_render_flag=None, layer=None, finish_pass=None, *,
           first_pass=0, seed_seq=1234567890, tile_rank=0, tile_world=1, max_paths_in_flight=0, flags=0,
           device_out=None, num_streams=0, tail_paths=0, shard_block=0):
    """pbrlab::Render (src/render.h:14-17).  Resizes and clears `layer`, renders `num_sample` passes, and
    returns (True, stats) -- the reference always returns true (render.cc:240).

    cancel_render_flag: optional ctypes.c_ubyte (the byte of the reference's std::atomic_bool) another thread may set
    while the call runs; it is read at every host round trip of the render loop.
    finish_pass: optional ctypes.c_size_t, stored to while the call runs as groups of passes complete.
    device_out: optional (rgba_ptr, count_ptr) DEVICE pointers (ints); then the layer is not touched and
    nothing is copied to the host (used with torch tensors + RCCL reduce)."""
    L = _lib.lib()
    desc = RenderDesc(width, height, num_sample, first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight,
                      flags, num_streams, tail_paths, shard_block)
    st = RenderStats()
    fin = finish_pass if finish_pass is not None else C.c_size_t(0)
    cancel = C.byref(cancel_render_flag) if cancel_render_flag is not None else None
    if device_out is not None:
        _chk(L.pbrhip_render_device(scene.h, C.byref(desc), cancel, C.c_void_p(device_out[0]),
                                    C.c_void_p(device_out[1]), C.byref(fin), C.byref(st)))
        return True, st.as_dict()
    if layer is None:
        raise ValueError("layer is required")
    if not (flags & RENDER_NO_CLEAR):
        layer.Resize(width, height)  # PrepareRendering (render.cc:99-100)
    _chk(L.pbrhip_render(scene.h, C.byref(desc), cancel, _ptr(layer.rgba), _ptr(layer.count, u32p), C.byref(fin),
                         C.byref(st)))
    return True, st.as_dict()


# pbrhip_denoise's defaults (include/pbrhip.h PBRHIP_DENOISE_*)
DENOISE_NO_ALBEDO = 1
DENOISE_ITERATIONS, DENOISE_NORMAL_SQUARINGS, DENOISE_SIGMA_COLOR, DENOISE_SIGMA_DEPTH = 5, 7, 0.5, 0.2


class FeatureLayer:
    """First-hit feature buffers (pbrhip_render_features): albedo (H, W, 4) = sum of albedo rgb | hits, normal_depth
    (H, W, 4) = sum of the viewer-facing shading normal | sum of the hit distance, count (H, W) = samples."""

    def __init__(self, w=0, h=0):
        self.Resize(w, h)

    def Resize(self, w, h):
        self.width, self.height = int(w), int(h)
        self.albedo = np.zeros((self.height, self.width, 4), np.float32)
        self.normal_depth = np.zeros((self.height, self.width, 4), np.float32)
        self.count = np.zeros((self.height, self.width), np.uint32)

    def Clear(self):
        self.albedo[...] = 0
        self.normal_depth[...] = 0
        self.count[...] = 0

    def mean_albedo(self):
        """(H, W, 3): the mean albedo over all samples, a miss counting as white (what the filter demodulates by); 1 without samples"""
        m = self.count.astype(np.float64)[..., None]
        a = self.albedo.astype(np.float64)
        return np.where(m > 0, (a[..., :3] + (m - a[..., 3:4])) / np.maximum(m, 1), 1.0).astype(np.float32)

    def mean_normal(self):
        """(H, W, 3): the normalised normal sum; 0 where no sample hit"""
        n = self.normal_depth[..., :3].astype(np.float64)
        l = np.sqrt((n * n).sum(-1, keepdims=True))
        return np.where(l > 0, n / np.where(l > 0, l, 1), 0.0).astype(np.float32)

    def mean_depth(self):
        """(H, W): the mean hit distance over the samples that hit; inf where none did"""
        k = self.albedo[..., 3].astype(np.float64)
        return np.where(k > 0, self.normal_depth[..., 3] / np.where(k > 0, k, 1), np.inf).astype(np.float32)


def RenderFeatures(scene, width, height, num_sample, layer=None, *, first_pass=0, seed_seq=1234567890, tile_rank=0, tile_world=1,
                   max_paths_in_flight=0, shard_block=0, no_clear=False, device_out=None):
    """pbrhip_render_features: the first-hit features of passes [first_pass, first_pass + num_sample) of the frame Render makes from the
    same arguments, into `layer` (a FeatureLayer; resized unless no_clear, which accumulates on top).  Returns the layer.
    device_out: optional (albedo_ptr, normal_depth_ptr, count_ptr) DEVICE pointers (ints, 0 / None = not wanted) instead of a layer."""
    L = _lib.lib()
    desc = RenderDesc(width, height, num_sample, first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight,
                      RENDER_NO_CLEAR if no_clear else 0, 0, 0, shard_block)
    if device_out is not None:
        _chk(L.pbrhip_render_features_device(scene.h, C.byref(desc), *[C.c_void_p(p or None) for p in device_out]))
        return None
    if layer is None:
        layer = FeatureLayer()
    if not no_clear or (layer.width, layer.height) != (width, height):
        layer.Resize(width, height)
    _chk(L.pbrhip_render_features(scene.h, C.byref(desc), layer.albedo.ctypes.data, layer.normal_depth.ctypes.data, layer.count.ctypes.data))
    return layer


# pbrhip_projection_rays_device's projections (include/pbrhip.h PBRHIP_PROJECTION_*)
PROJECTION_LATLONG, PROJECTION_FISHEYE, PROJECTION_ORTHO = 0, 1, 2
_PROJECTIONS = {"latlong": PROJECTION_LATLONG, "fisheye": PROJECTION_FISHEYE, "ortho": PROJECTION_ORTHO}
RAY_BUFFER_BYTES = 256 << 20  # RenderProjection's cap on its ray buffer: it renders in chunks of passes that fit


class DeviceRays:
    """A buffer of rays in device memory, allocated through the library (the HIP runtime it is linked with): .ptr, .shape = (P, H, W),
    .device.  numpy() downloads it as a RAY_DT array; close() (or the collector) frees it."""

    def __init__(self, shape, device):
        self.shape, self.device = tuple(int(n) for n in (shape if isinstance(shape, (tuple, list)) else (shape,))), int(device)
        self.L = _lib.lib()
        self.nbytes = int(np.prod(self.shape)) * RAY_DT.itemsize
        _chk(self.L.pbrhip_set_device(self.device))
        p = C.c_void_p()
        self._hip(self.L.hipMalloc(C.byref(p), C.c_size_t(max(self.nbytes, 1))), "hipMalloc")
        self.ptr = p.value

    @staticmethod
    def _hip(rc, what):
        if rc != 0:
            raise PbrHipError(-4, f"{what} failed with HIP error {rc}")

    def upload(self, rays):
        a = np.ascontiguousarray(rays)
        if a.nbytes != self.nbytes:
            raise ValueError("upload: the array does not have the buffer's size")
        self._hip(self.L.hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(a.ctypes.data), C.c_size_t(self.nbytes), 1), "hipMemcpy")
        return self

    def numpy(self):
        out = np.zeros(self.shape, RAY_DT)
        if self.nbytes:
            self._hip(self.L.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), 2), "hipMemcpy")
        return out

    def close(self):
        if getattr(self, "ptr", None):
            self.L.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ray_grid(shape, last, what):
    """(P, H, W) of a ray array's shape: (H, W) or (P, H, W), followed by `last` when it is not None"""
    shape = tuple(int(n) for n in shape)
    if last is not None:
        if len(shape) not in (3, 4) or shape[-1] != last:
            raise ValueError(f"{what} must have the shape (H, W, {last}) or (P, H, W, {last}), not {shape}")
        shape = shape[:-1]
    elif len(shape) not in (2, 3):
        raise ValueError(f"{what} must have the shape (H, W) or (P, H, W), not {shape}")
    p, h, w = ((1,) + shape)[-3:]
    if h <= 0 or w <= 0 or p <= 0:
        raise ValueError(f"{what} is empty: {shape}")
    return p, h, w


def _ray_source(rays, scene, num_sample):
    """The rays argument of RenderRays / RenderFeaturesRays -> (where, pointer, (P, H, W), keep-alive): a numpy RAY_DT array (H, W) or
    (P, H, W), a numpy float32 array (H, W, 8) or (P, H, W, 8) (org, tmin, dir, tmax), a DeviceRays, a (pointer, shape) pair of device
    memory, or a float32 tensor on the scene's device with data_ptr() and the float shapes.  P is 1 or num_sample.  TypeError /
    ValueError here, before any C call."""
    keep = rays
    if isinstance(rays, np.ndarray):
        if rays.dtype == RAY_DT:
            grid = _ray_grid(rays.shape, None, "a RAY_DT array")
        elif rays.dtype == np.float32:
            grid = _ray_grid(rays.shape, 8, "a float32 ray array")
        else:
            raise TypeError(f"a ray array must be RAY_DT or float32, not {rays.dtype}")
        keep = np.ascontiguousarray(rays)
        where, ptr = "host", keep.ctypes.data
    elif isinstance(rays, DeviceRays):
        where, ptr, grid = "device", rays.ptr, _ray_grid(rays.shape, None, "a DeviceRays buffer")
    elif isinstance(rays, (tuple, list)):
        if len(rays) != 2 or not isinstance(rays[1], (tuple, list)):
            raise TypeError("device rays are a tensor, a DeviceRays or a (pointer, (P, H, W)) pair")
        if not rays[0]:
            raise ValueError("the ray pointer is NULL")
        where, ptr, grid = "device", int(rays[0]), _ray_grid(rays[1], None, "a device ray buffer")
    elif hasattr(rays, "data_ptr"):
        if not str(getattr(rays, "dtype", "")).endswith("float32"):
            raise TypeError(f"a ray tensor must be float32, not {getattr(rays, 'dtype', None)}")
        grid = _ray_grid(getattr(rays, "shape", ()), 8, "a ray tensor")
        if not rays.is_contiguous():
            raise ValueError("a ray tensor must be contiguous")
        dev = getattr(rays, "device", None)
        if getattr(dev, "type", None) != "cuda":
            raise ValueError(f"a ray tensor must be in GPU memory, not on {dev}")
        want = getattr(scene, "device", None)
        if want is not None and dev.index is not None and dev.index != want:
            raise ValueError(f"the rays are on device {dev.index}, the scene on device {want}")
        where, ptr = "device", int(rays.data_ptr())
    else:
        raise TypeError(f"{type(rays).__name__} is no ray array")
    if grid[0] not in (1, int(num_sample)):
        raise ValueError(f"{grid[0]} planes of rays: one (reused by every pass) or num_sample = {num_sample}")
    return where, ptr, grid, keep


def RenderRays(scene, rays, num_sample, layer=None, *, camera_draws=2, device_out=None, stream=None, cancel_render_flag=None,
               finish_pass=None, **desc_kw):
    """pbrhip_render_rays: Render with the first ray of every sample taken from `rays` (see _ray_source for what it may
    be: host or device, (H, W) = one ray per pixel reused by every pass, or (num_sample, H, W)); the image is W x H.  A ray is traced as
    given, tmin and tmax included; its direction must be of unit length.  camera_draws (0 .. 16): how many draws of the sample's
    generator the rays' maker consumed -- 2 replays the reference's camera and a pinhole from Scene.CameraRays bit for bit, 4 a thin
    lens.  An inactive ray (NaN, infinite, zero direction, tmin < 0, tmax < tmin) adds (0, 0, 0, 1).  desc_kw: Render's keywords
    (first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight, flags, num_streams, tail_paths, shard_block); with per-pass rays
    and first_pass the buffer starts at first_pass.  stream: the hipStream_t device rays are produced on (None: torch's current stream
    for a tensor, else the null stream).  Returns the layer (made when None; resized and cleared unless RENDER_NO_CLEAR) with .stats
    attached; with device_out = (rgba_ptr, count_ptr) DEVICE pointers no layer is touched and the stats are returned."""
    if not 0 <= int(camera_draws) <= 16:
        raise ValueError(f"camera_draws {camera_draws} is not in 0 .. 16")
    where, ptr, (planes, height, width), keep = _ray_source(rays, scene, num_sample)
    if where == "host" and device_out is not None:
        raise ValueError("device_out needs rays in device memory")
    L = _lib.lib()
    desc = _desc(width, height, num_sample, **desc_kw)
    st = RenderStats()
    fin = finish_pass if finish_pass is not None else C.c_size_t(0)
    cancel = C.byref(cancel_render_flag) if cancel_render_flag is not None else None
    h = scene.h if scene is not None else None
    if device_out is not None:
        _chk(L.pbrhip_render_rays_device(h, C.byref(desc), ptr, planes, int(camera_draws), _device_stream(stream, rays), cancel,
                                         C.c_void_p(device_out[0]), C.c_void_p(device_out[1]), C.byref(fin), C.byref(st)))
        return st.as_dict()
    if layer is None:
        layer = RenderLayer()
    if not (desc.flags & RENDER_NO_CLEAR) or (layer.width, layer.height) != (width, height):
        layer.Resize(width, height)
    if where == "host":
        _chk(L.pbrhip_render_rays(h, C.byref(desc), ptr, planes, int(camera_draws), cancel, layer.rgba.ctypes.data, layer.count.ctypes.data,
                                  C.byref(fin), C.byref(st)))
    elif h is None:
        _chk(L.pbrhip_render_rays_device(None, C.byref(desc), ptr, planes, int(camera_draws), None, cancel, None, None, None, None))
    else:  # device rays into a host layer: through a device layer of the call's own
        out = DeviceRays((5 * height * width + 7) // 8, scene.device)  # rgba (16 B) + count (4 B) per pixel, in units of 32 bytes
        try:
            d_rgba, d_count = out.ptr, out.ptr + 16 * height * width
            if desc.flags & RENDER_NO_CLEAR:
                DeviceRays._hip(L.hipMemcpy(C.c_void_p(d_rgba), C.c_void_p(layer.rgba.ctypes.data), C.c_size_t(layer.rgba.nbytes), 1), "hipMemcpy")
                DeviceRays._hip(L.hipMemcpy(C.c_void_p(d_count), C.c_void_p(layer.count.ctypes.data), C.c_size_t(layer.count.nbytes), 1), "hipMemcpy")
            _chk(L.pbrhip_render_rays_device(h, C.byref(desc), ptr, planes, int(camera_draws), _device_stream(stream, rays), cancel,
                                             C.c_void_p(d_rgba), C.c_void_p(d_count), C.byref(fin), C.byref(st)))
            DeviceRays._hip(L.hipMemcpy(C.c_void_p(layer.rgba.ctypes.data), C.c_void_p(d_rgba), C.c_size_t(layer.rgba.nbytes), 2), "hipMemcpy")
            DeviceRays._hip(L.hipMemcpy(C.c_void_p(layer.count.ctypes.data), C.c_void_p(d_count), C.c_size_t(layer.count.nbytes), 2), "hipMemcpy")
        finally:
            out.close()
    layer.stats = st.as_dict()
    return layer


def RenderFeaturesRays(scene, rays, num_sample, layer=None, *, device_out=None, stream=None, first_pass=0, seed_seq=1234567890,
                       tile_rank=0, tile_world=1, max_paths_in_flight=0, shard_block=0, no_clear=False):
    """pbrhip_render_features_rays_device: RenderFeatures over the rays RenderRays takes (the first hit of each ray inside its tmin and
    tmax; an inactive ray is a miss).  Host rays are uploaded and the FeatureLayer downloaded through buffers of the call's own.
    device_out: (albedo_ptr, normal_depth_ptr, count_ptr) DEVICE pointers (0 / None = not wanted) instead of a layer, with device rays."""
    where, ptr, (planes, height, width), keep = _ray_source(rays, scene, num_sample)
    if where == "host" and device_out is not None:
        raise ValueError("device_out needs rays in device memory")
    L = _lib.lib()
    desc = RenderDesc(width, height, num_sample, first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight,
                      RENDER_NO_CLEAR if no_clear else 0, 0, 0, shard_block)
    h = scene.h if scene is not None else None
    if device_out is not None:
        _chk(L.pbrhip_render_features_rays_device(h, C.byref(desc), ptr, planes, _device_stream(stream, rays),
                                                  *[C.c_void_p(p or None) for p in device_out]))
        return None
    if h is None:
        _chk(L.pbrhip_render_features_rays_device(None, C.byref(desc), ptr, planes, None, None, None, None))
    if layer is None:
        layer = FeatureLayer()
    if not no_clear or (layer.width, layer.height) != (width, height):
        layer.Resize(width, height)
    npx = height * width
    own = DeviceRays((planes, height, width), scene.device).upload(keep) if where == "host" else None
    out = DeviceRays((9 * npx + 7) // 8, scene.device)  # albedo, normal_depth (16 B each) + count (4 B) per pixel, in units of 32 bytes
    try:
        ptrs = (out.ptr, out.ptr + 16 * npx, out.ptr + 32 * npx)
        arrays = (layer.albedo, layer.normal_depth, layer.count)
        if no_clear:
            for p, a in zip(ptrs, arrays):
                DeviceRays._hip(L.hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1), "hipMemcpy")
        _chk(L.pbrhip_render_features_rays_device(h, C.byref(desc), own.ptr if own else ptr, planes, None if own else _device_stream(stream, rays),
                                                  *[C.c_void_p(p) for p in ptrs]))
        for p, a in zip(ptrs, arrays):
            DeviceRays._hip(L.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), C.c_size_t(a.nbytes), 2), "hipMemcpy")
    finally:
        out.close()
        if own:
            own.close()
    return layer


def RenderProjection(scene, projection, width, height, num_sample, layer=None, param=0.0, *, rays=None, **kw):
    """A frame through one of Scene.ProjectionRays' projections ("latlong", "fisheye", "ortho"; the frame is SetCamera's): in chunks of
    passes whose rays fit RAY_BUFFER_BYTES (256 MiB; at least one pass), ProjectionRays then RenderRays(first_pass=..., flags |=
    RENDER_NO_CLEAR) per chunk -- the result does not depend on the chunking.  The ray buffer is a DeviceRays of the call's own, or
    `rays`: a float32 tensor of at least chunk x H x W x 8 elements on the scene's device (torch is not imported otherwise).  kw:
    RenderRays' keywords.  Returns the layer (or the last chunk's stats with device_out)."""
    width, height, num_sample = int(width), int(height), int(num_sample)
    if width <= 0 or height <= 0:
        raise ValueError("empty image")
    first_pass, flags = int(kw.pop("first_pass", 0)), int(kw.pop("flags", 0))
    seed_seq = kw.get("seed_seq", 1234567890)
    chunk = max(1, min(max(num_sample, 1), RAY_BUFFER_BYTES // (RAY_DT.itemsize * width * height)))
    if rays is not None:
        if not hasattr(rays, "data_ptr") or not str(getattr(rays, "dtype", "")).endswith("float32") or not rays.is_contiguous():
            raise TypeError("rays: a contiguous float32 tensor on the scene's device")
        chunk = min(chunk, int(rays.numel()) // (8 * width * height))
        if chunk < 1:
            raise ValueError("rays: room for at least one pass of H x W x 8 floats")
    if kw.get("device_out") is None:
        if layer is None:
            layer = RenderLayer()
        if not (flags & RENDER_NO_CLEAR) or (layer.width, layer.height) != (width, height):
            layer.Resize(width, height)
    own = None
    out = None
    try:
        done = 0
        while done < num_sample:
            n = min(chunk, num_sample - done)
            if rays is not None:
                buf = rays.view(-1)[:n * height * width * 8].view(n, height, width, 8)
                scene.ProjectionRays(projection, width, height, first_pass + done, n, param, out=buf, seed_seq=seed_seq, stream=kw.get("stream"))
            else:
                if own is None or own.shape[0] != n:
                    if own is not None:
                        own.close()
                    own = DeviceRays((n, height, width), scene.device)
                buf = scene.ProjectionRays(projection, width, height, first_pass + done, n, param, out=own, seed_seq=seed_seq, stream=kw.get("stream"))
            # (every chunk but a clearing call's first accumulates on top)
            out = RenderRays(scene, buf, n, layer, camera_draws=2, first_pass=first_pass + done,
                             flags=flags | (RENDER_NO_CLEAR if done else 0), **kw)
            done += n
    finally:
        if own is not None:
            own.close()
    return out if out is not None else layer


def _denoise_args(iterations, sigma_color, sigma_depth, normal_squarings, albedo):
    return (int(iterations), float(DENOISE_SIGMA_COLOR if sigma_color is None else sigma_color),
            float(DENOISE_SIGMA_DEPTH if sigma_depth is None else sigma_depth), int(normal_squarings), 0 if albedo else DENOISE_NO_ALBEDO)


def Denoise(layer, features=None, *, iterations=0, sigma_color=None, sigma_depth=None, normal_squarings=DENOISE_NORMAL_SQUARINGS,
            albedo=True, device=None):
    """pbrhip_denoise: the edge-avoiding A-trous filter of a RenderLayer guided by a FeatureLayer (None: by colour alone) -> (H, W, 4)
    float32, the denoised mean colour | 1.  iterations 0 = 5; a sigma of None = the library's default, <= 0 = that weight off."""
    h, w = layer.count.shape
    if features is not None and features.count.shape != (h, w):
        raise ValueError("features and layer differ in size")
    rgba, count = np.ascontiguousarray(layer.rgba, np.float32), np.ascontiguousarray(layer.count, np.uint32)
    f = (None, None, None)
    if features is not None:
        f = (np.ascontiguousarray(features.albedo, np.float32), np.ascontiguousarray(features.normal_depth, np.float32),
             np.ascontiguousarray(features.count, np.uint32))
    out = np.zeros((h, w, 4), np.float32)
    _chk(_lib.lib().pbrhip_denoise(_device if device is None else int(device), w, h, rgba.ctypes.data, count.ctypes.data,
                                   *[None if a is None else a.ctypes.data for a in f],
                                   *_denoise_args(iterations, sigma_color, sigma_depth, normal_squarings, albedo), out.ctypes.data))
    return out


def DenoiseDevice(device, width, height, rgba_ptr, count_ptr, out_ptr, features=None, *, iterations=0, sigma_color=None, sigma_depth=None,
                  normal_squarings=DENOISE_NORMAL_SQUARINGS, albedo=True):
    """pbrhip_denoise_device: the same on DEVICE pointers (ints) of `device`; features = (albedo_ptr, normal_depth_ptr, count_ptr) or None."""
    f = (None, None, None) if features is None else tuple(features)
    _chk(_lib.lib().pbrhip_denoise_device(int(device), width, height, rgba_ptr, count_ptr, *f,
                                          *_denoise_args(iterations, sigma_color, sigma_depth, normal_squarings, albedo), out_ptr))


# pbrhip_temporal_accumulate's defaults (include/pbrhip.h PBRHIP_TEMPORAL_*)
TEMPORAL_ALPHA_MIN, TEMPORAL_SIGMA_DEPTH, TEMPORAL_NORMAL_COS_MIN, TEMPORAL_MAX_HISTORY = 0.2, 0.05, 0.9, 32
NONE = 0xFFFFFFFF  # PBRHIP_NONE: MotionLayer.ident's slot of a miss


class MotionLayer:
    """pbrhip_render_motion's buffers: motion (H, W, 4) float32 = mx, my, z_prev, valid (0 none, 1 triangle, 2 curve),
    guide (H, W, 4) float32 = viewer-facing shading normal (a curve's tangent as it is) | t, ident (H, W, 4) uint32 = slot (NONE: a
    miss), bits of u, v, t.  Each is a numpy array, or a tensor on the scene's GPU when RenderMotion wrote into the caller's."""

    def __init__(self, motion, guide, ident):
        self.motion, self.guide, self.ident = motion, guide, ident


class TemporalHistory:
    """What TemporalAccumulate returns and takes back with the next frame: rgba (H, W, 4) = the accumulated mean | the history length,
    guide = the guide of the frame it was made for (numpy arrays, or tensors on one GPU)."""

    def __init__(self, rgba, guide):
        self.rgba, self.guide = rgba, guide

    def layer(self):
        """The RenderLayer Denoise takes for the accumulated frame: rgba = mean | 1, count = 1 (0 where the history holds nothing);
        Accumulate -> Denoise is the chain.  Downloads a tensor history."""
        rgba = np.array(self.rgba.cpu().numpy() if hasattr(self.rgba, "data_ptr") else self.rgba, np.float32)
        out = RenderLayer(rgba.shape[1], rgba.shape[0])
        out.count[...] = rgba[..., 3] > 0
        out.rgba[...] = rgba
        out.rgba[..., 3] = out.count
        return out


def _image_arg(a, shape, dtype, what, device=None):
    """An image argument of the temporal calls -> (pointer, is_device, keep-alive): None, a numpy array, or a contiguous tensor of that
    shape and dtype in GPU memory (on `device` when that is known).  TypeError / ValueError here, before any C call."""
    if a is None:
        return None, False, None
    if hasattr(a, "data_ptr"):
        if not str(getattr(a, "dtype", "")).endswith(dtype):
            raise TypeError(f"{what} must be {dtype}, not {getattr(a, 'dtype', None)}")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{what} must have the shape {tuple(shape)}, not {tuple(a.shape)}")
        if not a.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        dev = getattr(a, "device", None)
        if getattr(dev, "type", None) != "cuda":
            raise ValueError(f"{what} must be in GPU memory, not on {dev}")
        if device is not None and dev.index is not None and dev.index != device:
            raise ValueError(f"{what} is on device {dev.index}, not on device {device}")
        return int(a.data_ptr()), True, a
    keep = np.ascontiguousarray(a, dtype)
    if keep.shape != tuple(shape):
        raise ValueError(f"{what} must have the shape {tuple(shape)}, not {keep.shape}")
    return keep.ctypes.data, False, keep


def RenderMotion(scene, width, height, *, tile_rank=0, tile_world=1, shard_block=0, device_out=None):
    """pbrhip_render_motion: per pixel where the point the current camera's centre ray sees was at Scene.SnapshotPose()
    -> MotionLayer of numpy arrays.  device_out: optional (motion, guide, ident) -- float32, float32, int32 / uint32 (H, W, 4) tensors on
    the scene's GPU, or DEVICE pointers (ints); None / 0 = not wanted -- written in place; the MotionLayer then holds them as given."""
    L = _lib.lib()
    desc = RenderDesc(width, height, 1, 0, 0, tile_rank, tile_world, 0, 0, 0, 0, shard_block)
    shape = (int(height), int(width), 4)
    if device_out is not None:
        if len(device_out) != 3:
            raise TypeError("device_out: (motion, guide, ident)")
        ptrs = []
        for a, dt, what in zip(device_out, ("float32", "float32", "int32"), ("motion", "guide", "ident")):
            if a is None or isinstance(a, int):
                ptrs.append(a or None)
            else:
                ptrs.append(_image_arg(a, shape, dt, f"device_out's {what}", getattr(scene, "device", None))[0])
        _chk(L.pbrhip_render_motion_device(scene.h, C.byref(desc), *[C.c_void_p(p) for p in ptrs]))
        return MotionLayer(*device_out)
    out = MotionLayer(np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.uint32))
    _chk(L.pbrhip_render_motion(scene.h, C.byref(desc), out.motion.ctypes.data, out.guide.ctypes.data, out.ident.ctypes.data))
    return out


def TemporalAccumulate(layer, motion_layer, history=None, *, alpha_min=TEMPORAL_ALPHA_MIN, sigma_depth=TEMPORAL_SIGMA_DEPTH,
                       normal_cos_min=TEMPORAL_NORMAL_COS_MIN, max_history=TEMPORAL_MAX_HISTORY, device=None):
    """pbrhip_temporal_accumulate: the RenderLayer of the current frame (anything with .rgba sums and .count) blended into
    `history` (a TemporalHistory of the previous frame; None: none) where its MotionLayer says the history shows the same surface ->
    the new TemporalHistory.  With numpy arrays everything travels through the host; when layer.rgba is a tensor, every buffer has to be
    a tensor on that GPU (layer.count int32 / uint32) and the result is made of tensors too (torch is then the caller's)."""
    on_gpu = hasattr(layer.rgba, "data_ptr")
    h, w = (int(n) for n in tuple(layer.count.shape))
    dev = (layer.rgba.device.index or 0) if on_gpu else (_device if device is None else int(device))
    img, cnt = (h, w, 4), (h, w)
    args = [_image_arg(layer.rgba, img, "float32", "layer.rgba", dev if on_gpu else None),
            _image_arg(layer.count, cnt, "int32" if on_gpu else "uint32", "layer.count", dev if on_gpu else None),
            _image_arg(motion_layer.motion, img, "float32", "motion", dev if on_gpu else None),
            _image_arg(motion_layer.guide, img, "float32", "guide", dev if on_gpu else None),
            _image_arg(None if history is None else history.rgba, img, "float32", "history.rgba", dev if on_gpu else None),
            _image_arg(None if history is None else history.guide, img, "float32", "history.guide", dev if on_gpu else None)]
    if any(d != on_gpu for p, d, _ in args if p is not None):
        raise TypeError("TemporalAccumulate: the buffers are either all numpy arrays or all tensors on one GPU")
    params = (C.c_float(alpha_min), C.c_float(sigma_depth), C.c_float(normal_cos_min), C.c_uint32(int(max_history)))
    if on_gpu:
        import torch
        out = torch.empty_like(layer.rgba)
        torch.cuda.current_stream(layer.rgba.device).synchronize()  # (the library works on the device's null stream)
        _chk(_lib.lib().pbrhip_temporal_accumulate_device(dev, w, h, *[p for p, _, _ in args], *params, int(out.data_ptr())))
    else:
        out = np.zeros(img, np.float32)
        _chk(_lib.lib().pbrhip_temporal_accumulate(dev, w, h, *[p for p, _, _ in args], *params, out.ctypes.data))
    return TemporalHistory(out, motion_layer.guide)


# pbrhip_svgf_*'s defaults (include/pbrhip.h PBRHIP_SVGF_*)
SVGF_ALPHA_MIN, SVGF_ITERATIONS, SVGF_SIGMA_LUM, SVGF_LUM_EPS = 0.2, 5, 1.0, 1e-4


class SvgfHistory:
    """What SvgfAccumulate returns and takes back with the next frame: illum (H, W, 4) = the accumulated albedo-free
    illumination | the history length, var (H, W) = the variance of its luminance, guide = the guide and ids = the object ids (or None)
    of the frame it was made for.  Numpy arrays, or tensors on one GPU."""

    def __init__(self, illum, var, guide, ids=None):
        self.illum, self.var, self.guide, self.ids = illum, var, guide, ids


def _svgf_features(features, img, cnt, on_gpu, dev):
    """(albedo_hits, feature_count) of a FeatureLayer (anything with .albedo and .count), or two Nones"""
    if features is None:
        return [_image_arg(None, img, "float32", ""), _image_arg(None, cnt, "uint32", "")]
    return [_image_arg(features.albedo, img, "float32", "features.albedo", dev if on_gpu else None),
            _image_arg(features.count, cnt, "int32" if on_gpu else "uint32", "features.count", dev if on_gpu else None)]


def SvgfAccumulate(layer, motion_layer, history=None, features=None, ids=None, *, alpha_min=SVGF_ALPHA_MIN, sigma_depth=TEMPORAL_SIGMA_DEPTH,
                   normal_cos_min=TEMPORAL_NORMAL_COS_MIN, max_history=TEMPORAL_MAX_HISTORY, device=None):
    """pbrhip_svgf_accumulate: TemporalAccumulate on colour / albedo (`features`: a FeatureLayer of the frame, None: albedo
    1) that also rejects history of another object (`ids`: Scene.ObjectIds of the frame, None: no such test; a history made without ids
    is then taken without the test) and carries the variance of the luminance -> the new SvgfHistory.  With an emitter of black albedo in
    view pass no features, here and to SvgfFilter (include/pbrhip.h says why) -- or what SplitEmission makes of the layer and the features.
    Numpy arrays or tensors exactly
    as TemporalAccumulate takes them (ids, counts: int32 tensors)."""
    on_gpu = hasattr(layer.rgba, "data_ptr")
    h, w = (int(n) for n in tuple(layer.count.shape))
    dev = (layer.rgba.device.index or 0) if on_gpu else (_device if device is None else int(device))
    img, cnt, gd, it = (h, w, 4), (h, w), dev if on_gpu else None, "int32" if on_gpu else "uint32"
    with_ids = ids is not None and (history is None or history.ids is not None)
    args = ([_image_arg(layer.rgba, img, "float32", "layer.rgba", gd), _image_arg(layer.count, cnt, it, "layer.count", gd)]
            + _svgf_features(features, img, cnt, on_gpu, dev)
            + [_image_arg(motion_layer.motion, img, "float32", "motion", gd), _image_arg(motion_layer.guide, img, "float32", "guide", gd),
               _image_arg(ids if with_ids else None, cnt, it, "ids", gd),
               _image_arg(None if history is None else history.illum, img, "float32", "history.illum", gd),
               _image_arg(None if history is None else history.var, cnt, "float32", "history.var", gd),
               _image_arg(None if history is None else history.guide, img, "float32", "history.guide", gd),
               _image_arg(history.ids if with_ids and history is not None else None, cnt, it, "history.ids", gd)])
    if any(d != on_gpu for p, d, _ in args if p is not None):
        raise TypeError("SvgfAccumulate: the buffers are either all numpy arrays or all tensors on one GPU")
    params = (C.c_float(alpha_min), C.c_float(sigma_depth), C.c_float(normal_cos_min), C.c_uint32(int(max_history)))
    if on_gpu:
        import torch
        out, var = torch.empty_like(layer.rgba), torch.empty((h, w), dtype=torch.float32, device=layer.rgba.device)
        torch.cuda.current_stream(layer.rgba.device).synchronize()  # (the library works on the device's null stream)
        _chk(_lib.lib().pbrhip_svgf_accumulate_device(dev, w, h, *[p for p, _, _ in args], *params, int(out.data_ptr()), int(var.data_ptr())))
    else:
        out, var = np.zeros(img, np.float32), np.zeros(cnt, np.float32)
        _chk(_lib.lib().pbrhip_svgf_accumulate(dev, w, h, *[p for p, _, _ in args], *params, out.ctypes.data, var.ctypes.data))
    return SvgfHistory(out, var, motion_layer.guide, ids)


def SvgfFilter(history, features=None, *, iterations=0, sigma_lum=None, sigma_depth=None, normal_squarings=DENOISE_NORMAL_SQUARINGS,
               use_ids=True, feedback=False, device=None):
    """pbrhip_svgf_filter: the variance-guided A-trous filter of an SvgfHistory, the albedo of `features` multiplied back
    -> (H, W, 4) float32, colour | 1; with feedback=True -> (image, SvgfHistory) where the history's illum is the illumination after the
    first iteration: hand it to the next SvgfAccumulate in the place of `history`.  iterations 0 = 5; a sigma of None = the library's
    default, <= 0 = that weight off; use_ids=False filters across objects although the history has ids."""
    on_gpu = hasattr(history.illum, "data_ptr")
    h, w = (int(n) for n in tuple(history.illum.shape)[:2])
    dev = (history.illum.device.index or 0) if on_gpu else (_device if device is None else int(device))
    img, cnt, gd, it = (h, w, 4), (h, w), dev if on_gpu else None, "int32" if on_gpu else "uint32"
    args = ([_image_arg(history.illum, img, "float32", "history.illum", gd), _image_arg(history.var, cnt, "float32", "history.var", gd),
             _image_arg(history.guide, img, "float32", "history.guide", gd), _image_arg(history.ids if use_ids else None, cnt, it, "history.ids", gd)]
            + _svgf_features(features, img, cnt, on_gpu, dev))
    if any(d != on_gpu for p, d, _ in args if p is not None):
        raise TypeError("SvgfFilter: the buffers are either all numpy arrays or all tensors on one GPU")
    params = (int(iterations), C.c_float(SVGF_SIGMA_LUM if sigma_lum is None else sigma_lum),
              C.c_float(DENOISE_SIGMA_DEPTH if sigma_depth is None else sigma_depth), int(normal_squarings))
    if on_gpu:
        import torch
        out = torch.empty_like(history.illum)
        fb = torch.empty_like(history.illum) if feedback else None
        torch.cuda.current_stream(history.illum.device).synchronize()  # (the library works on the device's null stream)
        _chk(_lib.lib().pbrhip_svgf_filter_device(dev, w, h, *[p for p, _, _ in args], *params, int(out.data_ptr()),
                                                  None if fb is None else int(fb.data_ptr())))
    else:
        out = np.zeros(img, np.float32)
        fb = np.zeros(img, np.float32) if feedback else None
        _chk(_lib.lib().pbrhip_svgf_filter(dev, w, h, *[p for p, _, _ in args], *params, out.ctypes.data, None if fb is None else fb.ctypes.data))
    return (out, SvgfHistory(fb, history.var, history.guide, history.ids)) if feedback else out


class EmissionLayer:
    """The first-hit emission layer (pbrhip_render_features_emission): emission (H, W, 4) float32 = the sum of what the
    renderer adds to a sample's radiance at depth 0 (an area light seen from its front, or the environment behind a miss) | the number
    of samples that added one.  A numpy array, or a tensor on one GPU when the caller made it."""

    def __init__(self, w=0, h=0):
        self.Resize(w, h)

    def Resize(self, w, h):
        self.width, self.height = int(w), int(h)
        self.emission = np.zeros((self.height, self.width, 4), np.float32)

    def Clear(self):
        self.emission[...] = 0


def RenderFeaturesEmission(scene, width, height, num_sample, layer=None, emission=None, *, first_pass=0, seed_seq=1234567890, tile_rank=0,
                           tile_world=1, max_paths_in_flight=0, shard_block=0, no_clear=False, device_out=None):
    """pbrhip_render_features_emission: RenderFeatures -- the same buffers, bit for bit, from the same keywords -- and the
    EmissionLayer of the same samples, in one trace -> (FeatureLayer, EmissionLayer).  device_out: optional (albedo_ptr,
    normal_depth_ptr, count_ptr, emission_ptr) DEVICE pointers (ints, 0 / None = not wanted) instead of the layers."""
    L = _lib.lib()
    desc = RenderDesc(width, height, num_sample, first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight,
                      RENDER_NO_CLEAR if no_clear else 0, 0, 0, shard_block)
    if device_out is not None:
        if len(device_out) != 4:
            raise TypeError("device_out: (albedo, normal_depth, count, emission)")
        _chk(L.pbrhip_render_features_emission_device(scene.h, C.byref(desc), *[C.c_void_p(p or None) for p in device_out]))
        return None
    if layer is None:
        layer = FeatureLayer()
    if emission is None:
        emission = EmissionLayer()
    if not no_clear or (layer.width, layer.height) != (width, height):
        layer.Resize(width, height)
    if not no_clear or (emission.width, emission.height) != (width, height):
        emission.Resize(width, height)
    _chk(L.pbrhip_render_features_emission(scene.h, C.byref(desc), layer.albedo.ctypes.data, layer.normal_depth.ctypes.data,
                                           layer.count.ctypes.data, emission.emission.ctypes.data))
    return layer, emission


def _bare(cls, **fields):
    """an instance of a layer class around buffers that exist already (numpy arrays or tensors)"""
    out = cls.__new__(cls)
    out.__dict__.update(fields)
    return out


def SplitEmission(layer, emission, features=None, *, device=None):
    """pbrhip_emission_split: the RenderLayer's sums without the directly seen emission (clamped at 0), and the
    FeatureLayer with a miss counted as black albedo (hits := samples) -> (RenderLayer, FeatureLayer or None): what SvgfAccumulate,
    SvgfFilter and Denoise take in the place of the originals; MergeEmission adds the emission back to their result.  `emission`: an
    EmissionLayer or its array.  Numpy arrays or tensors exactly as SvgfAccumulate takes them; the inputs are left as they are."""
    em = getattr(emission, "emission", emission)
    on_gpu = hasattr(layer.rgba, "data_ptr")
    h, w = (int(n) for n in tuple(layer.count.shape))
    dev = (layer.rgba.device.index or 0) if on_gpu else (_device if device is None else int(device))
    img, cnt, gd, it = (h, w, 4), (h, w), dev if on_gpu else None, "int32" if on_gpu else "uint32"
    args = ([_image_arg(layer.rgba, img, "float32", "layer.rgba", gd), _image_arg(layer.count, cnt, it, "layer.count", gd),
             _image_arg(em, img, "float32", "emission", gd)] + _svgf_features(features, img, cnt, on_gpu, dev))
    if any(d != on_gpu for p, d, _ in args if p is not None):
        raise TypeError("SplitEmission: the buffers are either all numpy arrays or all tensors on one GPU")
    ptrs = [p for p, _, _ in args]
    if on_gpu:
        import torch
        out = torch.empty_like(layer.rgba)
        alb = None if features is None else torch.empty_like(features.albedo)
        torch.cuda.current_stream(layer.rgba.device).synchronize()  # (the library works on the device's null stream)
        _chk(_lib.lib().pbrhip_emission_split_device(dev, w, h, *ptrs, int(out.data_ptr()), None if alb is None else int(alb.data_ptr())))
    else:
        out = np.zeros(img, np.float32)
        alb = None if features is None else np.zeros(img, np.float32)
        _chk(_lib.lib().pbrhip_emission_split(dev, w, h, *ptrs, out.ctypes.data, None if alb is None else alb.ctypes.data))
    split = _bare(RenderLayer, width=w, height=h, rgba=out, count=layer.count)
    if features is None:
        return split, None
    return split, _bare(FeatureLayer, width=w, height=h, albedo=alb, normal_depth=features.normal_depth, count=features.count)


def MergeEmission(rgba, emission, count, *, device=None):
    """pbrhip_emission_merge: a filtered image of the split layer (H, W, 4) + the mean of the emission layer over `count`
    samples (the RenderLayer's count) -> (H, W, 4) float32, the alpha as it came.  Numpy arrays, or tensors on one GPU."""
    em = getattr(emission, "emission", emission)
    on_gpu = hasattr(rgba, "data_ptr")
    h, w = (int(n) for n in tuple(rgba.shape)[:2])
    dev = (rgba.device.index or 0) if on_gpu else (_device if device is None else int(device))
    img, cnt, gd = (h, w, 4), (h, w), dev if on_gpu else None
    args = [_image_arg(rgba, img, "float32", "rgba", gd), _image_arg(em, img, "float32", "emission", gd),
            _image_arg(count, cnt, "int32" if on_gpu else "uint32", "count", gd)]
    if any(d != on_gpu for p, d, _ in args):
        raise TypeError("MergeEmission: the buffers are either all numpy arrays or all tensors on one GPU")
    ptrs = [p for p, _, _ in args]
    if on_gpu:
        import torch
        out = torch.empty_like(rgba)
        torch.cuda.current_stream(rgba.device).synchronize()  # (the library works on the device's null stream)
        _chk(_lib.lib().pbrhip_emission_merge_device(dev, w, h, *ptrs, int(out.data_ptr())))
    else:
        out = np.zeros(img, np.float32)
        _chk(_lib.lib().pbrhip_emission_merge(dev, w, h, *ptrs, out.ctypes.data))
    return out


# pbrhip_render_adaptive's defaults (include/pbrhip.h PBRHIP_ADAPTIVE_*)
ADAPTIVE_FIRST_LEVEL, ADAPTIVE_THRESHOLD, ADAPTIVE_TILE = 8, 0.07, 8


def RenderAdaptive(scene, width, height, max_sample, threshold=ADAPTIVE_THRESHOLD, first_level=0, layer=None, cancel_render_flag=None,
                   finish_pass=None, device_out=None, **desc_kw):
    """pbrhip_render_adaptive: Render with a sample count per 8x8 tile -- tiles whose error estimate has fallen to
    `threshold` stop, the rest render on up to `max_sample` passes.  Pixel p of the layer holds, bit for bit, what Render with
    num_sample = layer.count[p] holds at p.  first_level 0 = 8; desc_kw: Render's keywords (first_pass, seed_seq, tile_rank, tile_world,
    max_paths_in_flight, num_streams, tail_paths, shard_block -- a multiple of 8 --, flags).  Returns the layer (resized and cleared)
    with .tile_error (ceil(H / 8), ceil(W / 8)) float32, .samples and .rounds attached.
    device_out: optional (rgba_ptr, count_ptr, tile_error_ptr or None) DEVICE pointers (ints) instead of a layer; returns
    (samples, rounds)."""
    L = _lib.lib()
    desc = _desc(width, height, max_sample, **desc_kw)
    fin = finish_pass if finish_pass is not None else C.c_size_t(0)
    cancel = C.byref(cancel_render_flag) if cancel_render_flag is not None else None
    samples, rounds = C.c_uint64(0), C.c_uint32(0)
    if device_out is not None:
        _chk(L.pbrhip_render_adaptive_device(scene.h if scene is not None else None, C.byref(desc), float(threshold), int(first_level), cancel,
                                             *[C.c_void_p(p or None) for p in device_out], C.byref(fin), C.byref(samples), C.byref(rounds)))
        return samples.value, rounds.value
    if layer is None:
        layer = RenderLayer()
    layer.Resize(width, height)
    tile_error = np.zeros((-(-int(height) // ADAPTIVE_TILE), -(-int(width) // ADAPTIVE_TILE)), np.float32)
    _chk(L.pbrhip_render_adaptive(scene.h if scene is not None else None, C.byref(desc), float(threshold), int(first_level), cancel,
                                  layer.rgba.ctypes.data, layer.count.ctypes.data, tile_error.ctypes.data, C.byref(fin), C.byref(samples),
                                  C.byref(rounds)))
    layer.tile_error, layer.samples, layer.rounds = tile_error, samples.value, rounds.value
    return layer


def adaptive_step(rgba, snapshot, n_prev, n_now, threshold, tiles_in, tile_error=None, device=None):
    """pbrhip_adaptive_step, a test hook: one decision step of RenderAdaptive on given layers.  rgba (H, W, 4) = the layer at level n_now,
    snapshot (H, W, 4) = the layer at level n_prev, tiles_in = the active tile ids.  Returns (tiles_out, pixels_out, tile_error,
    new_snapshot): the tiles that stay active in the order they had, their pixels, the tiles' error (entries of other tiles as given,
    0 without tile_error) and the snapshot after the step."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    snap = np.array(snapshot, np.float32, order="C", copy=True).reshape(h, w, 4)
    tiles_in = np.ascontiguousarray(tiles_in, np.uint32).reshape(-1)
    th, tw = -(-h // ADAPTIVE_TILE), -(-w // ADAPTIVE_TILE)
    err = np.zeros((th, tw), np.float32) if tile_error is None else np.array(tile_error, np.float32, order="C", copy=True).reshape(th, tw)
    tiles_out, pixels_out = np.zeros(max(len(tiles_in), 1), np.uint32), np.zeros(h * w, np.uint32)
    nt, npx = C.c_uint32(0), C.c_uint32(0)
    _chk(_lib.lib().pbrhip_adaptive_step(_device if device is None else int(device), w, h, rgba.ctypes.data, snap.ctypes.data, int(n_prev),
                                         int(n_now), float(threshold), tiles_in.ctypes.data, len(tiles_in), tiles_out.ctypes.data,
                                         C.byref(nt), pixels_out.ctypes.data, C.byref(npx), err.ctypes.data))
    return tiles_out[:nt.value].copy(), pixels_out[:npx.value].copy(), err, snap


def _desc(width, height, num_sample, first_pass=0, seed_seq=1234567890, tile_rank=0, tile_world=1,
          max_paths_in_flight=0, flags=0, num_streams=0, tail_paths=0, shard_block=0):
    return RenderDesc(width, height, num_sample, first_pass, seed_seq, tile_rank, tile_world, max_paths_in_flight,
                      flags, num_streams, tail_paths, shard_block)


def replicate(scene, device):
    """pbrhip_scene_replicate: a committed scene's copy on `device` (device-to-device, no second BVH build)."""
    out = Scene.__new__(Scene)
    out.L = _lib.lib()
    h = C.c_void_p()
    _chk(out.L.pbrhip_scene_replicate(scene.h, int(device), C.byref(h)))
    out.h = h
    out.device = int(device)
    return out


def RenderMulti(scenes, width, height, num_sample, cancel_render_flag=None, layer=None, finish_pass=None, **kw):
    """pbrhip_render_multi: one frame over several devices of this process (scenes[i] = the scene on device i);
    returns (True, [stats per device])."""
    L = _lib.lib()
    desc = _desc(width, height, num_sample, **kw)
    n = len(scenes)
    hs = (C.c_void_p * n)(*[s.h for s in scenes])
    st = (RenderStats * n)()
    fin = finish_pass if finish_pass is not None else C.c_size_t(0)
    cancel = C.byref(cancel_render_flag) if cancel_render_flag is not None else None
    if not (desc.flags & RENDER_NO_CLEAR):
        layer.Resize(width, height)
    _chk(L.pbrhip_render_multi(hs, n, C.byref(desc), cancel, _ptr(layer.rgba), _ptr(layer.count, u32p), C.byref(fin), st))
    return True, [x.as_dict() for x in st]


class Comm:
    """pbrhip_comm: the library's RCCL communicator for one-process-per-GPU jobs.  `unique_id()` on one rank, hand the
    bytes to every rank (e.g. torch.distributed.broadcast_object_list), then Comm(id, rank, world) on every rank."""

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        _chk(_lib.lib().pbrhip_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid, rank, world):
        self.L = _lib.lib()
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        buf = (C.c_ubyte * 128)(*uid)
        _chk(self.L.pbrhip_comm_create(C.byref(h), buf, self.rank, self.world))
        self.h = h

    def reduce_layer(self, rgba_ptr, count_ptr, num_pixels, root=0):
        _chk(self.L.pbrhip_comm_reduce_layer(self.h, C.c_void_p(rgba_ptr), C.c_void_p(count_ptr), C.c_size_t(num_pixels), int(root)))

    def gather_layer(self, scene, width, height, rgba_ptr, count_ptr, shard_block=0, root=0):
        desc = _desc(width, height, 0, tile_rank=self.rank, tile_world=self.world, shard_block=shard_block)
        _chk(self.L.pbrhip_comm_gather_layer(self.h, scene.h, C.byref(desc), C.c_void_p(rgba_ptr), C.c_void_p(count_ptr), int(root)))

    def close(self):
        if getattr(self, "h", None):
            self.L.pbrhip_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene_from_desc(desc, bvh_builder=BVH_HOST_SAH):
    from . import scenes
    s = Scene()
    if bvh_builder != BVH_HOST_SAH:
        s.SetBvhBuilder(bvh_builder)
    scenes.build_scene(s, desc, make_principled, make_hair)
    return s
