"""ctypes access to oracle/_ref/libref_io.so: the reference's own host I/O code (vendored tinyobjloader, cyhair.cc,
curve-mesh-io.cc, image-io.cc + stb) compiled unmodified by oracle/Makefile.  Test infrastructure only.

Where that library is not built, the loaders and the JPEG writer below answer from tests/golden/io/ref_io_outputs.npz, keyed by
the bytes of their input: the bytes the writer wrote, and for the loaders a digest of what they returned (checked against this
repository's own loader on the same bytes), recorded by tests/golden/make_ref_outputs.py.  An input the file does not hold is an
error, never a skip.  The EXR writer is not stored (save_exr)."""
import ctypes as C
import hashlib
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "oracle", "_ref", "libref_io.so")
_L = None


STORED = os.path.join(ROOT, "tests", "golden", "io", "ref_io_outputs.npz")
RECORD = None   # set by tests/golden/make_ref_outputs.py to the file save_recorded() writes: keep every live answer
_stored = _index = None
_recorded = {}


def available():
    """the live library is built (else the stored answers stand in for it)"""
    return os.path.exists(PATH)


def _key(kind, *parts):
    """content key of one call: the kind of call and the bytes of its inputs (file contents, pixels, parameters)"""
    h = hashlib.sha256(kind.encode())
    for p in parts:
        if isinstance(p, np.ndarray):
            b = str(p.dtype).encode() + str(p.shape).encode() + np.ascontiguousarray(p).tobytes()
        else:
            b = p if isinstance(p, bytes) else repr(p).encode()
        h.update(len(b).to_bytes(8, "little") + b)
    return kind + "." + h.hexdigest()[:32]


def _digest(*arrays):
    """sha256 over the dtypes, shapes and bytes of `arrays`"""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def _unlike(ours, shape, dtype):
    """an array of `shape` whose bits are not those of `ours`: the stand-in for a stored answer that `ours` does not match"""
    udt = np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64
    x = np.full(shape, np.nan, dtype) if np.dtype(dtype).kind == "f" else np.full(shape, np.iinfo(dtype).max, dtype)
    if ours is not None and np.shape(ours) == x.shape and x.size and \
            np.array_equal(np.ascontiguousarray(ours, dtype).view(udt), x.view(udt)):
        x.reshape(-1)[0] = 0
    return x


def _file(path):
    try:
        with open(path, "rb") as f:
            return f.read()
    except OSError:
        return b"<missing>"


def _answer(key, live, stored_form=None):
    """live() -> dict of arrays from the library when it is built -- recorded as stored_form(answer) if RECORD is set --, else
    the stored arrays of `key`"""
    if available():
        out = {k: np.asarray(v) for k, v in live().items()}
        if RECORD:
            _recorded[key] = stored_form(out) if stored_form else out
        return out
    return _stored_answer(key)


def _stored_answer(key):
    global _stored, _index
    if _stored is None:
        z = np.load(STORED)
        _stored = z["blob"].tobytes()
        off = z["offsets"]
        _index = {k: (int(off[i]), int(off[i + 1])) for i, k in enumerate(z["keys"])}
    if key not in _index:
        raise KeyError(f"{key}: the reference's answer for this input is not in {STORED} (tests/golden/make_ref_outputs.py)")
    a, b = _index[key]
    with np.load(io.BytesIO(_stored[a:b])) as z:
        return {k: z[k] for k in z.files}


def save_recorded():
    """one compressed blob of the recorded answers (one uncompressed .npz each), an index of keys and offsets"""
    keys, parts, offsets = sorted(_recorded), [], [0]
    for k in keys:
        buf = io.BytesIO()
        np.savez(buf, **_recorded[k])
        parts.append(buf.getvalue())
        offsets.append(offsets[-1] + len(parts[-1]))
    np.savez_compressed(RECORD, keys=np.array(keys), offsets=np.array(offsets, np.int64),
                        blob=np.frombuffer(b"".join(parts), np.uint8))
    return len(keys)


def _written(path, live_ok):
    """a writer's answer: its verdict and the bytes of the file it left (replayed into `path`)"""
    return {"ok": np.array([bool(live_ok)]), "data": np.frombuffer(_file(path), np.uint8) if os.path.exists(path) else np.zeros(0, np.uint8),
            "exists": np.array([os.path.exists(path)])}


def _replay_file(path, a):
    if bool(a["exists"][0]) and not available():
        with open(path, "wb") as f:
            f.write(a["data"].tobytes())
    return bool(a["ok"][0])


def lib():
    global _L
    if _L is None:
        L = C.CDLL(PATH)
        for n in ("refio_obj_load", "refio_hair_load", "refio_image_load"):
            getattr(L, n).restype = C.c_void_p
        L.refio_obj_load.argtypes = [C.c_char_p, C.c_char_p]
        L.refio_obj_size.restype = C.c_size_t
        L.refio_obj_size.argtypes = [C.c_void_p, C.c_int]
        L.refio_obj_data.restype = C.c_void_p
        L.refio_obj_data.argtypes = [C.c_void_p, C.c_int]
        L.refio_obj_ok.argtypes = [C.c_void_p]
        L.refio_obj_free.argtypes = [C.c_void_p]
        L.refio_hair_load.argtypes = [C.c_char_p, C.c_int]
        L.refio_hair_ok.argtypes = [C.c_void_p]
        L.refio_hair_size.restype = C.c_size_t
        L.refio_hair_size.argtypes = [C.c_void_p, C.c_int]
        L.refio_hair_data.restype = C.c_void_p
        L.refio_hair_data.argtypes = [C.c_void_p, C.c_int]
        L.refio_hair_free.argtypes = [C.c_void_p]
        L.refio_image_load.argtypes = [C.c_char_p, C.c_char_p]
        L.refio_image_ok.argtypes = [C.c_void_p]
        L.refio_image_dims.argtypes = [C.c_void_p] + [C.POINTER(C.c_size_t)] * 3
        L.refio_image_data.restype = C.c_void_p
        L.refio_image_data.argtypes = [C.c_void_p]
        L.refio_image_free.argtypes = [C.c_void_p]
        L.refio_cli_output.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        L.refio_write_png_u8.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
        L.refio_save_exr.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.refio_write_jpg.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.refio_parse_texopt.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        _L = L
    return _L


def _arr(h, which, dtype, fn_size, fn_data):
    n = fn_size(h, which)
    if n == 0:
        return np.zeros(0, dtype)
    p = fn_data(h, which)
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(p), dtype=dtype).copy()


def obj_load(filename, base_dir):
    """tinyobj::LoadObj as triangle-mesh-io.cc calls it -> dict"""
    text = _file(filename)
    mtls = [tok for line in text.splitlines() if line.strip().startswith(b"mtllib") for tok in line.split()[1:]]
    key = _key("obj", text, *[m + b"=" + _file(os.path.join(base_dir, os.fsdecode(m))) for m in mtls])
    a = _answer(key, lambda: _obj_load_live(filename, base_dir))
    out = {k: v for k, v in a.items() if k != "text"}
    out["ok"], out["text"] = bool(a["ok"][0]), a["text"].tobytes().decode(errors="replace")
    return out


def _obj_load_live(filename, base_dir):
    L = lib()
    h = L.refio_obj_load(os.fsencode(filename), os.fsencode(base_dir))
    try:
        out = {"ok": bool(L.refio_obj_ok(h))}
        for which, (key, dt) in enumerate([("vertices", np.float32), ("normals", np.float32), ("texcoords", np.float32),
                                           ("corners", np.int32), ("shape_first", np.int32), ("material_ids", np.int32)]):
            out[key] = _arr(h, which, dt, L.refio_obj_size, L.refio_obj_data)
        out["ok"], out["text"] = np.array([out["ok"]]), _arr(h, 6, np.uint8, L.refio_obj_size, L.refio_obj_data)
        return out
    finally:
        L.refio_obj_free(h)


def _hair_digest(ok, vertices, indices):
    return _digest(np.array([bool(ok)]), np.asarray(vertices, np.float32), np.asarray(indices).astype(np.int64))


def hair_load(path, memory_saving_mode=False):
    """curve-mesh-io.cc LoadCurveMeshAsCubicBezierCurve -> (ok, vertices (n, 4) f32, indices u32).  Stored as a digest: without the
    library, this repository's loader reads the same bytes, and its answer stands for the reference's only where the digests agree
    (else stand-ins that differ from it bit for bit are returned, so the test's comparison fails as it would against the library)"""
    key = _key("hair", _file(path), bool(memory_saving_mode))
    a = _answer(key, lambda: _hair_load_live(path, memory_saving_mode),
                lambda r: {"ok": r["ok"], "nv": np.array([len(r["vertices"])]), "ni": np.array([len(r["indices"])]),
                           "sha256": _hair_digest(r["ok"][0], r["vertices"], r["indices"])})
    if available():
        return bool(a["ok"][0]), a["vertices"], a["indices"]
    from pbrlab_amd import io_api
    ok, v, i = io_api.LoadCurveMeshAsCubicBezierCurve(path, memory_saving_mode)
    if np.array_equal(_hair_digest(ok, v, i), a["sha256"]):
        return ok, v, i
    return bool(a["ok"][0]), _unlike(v, (int(a["nv"][0]), 4), np.float32), _unlike(i, (int(a["ni"][0]),), np.uint32)


def _hair_load_live(path, memory_saving_mode):
    L = lib()
    h = L.refio_hair_load(os.fsencode(path), int(memory_saving_mode))
    try:
        return {"ok": np.array([bool(L.refio_hair_ok(h))]), "vertices": _arr(h, 0, np.float32, L.refio_hair_size, L.refio_hair_data).reshape(-1, 4),
                "indices": _arr(h, 1, np.uint32, L.refio_hair_size, L.refio_hair_data)}
    finally:
        L.refio_hair_free(h)


def image_load(filename, asset_path=""):
    """image-io.cc LoadImageFromFile -> (h, w, c) float32, or None where it fails.  Stored as the verdict, the shape and a digest of
    the pixels: without the library, this repository's loader reads the same bytes, and its pixels stand for the reference's only
    where the digests agree (else a stand-in of the reference's shape that differs from them bit for bit)"""
    key = _key("image", os.path.basename(filename), _file(os.path.join(asset_path, filename)), _file(filename))
    a = _answer(key, lambda: {"pixels": _image_load_live(filename, asset_path)},
                lambda r: {"ok": np.array([r["pixels"].ndim == 3]), "shape": np.array(r["pixels"].shape, np.int64),
                           "sha256": _digest(np.ascontiguousarray(r["pixels"], np.float32))})
    if available():
        return None if a["pixels"].ndim != 3 else a["pixels"]
    if not a["ok"][0]:
        return None
    from pbrlab_amd import io_api
    try:
        ours = np.ascontiguousarray(io_api.LoadImageFromFile(filename, asset_path), np.float32)
    except io_api.PbrIoError:
        ours = None
    if ours is not None and np.array_equal(_digest(ours), a["sha256"]):
        return ours
    return _unlike(ours, tuple(int(n) for n in a["shape"]), np.float32)


def _image_load_live(filename, asset_path):
    L = lib()
    h = L.refio_image_load(os.fsencode(filename), os.fsencode(asset_path))
    try:
        if not L.refio_image_ok(h):
            return np.zeros(0, np.float32)
        w, hh, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.refio_image_dims(h, C.byref(w), C.byref(hh), C.byref(c))
        n = w.value * hh.value * c.value
        p = L.refio_image_data(h)
        return np.frombuffer((C.c_char * (n * 4)).from_address(p), dtype=np.float32).copy().reshape(hh.value, w.value, c.value)
    finally:
        L.refio_image_free(h)


def cli_output(filename, directory, rgba, count):
    rgba = np.ascontiguousarray(rgba, np.float32)
    count = np.ascontiguousarray(count, np.uint32)
    h, w = count.shape
    return bool(lib().refio_cli_output(os.fsencode(filename), os.fsencode(directory), rgba.ctypes.data, count.ctypes.data, w, h))


def parse_texopt(value):
    name = C.create_string_buffer(1024)
    cs = C.create_string_buffer(256)
    ok = lib().refio_parse_texopt(value.encode(), name, 1024, cs, 256)
    return bool(ok), name.value.decode(), cs.value.decode()


def save_exr(path, planes, names, half=False, compression=3, line_order=0):
    """tinyexr's writer (test-file generator).  planes: (nchan, h, w) float32; names: alphabetical channel names.  Live library only:
    its files are random float planes that do not compress, too large to store (tests/test_io_cpu.py skips its two EXR fuzz tests
    where the library is not built)"""
    planes = np.ascontiguousarray(planes, np.float32)
    nchan, h, w = planes.shape
    assert list(names) == sorted(names)
    blob = b"".join(n.encode() + b"\0" for n in names)
    return bool(lib().refio_save_exr(os.fsencode(path), planes.ctypes.data, blob, nchan, w, h, int(half), compression, line_order))


def save_exr_isolated(path, planes, names, half=False, compression=3, line_order=0):
    """save_exr in a child process: tinyexr's PIZ compressor crashes on some inputs (seen: one FLOAT channel of smooth data,
    38 x 34), which must not take the test run down.  Returns False when the child failed."""
    import pickle
    import subprocess
    import sys
    blob = pickle.dumps((path, np.ascontiguousarray(planes, np.float32), list(names), half, compression, line_order))
    code = ("import pickle, sys; sys.path.insert(0, %r); import _refio; a = pickle.loads(sys.stdin.buffer.read()); "
            "sys.exit(0 if _refio.save_exr(*a) else 1)") % os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", code], input=blob, capture_output=True)
    return r.returncode == 0 and os.path.exists(path)


def write_jpg(path, pixels, quality=90):
    """stb_image_write's JPEG writer (test-file generator).  pixels: (h, w, c) uint8"""
    px = np.ascontiguousarray(pixels, np.uint8)
    h, w, c = px.shape
    return _replay_file(path, _answer(_key("write_jpg", px, quality), lambda: _written(
        path, lib().refio_write_jpg(os.fsencode(path), px.ctypes.data, w, h, c, quality))))
