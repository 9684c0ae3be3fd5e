"""The gfx950 code object inside a built libpbrhip.so: the one place that extracts and reads it (no GPU needed).

The budget tests and scripts/ktable.py share it.  `available()` says whether the library and the LLVM tools are there; a test that
needs them skips where it calls this module.  The code object is unbundled once per process and library; `kernel_table()` and
`disassembly()` are read from it once each.  Kernels are named as the source names them: `k_trace<false, false, true, false>`."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "pbrlab_amd", "libpbrhip.so")
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def available(lib=LIB):
    return os.path.exists(lib) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler")) and shutil.which("c++filt") is not None


def waves_per_simd(vgprs):
    """Occupancy class: 512 registers per lane and SIMD, allocated in eights, at most 8 waves."""
    alloc = -(-vgprs // 8) * 8
    return min(8, 512 // alloc)


def _run(*cmd):
    return subprocess.run(list(cmd), check=True, capture_output=True, text=True).stdout


@functools.lru_cache(maxsize=None)
def code_object(lib=LIB):
    """Path of the library's gfx950 code object, unbundled into a temporary directory that lives as long as the process."""
    tmp = tempfile.mkdtemp(prefix="pbrhip_co_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    _run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib)
    _run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
         f"--output={co}")
    return co


def _source_names(mangled):
    demangled = _run("c++filt", *mangled).split("\n")
    return [d.replace("void pb::", "").replace("pb::", "").split("(")[0] for d in demangled[:len(mangled)]]


@functools.lru_cache(maxsize=None)
def kernel_table(lib=LIB):
    """{kernel: {vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size}} from the code object's metadata."""
    notes = _run(os.path.join(LLVM, "llvm-readelf"), "--notes", code_object(lib))
    # a kernel's record lists its keys in alphabetical order: .args (whose entries have a .name of their own), .group_segment_fixed_size,
    # the kernel's .name, then the other three -- so the LDS size is held until the name comes, and only a kernel's record gets a .vgpr_count
    table, cur, lds = {}, {}, 0
    for line in notes.splitlines():
        m = re.match(r"\s+(?:- )?\.(name|" + "|".join(FIELDS) + r"):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "group_segment_fixed_size":
            lds = int(m.group(2))
        elif m.group(1) == "name":
            cur = table[m.group(2)] = {"group_segment_fixed_size": lds}
        else:
            cur[m.group(1)] = int(m.group(2))
    table = {k: v for k, v in table.items() if "vgpr_count" in v}
    return dict(zip(_source_names(list(table)), table.values()))


@functools.lru_cache(maxsize=None)
def disassembly(lib=LIB):
    """{kernel: [instruction lines]} without what depends on where the kernel lies in the code object: the address comment, the
    <symbol+offset> of a branch target, the padding behind the last s_endpgm, and the literal of the s_add_u32 behind an s_getpc_b64
    (the distance to a constant table).  Two builds of one kernel compare equal exactly when their instructions are the same."""
    bodies, cur = {}, None
    for line in _run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", code_object(lib)).splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = bodies.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"<[^>]*>", "<L>", re.sub(r"\s*//.*$", "", line)).strip())
    for v in bodies.values():
        while v and (v[-1] in ("s_nop 0", "...") or v[-1].startswith("s_code_end")):
            v.pop()
        for i in range(1, len(v)):
            if v[i - 1].startswith("s_getpc_b64"):
                v[i] = re.sub(r"0x[0-9a-f]+$", "<PCREL>", v[i])
    return dict(zip(_source_names(list(bodies)), bodies.values()))
