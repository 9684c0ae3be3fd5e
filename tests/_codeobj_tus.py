"""Every gfx950 code object of libpbrhip.so.  The library links one offload bundle per HIP translation unit into its .hip_fatbin
section; `_codeobj` reads the first (kernels.hip's).  This reads them all, for the kernels of the other translation units
(features.hip, denoise.hip): {kernel: {vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size}}."""
import atexit
import functools
import os
import re
import shutil
import tempfile

import _codeobj as CO

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


@functools.lru_cache(maxsize=None)
def code_objects(lib=CO.LIB):
    tmp = tempfile.mkdtemp(prefix="pbrhip_cos_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    fat = os.path.join(tmp, "fat.bin")
    CO._run(os.path.join(CO.LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for i, at in enumerate(starts):
        piece, co = os.path.join(tmp, f"bundle{i}.bin"), os.path.join(tmp, f"dev{i}.co")
        with open(piece, "wb") as f:
            f.write(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        CO._run(os.path.join(CO.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
        if os.path.getsize(co) > 0:
            out.append(co)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kernel_table(lib=CO.LIB):
    """The union of the kernel tables of the library's code objects (the metadata parse is _codeobj.kernel_table's)."""
    table = {}
    for co in code_objects(lib):
        notes = CO._run(os.path.join(CO.LLVM, "llvm-readelf"), "--notes", co)
        part, cur, lds = {}, {}, 0
        for line in notes.splitlines():
            m = re.match(r"\s+(?:- )?\.(name|" + "|".join(CO.FIELDS) + r"):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                cur = part[m.group(2)] = {"group_segment_fixed_size": lds}
            else:
                cur[m.group(1)] = int(m.group(2))
        part = {k: v for k, v in part.items() if "vgpr_count" in v}
        if part:
            table.update(zip(CO._source_names(list(part)), part.values()))
    return table
