"""Register / scratch budgets of the svgf.hip kernels, read from the built libpbrhip.so in test_kernel_budgets.py's style (no
GPU needed).  svgf.hip is a translation unit of its own, so its kernels live in a code object of their own inside the library's fat
binary: this file walks every bundle of the section, not only the first.

No kernel may use scratch: the filter's 25 taps are unrolled, and a spill inside them would cost every tap.  The VGPR ceilings are the
measured counts rounded up to the next allocation granule of eight: a change that crosses one has to be re-measured on the GPU first."""
import os
import re
import subprocess
import tempfile

import pytest

import _codeobj as CO

# kernel -> (max VGPRs, max scratch bytes); measured: 10, 43, 52, 50, 48
BUDGETS = {
    "k_object_ids": (16, 0),             # 10
    "k_svgf_accumulate": (48, 0),        # 43
    "k_svgf_prepare": (56, 0),           # 52
    "k_svgf_iteration<false>": (56, 0),  # 50
    "k_svgf_iteration<true>": (56, 0),   # 48
}
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _all_kernels():
    """{kernel: {vgpr_count, private_segment_fixed_size, ...}} over every gfx950 code object bundled into the library"""
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    table = {}
    with tempfile.TemporaryDirectory(prefix="pbrhip_svgf_") as tmp:
        fat, part, co = (os.path.join(tmp, n) for n in ("fat.bin", "part.bin", "dev.co"))
        CO._run(os.path.join(CO.LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", CO.LIB)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(MAGIC, blob)] + [len(blob)]
        for a, b in zip(starts, starts[1:]):
            open(part, "wb").write(blob[a:b])
            r = subprocess.run([os.path.join(CO.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = CO._run(os.path.join(CO.LLVM, "llvm-readelf"), "--notes", co)
            os.remove(co)
            found, cur = {}, {}
            for line in notes.splitlines():
                m = re.match(r"\s+(?:- )?\.(name|" + "|".join(CO.FIELDS) + r"):\s+(\S+)", line)
                if not m:
                    continue
                if m.group(1) == "name":
                    cur = found[m.group(2)] = {}
                else:
                    cur[m.group(1)] = int(m.group(2))
            found = {k: v for k, v in found.items() if "vgpr_count" in v}
            table.update(zip(CO._source_names(list(found)), found.values()))
    return table


def test_svgf_kernels_use_no_scratch_and_stay_within_their_registers():
    table = _all_kernels()
    for name, (vgprs, scratch) in BUDGETS.items():
        assert name in table, (name, sorted(k for k in table if "svgf" in k or "object" in k))
        got = table[name]
        print(name, got)
        assert got["private_segment_fixed_size"] <= scratch, (name, got)
        assert got["vgpr_count"] <= vgprs, (name, got)
    # and nothing in svgf.hip escaped the table above
    assert sorted(k for k in table if "svgf" in k or k == "k_object_ids") == sorted(BUDGETS)
