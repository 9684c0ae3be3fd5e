"""Register / scratch / LDS budgets of the emission.hip kernels, read from the built libpbrhip.so in
test_svgf_budgets.py's style (no GPU needed): emission.hip is a translation unit of its own, so every bundle of the fat binary is walked.

No kernel may use scratch.  The VGPR ceilings are the measured counts rounded up to the next allocation granule of eight.  The traced
kernel must stay in k_features' occupancy class: the same 40 KB of LDS stack and __launch_bounds__(256, 4) -- four blocks per CU, four
waves per SIMD, at most 128 VGPRs -- so both kernels' counts are read from the same table and printed side by side.  Measured:
k_features<true, false> / <true, true> / <false, true> 112 / 109 / 113, k_features_emission 122 / 119 / 123 (the emission sums are four
more live registers across the traversal, and the light record's gather is scheduled beside the albedo's)."""
import os
import re
import subprocess
import tempfile

import pytest

import _codeobj as CO

# kernel -> (max VGPRs, max scratch bytes, LDS bytes); measured VGPRs in the comments
BUDGETS = {
    "k_features_emission<true, false>": (128, 0, 40960),  # 122
    "k_features_emission<true, true>": (120, 0, 40960),   # 119
    "k_features_emission<false, true>": (128, 0, 40960),  # 123
    "k_emission_split": (16, 0, 0),                       # 13
    "k_emission_merge": (32, 0, 0),                       # 29
}
FEATURES = ("k_features<true, false>", "k_features<true, true>", "k_features<false, true>")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _all_kernels():
    """{kernel: {vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size}} over every gfx950 code object bundled
    into the library.  A kernel's record lists .group_segment_fixed_size before its .name (_codeobj.kernel_table's note): it is held
    until the name comes."""
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    table = {}
    with tempfile.TemporaryDirectory(prefix="pbrhip_emission_") as tmp:
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
            found, cur, lds = {}, {}, 0
            for line in notes.splitlines():
                m = re.match(r"\s+(?:- )?\.(name|" + "|".join(CO.FIELDS) + r"):\s+(\S+)", line)
                if not m:
                    continue
                if m.group(1) == "group_segment_fixed_size":
                    lds = int(m.group(2))
                elif m.group(1) == "name":
                    cur = found[m.group(2)] = {"group_segment_fixed_size": lds}
                else:
                    cur[m.group(1)] = int(m.group(2))
            found = {k: v for k, v in found.items() if "vgpr_count" in v}
            table.update(zip(CO._source_names(list(found)), found.values()))
    return table


def test_emission_kernels_use_no_scratch_and_stay_within_their_registers():
    table = _all_kernels()
    for name, (vgprs, scratch, lds) in BUDGETS.items():
        assert name in table, (name, sorted(k for k in table if "emission" in k))
        got = table[name]
        print(name, got)
        assert got["private_segment_fixed_size"] <= scratch, (name, got)
        assert got["vgpr_count"] <= vgprs, (name, got)
        assert got["group_segment_fixed_size"] == lds, (name, got)
    # and nothing in emission.hip escaped the table above
    assert sorted(k for k in table if "emission" in k) == sorted(BUDGETS)


def test_traced_kernel_stays_in_k_features_occupancy_class():
    table = _all_kernels()
    for base in FEATURES:
        new = base.replace("k_features", "k_features_emission")
        a, b = table[base], table[new]
        print(f"{base}: {a['vgpr_count']} VGPRs, {a['group_segment_fixed_size']} B LDS; {new}: {b['vgpr_count']} VGPRs, {b['group_segment_fixed_size']} B LDS")
        assert b["group_segment_fixed_size"] == a["group_segment_fixed_size"] == 40960
        assert CO.waves_per_simd(b["vgpr_count"]) == CO.waves_per_simd(a["vgpr_count"]) == 4  # __launch_bounds__(256, 4): 128 VGPRs
        assert b["private_segment_fixed_size"] == a["private_segment_fixed_size"] == 0
