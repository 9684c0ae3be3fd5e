"""Register / scratch budgets of the environment light's kernels, read from the gfx950 code object like
test_kernel_budgets.py does.

No environment kernel reads or writes scratch: the disassembly of every one of them holds no scratch or buffer instruction, and
its private segment is 0 bytes -- except k_shade_principled<6> (textured materials), whose code object reserves 8 bytes that no
instruction touches, exactly like its twin k_shade_principled<2> of the parent.  Occupancy classes are the twins', except
k_shade_principled<5> (media + environment): three waves per SIMD, where four spilled 12 bytes; its measured cost is in
profiles/README.md."""
import os
import re
import shutil
import subprocess
import tempfile

from test_kernel_budgets import LLVM, ROOT, kernel_table, waves_per_simd

# kernel -> (max VGPRs, min waves per SIMD)
ENV_BUDGETS = {
    "k_classify_env": (64, 8),
    "k_shade_hair_env": (128, 4),
    "k_sss_step_env": (128, 4),
    "k_shade_principled<4>": (128, 4),
    "k_shade_principled<5>": (168, 3),
    "k_shade_principled<6>": (168, 3),
    "k_tail<4, false, false, true>": (168, 3),
    "k_tail<4, false, true, true>": (168, 3),
    "k_tail<5, false, false, true>": (168, 3),
    "k_tail<5, false, true, true>": (168, 3),
    "k_tail<6, false, false, true>": (168, 3),
}
RESERVED_UNUSED = {"k_shade_principled<6>": 8}  # private bytes the compiler reserves and no instruction uses (its twin <2> too)


def _env_kernels(table):
    return [k for k in table if k.endswith("_env") or re.match(r"k_(shade_principled|tail)<[456][,>]", k)]


def test_env_kernels_stay_within_their_budgets():
    table = kernel_table()
    for name, (vgprs, waves) in ENV_BUDGETS.items():
        assert name in table, (name, sorted(_env_kernels(table)))
        got = table[name]
        assert got["vgpr_count"] <= vgprs, (name, got)
        assert waves_per_simd(got["vgpr_count"]) >= waves, (name, got)


def test_every_env_kernel_has_no_scratch():
    table = kernel_table()
    env = _env_kernels(table)
    assert len(env) >= 3 + 3 + 16
    for k in env:
        assert table[k]["private_segment_fixed_size"] <= RESERVED_UNUSED.get(k, 0), (k, table[k])
    # and no instruction of any of them touches scratch
    lib = os.path.join(ROOT, "pbrlab_amd", "libpbrhip.so")
    tmp = tempfile.mkdtemp()
    try:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    bodies, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = bodies.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line)
    names = list(bodies)
    demangled = subprocess.run(["c++filt"] + names, check=True, capture_output=True, text=True).stdout.split("\n")
    by_name = {d.replace("void pb::", "").replace("pb::", "").split("(")[0]: bodies[n] for d, n in zip(demangled, names)}
    for k in env:
        assert k in by_name, k
        bad = [l for l in by_name[k] if re.search(r"\b(scratch_|buffer_)", l)]
        assert not bad, (k, bad[:4])
