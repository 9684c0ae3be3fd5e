#!/usr/bin/env python3
"""The kernels of a built library, read from its gfx950 code object (tests/_codeobj.py):

  scripts/ktable.py [libpbrhip.so] [name prefix ...]          registers / scratch / LDS of each kernel
  scripts/ktable.py [libpbrhip.so] --diff OTHER.so [old=new ...]
      OTHER's kernels against this library's, instruction by instruction (position-independent text) and by their metadata;
      old=new renames a kernel of OTHER first.  Exit status 1 when a kernel differs or exists on one side only."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _codeobj as CO


def show(lib, prefixes):
    for n, v in sorted(CO.kernel_table(lib).items()):
        if not prefixes or n.startswith(prefixes):
            print(f"{n:50s} vgpr {v['vgpr_count']:4d} sgpr {v['sgpr_count']:4d} scratch {v['private_segment_fixed_size']:4d} lds {v['group_segment_fixed_size']:6d}")


def diff(lib, other, renames):
    ren = dict(r.split("=", 1) for r in renames)
    new_t, new_d = CO.kernel_table(lib), CO.disassembly(lib)
    old_t = {ren.get(k, k): v for k, v in CO.kernel_table(other).items()}
    old_d = {ren.get(k, k): v for k, v in CO.disassembly(other).items()}
    only_old, only_new = sorted(set(old_t) - set(new_t)), sorted(set(new_t) - set(old_t))
    lib, other = os.path.relpath(lib), os.path.relpath(other)
    print(f"kernels: {len(old_t)} in {other}, {len(new_t)} in {lib}")
    for side, names in ((other, only_old), (lib, only_new)):
        for n in names:
            print(f"only in {side}: {n}")
    same = different = 0
    for n in sorted(set(old_t) & set(new_t)):
        meta = [f"{f} {old_t[n][f]} -> {new_t[n][f]}" for f in CO.FIELDS if old_t[n][f] != new_t[n][f]]
        if old_d[n] == new_d[n] and not meta:
            same += 1
            continue
        different += 1
        moved = sum(1 for a, b in zip(old_d[n], new_d[n]) if a != b)
        print(f"DIFF {n}: {len(old_d[n])} -> {len(new_d[n])} instructions, {moved} lines differ in place" + "".join("; " + m for m in meta))
    print(f"identical: {same} different: {different}")
    return 1 if different or only_old or only_new else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    lib = args.pop(0) if args and args[0] != "--diff" else CO.LIB
    if args and args[0] == "--diff":
        if len(args) < 2:
            sys.exit(__doc__)
        sys.exit(diff(lib, args[1], args[2:]))
    show(lib, tuple(args))
