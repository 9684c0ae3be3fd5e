"""CPU: what the host builder's cost buys on rays like the renderer's (pbrlab_amd/csrc/bvh_build.cpp, host_scene.h::BvhBuildOptions,
DESIGN.md section 8 "The cost") -- tests/cpp/bvh_rays_check.cc compiled for the host only.  On the reduced Cornell scene (17 688
triangles with their corners, the two triangles of the light marked) it builds the tree with the passes off, with the pricing of
before (BvhBuildOptions::cost = kBvhCostPrims) and with what a scene commit asks for by default (kBvhCostTurns), and walks 20 000 camera rays, 20 000 bounce rays that start on
the surfaces and their shadow rays to the light through the collapsed tree.  Held: on bounce and on shadow rays the turns a ray pays,
kCostNode x node visits + kCostLeaf x leaf turns, are fewer with the defaults than with the pricing of before; a shadow ray takes no
more leaf turns than on the builder's own tree; two builds are byte-identical; the pricing of before reproduces the tree of the
commit before this cost (tests/golden/bvh_cost_parent_hashes.txt, recorded from that commit's build_bvh + build_qtree).  Small and
degenerate box sets are built under the turn cost and checked for complete trees within the stack.  The program
runs once more under ASan + UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

from pbrlab_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CS = os.path.join(ROOT, "pbrlab_amd", "csrc")


def _compile(exe, extra=()):
    assert os.path.exists(HIPCC), "hipcc builds the library: without it nothing here can be tested"
    subprocess.check_call([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", *extra, "-I" + CS, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bvh_rays_check.cc"), os.path.join(CS, "bvh_build.cpp"), "-o", exe, "-lpthread"])
    return exe


def write_triangles(path, desc):
    """uint32 n, uint32 nl, the corners of the n triangles (9 floats each), the indices of the nl emissive ones (shapes named light*)"""
    v = desc.vertices[:, :3].astype(np.float32)
    tri = np.concatenate([v[s.vertex_ids] for s in desc.shapes])       # (n, 3, 3)
    lights, base = [], 0
    for s in desc.shapes:
        if s.name[:5] == "light":
            lights += list(range(base, base + len(s.vertex_ids)))
        base += len(s.vertex_ids)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(tri), len(lights)))
        f.write(np.ascontiguousarray(tri, np.float32).tobytes())
        f.write(np.asarray(lights, np.uint32).tobytes())
    return len(tri), len(lights)


@pytest.fixture(scope="module")
def cornell_triangles(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("triangles") / "cornell.tri")
    assert write_triangles(path, scenes.cornell_scene(monkey_subdiv=3, lucy_nu=256, lucy_nv=32)) == (17688, 2)
    return path


def _fields(line, first):
    it = line.split()
    return {it[i]: it[i + 1] for i in range(first, len(it) - 1, 2)}


def _parse(out):
    trees = {ln.split()[1]: _fields(ln, 2) for ln in out.splitlines() if ln.startswith("tree ")}
    rays = {(ln.split()[1], ln.split()[2]): {k: float(v) for k, v in _fields(ln, 3).items()} for ln in out.splitlines() if ln.startswith("rays ") and ln != "rays ok"}
    return trees, rays


@pytest.fixture(scope="module")
def walked(tmp_path_factory, cornell_triangles):
    """the checker's lines on the reduced scene, once for every test here"""
    exe = _compile(str(tmp_path_factory.mktemp("rays") / "bvh_rays_check"))
    r = subprocess.run([exe, cornell_triangles], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "rays ok" in r.stdout, r.stdout + r.stderr
    return (r.stdout,) + _parse(r.stdout)


def test_turns_per_ray_fall_against_the_pricing_of_before(walked):
    out, trees, rays = walked
    head = _fields(out.splitlines()[0], 1)
    node, leaf = float(head["cost_node"]), float(head["cost_leaf"])
    assert int(trees["default"]["moves"]) > 0 and int(trees["parent"]["moves"]) > 0 and int(trees["off"]["moves"]) == 0
    for kind in ("bounce", "shadow"):
        new, old = rays[("default", kind)], rays[("parent", kind)]
        t_new, t_old = node * new["nodes"] + leaf * new["leaves"], node * old["nodes"] + leaf * old["leaves"]
        print(f"{kind}: turns per ray {t_old:.4f} -> {t_new:.4f}; nodes {old['nodes']} -> {new['nodes']}, leaf turns {old['leaves']} -> {new['leaves']}")
        assert t_new < t_old, kind


def test_shadow_rays_take_no_more_leaf_turns_than_on_the_builders_tree(walked):
    _, _, rays = walked
    print(f"shadow leaf turns per ray: passes off {rays[('off', 'shadow')]['leaves']}, default {rays[('default', 'shadow')]['leaves']}")
    assert rays[("default", "shadow")]["leaves"] <= rays[("off", "shadow")]["leaves"]


def test_the_pricing_of_before_gives_the_tree_of_before(walked):
    """(two builds per option set byte-identical: the checker fails otherwise)"""
    _, trees, _ = walked
    want = _fields(open(os.path.join(ROOT, "tests", "golden", "bvh_cost_parent_hashes.txt")).read().splitlines()[0], 1)
    got = trees["parent"]
    assert (got["passes"], got["nodes_hash"], got["qtree_hash"]) == (want["passes"], want["nodes_hash"], want["qtree_hash"])
    assert trees["default"]["nodes_hash"] != got["nodes_hash"]


def test_small_and_degenerate_sets_under_the_turn_cost(tmp_path):
    """bvh_reinsert_check.cc builds its sets without options, that is under the pricing of before; here the same shapes under the turn
    cost: complete trees within the stack, byte-identical twice, the cost with the passes not above the builder's tree's"""
    exe = _compile(str(tmp_path / "bvh_rays_check"))
    r = subprocess.run([exe, "--sets"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "sets ok" in r.stdout, r.stdout + r.stderr
    sets = {ln.split()[1]: _fields(ln, 2) for ln in r.stdout.splitlines() if ln.startswith("set ")}
    assert len(sets) == 10
    for name, f in sets.items():
        assert float(f["cost_on"]) <= float(f["cost_off"]), name
    assert int(sets["walls_3000"]["moves"]) > 0 and float(sets["walls_3000"]["cost_on"]) < float(sets["walls_3000"]["cost_off"])


def test_under_the_sanitizers(tmp_path, cornell_triangles):
    exe = _compile(str(tmp_path / "bvh_rays_check_san"), ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for args in (["--sets"], [cornell_triangles]):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and " ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
