"""Records what the set-up of the PARENT commit leaves on the device, for tests/test_gpu_setup_equals_parent.py: per configuration the
checksums of the addressing, the checksums of the tile tables and the engine's device bytes, into tests/golden/setup_checksums.json.

    python scripts/record_setup_checksums.py                 # checks the parent out of git into a temporary directory and builds it
    python scripts/record_setup_checksums.py --lib PATH      # a libsmgpu.so of the parent that stands already

Needs a GPU.  The configurations are defined here and travel inside the file, so the test runs exactly what was recorded."""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = "e917966"
KNOBS = ("SMGPU_DEVICE_TOPOLOGY", "SMGPU_DEVICE_TILES", "SMGPU_TILE_SHARE", "SMGPU_GEOM_T", "SMGPU_SMOOTH_T", "SMGPU_FILTER")
MESHES = ("hex", "cavity", "hedgehog")


def configurations():
    for mesh, topo, tiles, share in itertools.product(MESHES, "10", "102", "10"):
        yield mesh, {"SMGPU_DEVICE_TOPOLOGY": topo, "SMGPU_DEVICE_TILES": tiles, "SMGPU_TILE_SHARE": share}
    for T in ("64", "128"):
        yield "hex", {"SMGPU_GEOM_T": T, "SMGPU_SMOOTH_T": T}
    yield "hex", {"SMGPU_FILTER": "0"}


def build_parent(where):
    """the parent's sources out of git, its libsmgpu.so built beside them"""
    tar = subprocess.run(["git", "-C", ROOT, "archive", PARENT, "smoothmesh_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", where], input=tar, check=True)
    csrc = os.path.join(where, "smoothmesh_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, os.path.join(csrc, "libsmgpu.so")])
    return os.path.join(csrc, "libsmgpu.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="libsmgpu.so of the parent commit (default: built from git)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "setup_checksums.json"))
    a = ap.parse_args()
    tmp = None
    if not a.lib:
        tmp = tempfile.TemporaryDirectory()
        a.lib = build_parent(tmp.name)
    os.environ["SMOOTHMESH_SMGPU_LIB"] = os.path.abspath(a.lib)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from test_gpu_setup_equals_parent import mesh_of
    from smoothmesh_amd import SmoothEngine
    cases, lists = [], []      # (many configurations give the same tables: each distinct list of checksums is written once)

    def index_of(sums):
        word = "".join(f"{x:016x}" for x in sums)
        if word not in lists:
            lists.append(word)
        return lists.index(word)

    for mesh, env in configurations():
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        e = SmoothEngine(mesh_of(mesh))
        cases.append({"mesh": mesh, "env": env, "addressing": index_of(e.debug_addressing_checksums()),
                      "tiles": index_of(e.debug_tile_checksums()), "deviceBytes": int(e.sizes()["deviceBytes"])})
        e.close()
    with open(a.out, "w") as f:
        f.write('{"parent": "%s",\n"lists": [\n%s],\n"cases": [\n%s]}\n' % (PARENT, ",\n".join(json.dumps(x) for x in lists),
                                                                      ",\n".join(json.dumps(c) for c in cases)))
    print(f"{len(cases)} configurations -> {a.out}")


if __name__ == "__main__":
    main()
