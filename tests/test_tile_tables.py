"""The LDS tile tables (csrc/tiles.cpp) decoded back into global ids and held to the mesh, at every tile shape the engine can be set
to (SMGPU_GEOM_T / SMGPU_SMOOTH_T, the caps) and at caps placed on, below and above one element's need.  The decoder,
tests/native/tile_tables_check.cpp, derives the adjacency from faces / owner / neighbour itself, so a mistake that the host and the
device builders share (they are only compared with each other elsewhere) still shows.  CPU only."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothmesh_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

HARD = {"gp": "geom", "gf": "geom", "sc": "smooth", "sn": "smooth", "ep": "edge", "ef": "edge", "ec": "edge"}
ERRORS = {"geom": "a single cell exceeds the LDS tile capacity", "smooth": "a single point exceeds the LDS tile capacity",
          "edge": "a single edge exceeds the LDS tile capacity"}
CAPS = ("gp", "gf", "gw", "sc", "sn", "st", "ep", "ef", "ec", "et")


def _dump_mesh(path, m):
    with open(path, "wb") as f:
        np.array([m.nPoints, m.nCells, m.nFaces, m.nInternalFaces], dtype=np.int32).tofile(f)
        for a, t in ((m.points, np.float64), (m.faceOffsets, np.int32), (m.facePoints, np.int32), (m.owner, np.int32), (m.neighbour, np.int32),
                     (m.find_internal_points(), np.uint8)):
            np.ascontiguousarray(a, dtype=t).tofile(f)


def _meshes():
    from smoothmesh_amd.meshgen import add_baffle, baffle_in_plane, hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    from test_gpu_edge_cases import _fan_mesh
    from test_gpu_topology import _hedgehog
    lattice = hex_block(8, 8, 6)
    return {"hex": lambda: hex_block(12, 10, 9, jitter=0.25, seed=8),                # uniform tiles, the unrolled quad / hex flags
            "cavity": lambda: cavity_mesh(10, jitter=0.2, seed=3),                  # mixed tiles, hanging nodes
            "fan14": lambda: _fan_mesh(12),                                         # pair masks beyond the first 8 neighbours
            "fan22": lambda: _fan_mesh(20),                                         # no pair masks
            "hedgehog": _hedgehog,                                                  # tetrahedra, 42 neighbours, 120 corners
            "baffle": lambda: add_baffle(hex_block(8, 8, 6, jitter=0.1, seed=5), baffle_in_plane(lattice, 0, 0.5))}   # non-manifold edges


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_tables")
    exe = str(d / "tile_tables_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "tile_tables_check.cpp"),
                           os.path.join(CSRC, "topology.cpp"), os.path.join(CSRC, "tiles.cpp")])
    return exe, d


def _run(exe, mesh, env=None, timeout=300, **kv):
    r = subprocess.run([exe, mesh] + [f"{k}={v}" for k, v in kv.items()], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    out = r.stdout
    need = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[0])} if out.startswith("need ") else {}
    last = out.strip().splitlines()[-1] if out.strip() else ""
    tiles = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", last)} if last.startswith("tiles ") else {}
    fails = [ln for ln in out.splitlines() if ln.startswith("FAIL ")]
    errors = [ln for ln in out.splitlines() if ln.startswith("error ")]
    return r.returncode, need, tiles, fails, errors, out + r.stderr


@pytest.mark.parametrize("threads", [64, 128, 256])
@pytest.mark.parametrize("name", ["hex", "cavity", "fan14", "fan22", "hedgehog", "baffle"])
def test_tile_tables_decode_to_the_mesh(decoder, name, threads):
    exe, d = decoder
    path = str(d / f"{name}.bin")
    if not os.path.exists(path):
        _dump_mesh(path, _meshes()[name]())
    rc, need, info, fails, errors, out = _run(exe, path, T=threads)
    assert rc == 0 and not fails and not errors and need, out
    if name == "fan14":
        assert 8 < info["maxPointPoints"] <= 16
    if name in ("fan22", "hedgehog"):
        assert info["maxPointPoints"] > 16
    if name == "baffle":
        assert info["nonManifoldEdges"] > 0
    soft = {"gw": need["gw"] - 1, "st": need["st"] - 1, "et": need["et"] - 1}
    shapes = {
        "default": {},                                                  # what smgpu.hip derives from T
        # (SMGPU_GEOM_CELLS=1 alone would also shrink the derived point / face caps below one hex cell's need: the caps of T stay)
        "one element per tile": {"gc": 1, "gp": min(3 * threads, 1400), "gf": min(2 * threads, 1400), "st": 1, "et": 1},
        "caps at one element's need": {k: need[k] for k in CAPS},       # the '>' boundary: an element that fills a cap exactly fits
        "caps at twice the need": {k: 2 * need[k] for k in CAPS},       # tiles that close exactly on a cap
        "soft caps below one element": soft,                            # capWeighted / capTotal: an element alone may exceed them
    }
    for morton in (1, 0):
        for shape, caps in shapes.items():
            rc, _, info, fails, errors, out = _run(exe, path, T=threads, morton=morton, subset=7 + threads, **caps)
            assert rc == 0 and not fails and not errors, (shape, morton, out)
            if shape == "one element per tile":
                assert (info["geom"], info["smooth"], info["edge"]) == (info["cells"], info["points"], info["edges"]), (shape, out)
        # a hard cap one below the largest element's need: that builder refuses with its documented message, the others are unaffected
        for k, who in HARD.items():
            rc, _, _, fails, errors, out = _run(exe, path, T=threads, morton=morton, **{k: need[k] - 1})
            assert errors == [f"error {who}: {ERRORS[who]}"] and not fails, (k, morton, out)


@pytest.fixture(scope="module")
def big_block(decoder):
    """a 128^3 block: 2.10 M cells, 2.15 M points, 6.39 M edges -- every greedy pass cuts its sequence into segments"""
    from smoothmesh_amd.meshgen import hex_block
    _, d = decoder
    path = str(d / "block128.bin")
    m = hex_block(128, jitter=0.2, seed=1)
    assert m.nCells >= 2 << 20 and m.nPoints >= 2 << 20
    _dump_mesh(path, m)
    return path


@pytest.mark.parametrize("segments", [1, 7, 64])
def test_segmented_tiling(decoder, big_block, segments):
    """SMGPU_TILE_SEGMENTS with 64 host threads (each count in a process of its own: tileSegments() and hostThreads() are cached):
    the cuts n*sg/segs are tile boundaries, every other boundary is forced by a cap, and every table invariant still holds"""
    exe, _ = decoder
    env = {"SMGPU_TILE_SEGMENTS": str(segments), "SMGPU_HOST_THREADS": "64"}
    rc, _, info, fails, errors, out = _run(exe, big_block, env=env, timeout=900, segs=min(segments, 64))
    assert rc == 0 and not fails and not errors, out
    assert info["edges"] >= 4 << 20 and info["geom"] > 0 and info["smooth"] > 0 and info["edge"] > 0
