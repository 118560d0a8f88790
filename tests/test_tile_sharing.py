"""The lattice Z-curve keys (SMGPU_TILE_LATTICE) and the shared topology blocks (SMGPU_TILE_SHARE) of the LDS tile tables
(csrc/tiles.cpp), on the CPU: tests/native/tile_sharing_check.cpp builds the three tile sets with each knob combination, expands
every tile's rows through the remapped bases and compares them entry for entry with the rows the tile owns (the unshared build),
and holds the tiles to capWeighted / capTotal.  What the tables decode to is test_tile_tables.py's business; it runs with the
default knobs, i.e. on lattice keys."""
import os
import re
import shutil
import subprocess

import pytest

from test_tile_tables import CSRC, ROOT, _dump_mesh, _meshes

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_sharing")
    exe = str(d / "tile_sharing_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "tile_sharing_check.cpp"),
                           os.path.join(CSRC, "topology.cpp"), os.path.join(CSRC, "tiles.cpp")])
    return exe, d


def _sets(exe, path, threads):
    r = subprocess.run([exe, path, f"T={threads}"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "done fails=0" in out and "FAIL" not in out and "error" not in out, out
    sets = {}
    for ln in r.stdout.splitlines():
        if not ln.startswith("set "):
            continue
        head = {k: int(v) for k, v in re.findall(r"(lattice|share)=(\d)", ln)}
        parts = re.split(r" (geom|smooth|edge) ", ln)
        vals = {parts[i]: {k: float(v) for k, v in re.findall(r"(\w+)=([\d.]+)", parts[i + 1])} for i in range(1, len(parts), 2)}
        sets[(head["lattice"], head["share"])] = vals
    assert sorted(sets) == [(0, 0), (0, 1), (1, 0), (1, 1)], out
    return sets


def _mesh(name):
    from smoothmesh_amd.meshgen import hex_block
    if name == "hex36":
        return hex_block(36, jitter=0.2, seed=8)      # a side that is no power of two: 4.5 bricks of 8 cells
    return _meshes()[name]()


@pytest.mark.parametrize("threads", [256, 128])
@pytest.mark.parametrize("name", ["hex36", "cavity", "baffle", "fan14", "fan22"])
def test_shared_blocks_expand_to_the_unshared_tables(checker, name, threads):
    exe, d = checker
    path = str(d / f"{name}.bin")
    if not os.path.exists(path):
        _dump_mesh(path, _mesh(name))
    sets = _sets(exe, path, threads)
    for lattice in (0, 1):
        off, on = sets[(lattice, 0)], sets[(lattice, 1)]
        for who, blocks in (("geom", ("fv", "cf")), ("smooth", ("pc", "pp", "pf")), ("edge", ("ef", "ec"))):
            # SMGPU_TILE_SHARE=0: every tile reads its own block; sharing changes the bases alone, not the tiling or what is staged
            assert all(off[who][b] == off[who]["tiles"] for b in blocks), (who, off)
            assert all(1 <= on[who][b] <= on[who]["tiles"] for b in blocks), (who, on)
            assert {k: v for k, v in on[who].items() if k not in blocks} == {k: v for k, v in off[who].items() if k not in blocks}


def test_lattice_keys_make_the_tiles_of_a_hex_block_identical_bricks(checker):
    """36^3 cells, T = 256 (128 cells / 256 points per tile): with lattice keys the geometry tiles are aligned 8 x 4 x 4 bricks of
    225 points and 464 faces at most, and the CPU build gives 27 distinct faceVerts and 27 distinct cellFaces blocks for 365
    tiles (one per position of a brick against the block's boundary: 3 x 3 x 3); with bounding-box keys every block is its own.
    Held to a tenth of the tiles."""
    exe, d = checker
    path = str(d / "hex36.bin")
    if not os.path.exists(path):
        _dump_mesh(path, _mesh("hex36"))
    sets = _sets(exe, path, 256)
    lat, box = sets[(1, 1)], sets[(0, 1)]
    assert lat["geom"]["tiles"] == 365
    assert lat["geom"]["fv"] <= 36 and lat["geom"]["cf"] <= 36, lat      # measured: 27 and 27 of 365
    assert lat["smooth"]["pc"] <= 99 and lat["smooth"]["pp"] <= 99 and lat["smooth"]["pf"] <= 99, lat      # measured: 57 of 198 (a half)
    assert lat["geom"]["maxP"] == 225 and lat["geom"]["maxF"] == 464, lat
    # fewer faces computed twice, fewer points and records staged than on the bounding-box keys
    assert lat["geom"]["faces_x"] < box["geom"]["faces_x"] and lat["geom"]["points_x"] < box["geom"]["points_x"], (lat, box)
    assert lat["smooth"]["cells_x"] < box["smooth"]["cells_x"] and lat["smooth"]["nbrs_x"] < box["smooth"]["nbrs_x"], (lat, box)
