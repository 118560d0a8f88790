"""The tile kernels on lattice Z-curve keys and shared topology blocks (SMGPU_TILE_LATTICE, SMGPU_TILE_SHARE):
coordinates, residuals and nFrozenPoints of a few iterations are the oracle's bit for bit under all four knob combinations, with the
constraints off and on, on a hex block and on the polyhedral cavity mesh -- and with the tile tables built on the device and on the
host.  The set-up log (SMGPU_VERBOSE=1) shows that the tile kernels ran on the tables the knobs ask for."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GEOM = re.compile(r"\[smgpu\] geometry tiles: (\d+) tiles, distinct blocks: faceVerts (\d+), cellFaces (\d+) \(SMGPU_TILE_LATTICE=(\d) SMGPU_TILE_SHARE=(\d)\)")
_SMOOTH = re.compile(r"\[smgpu\] smoothing tiles: (\d+) tiles, distinct blocks: pcEll (\d+), ppEll\+pairEll (\d+), pfEll (\d+)")
_ITERS = {"hex": 4, "cavity": 3}


def _mesh(kind):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    if kind == "hex":
        return hex_block(36, 28, 20, lengths=(0.9, 0.7, 0.5), jitter=0.25, seed=8)      # 20160 cubic cells: aligned 8 x 4 x 4 bricks, partial ones on one side
    return cavity_mesh(16, jitter=0.2, seed=3)                 # hexahedra, polyhedra and hanging nodes in one tile


def _run(mesh, prm, iters, lattice, share, device_tiles, monkeypatch, capfd):
    from smoothmesh_amd import SmoothEngine
    with monkeypatch.context() as mp:
        mp.setenv("SMGPU_TILE_LATTICE", str(lattice))
        mp.setenv("SMGPU_TILE_SHARE", str(share))
        mp.setenv("SMGPU_DEVICE_TILES", str(device_tiles))
        mp.setenv("SMGPU_VERBOSE", "1")
        capfd.readouterr()
        e = SmoothEngine(mesh)
        e.set_params(prm)
        e.enable_timing(True)
        n, res, frz = e.iterate(iters, 0.0)
        r = dict(n=n, res=res, frz=frz, pts=e.get_points(), cnt={c["name"]: c["launches"] for c in e.counters()}, sums=e.debug_tile_checksums())
        e.close()
        r["err"] = capfd.readouterr().err
    return r


@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("kind", ["hex", "cavity"])
def test_knob_combinations_equal_the_oracle_bit_for_bit(kind, constraints, oracle_lib, monkeypatch, capfd):
    from smoothmesh_amd import default_params
    mesh = _mesh(kind)
    o = oracle_lib.Oracle(mesh)
    prm = default_params(o.mesh_stats()[0], edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
    o.set_params(prm)
    n_o, res_o, frz_o = o.iterate(_ITERS[kind], 0.0)
    pts_o = o.points()
    distinct = {}
    for lattice in (1, 0):
        for share in (1, 0):
            sums = []
            for device_tiles in (1, 0):
                r = _run(mesh, prm, _ITERS[kind], lattice, share, device_tiles, monkeypatch, capfd)
                g, s = _GEOM.search(r["err"]), _SMOOTH.search(r["err"])
                print(kind, constraints, "lattice", lattice, "share", share, "device tiles", device_tiles, "geom", g and g.groups(), "smooth", s and s.groups(),
                      "max |dx|", float(np.max(np.abs(r["pts"] - pts_o))), "residuals equal", np.array_equal(r["res"], res_o))
                assert g and s, r["err"]
                assert (int(g.group(4)), int(g.group(5))) == (lattice, share), r["err"]
                assert r["cnt"]["k_geom_tile"] > 0 and r["cnt"]["k_face_geom"] == 0      # the tile kernels, not the direct-gather fall-back
                tiles, fv, cf = int(g.group(1)), int(g.group(2)), int(g.group(3))
                if not share:
                    assert fv == cf == tiles and all(int(s.group(i)) == int(s.group(1)) for i in (2, 3, 4)), r["err"]
                assert r["n"] == n_o == _ITERS[kind]
                assert np.array_equal(r["frz"], frz_o)
                assert np.array_equal(r["res"], res_o)
                assert np.array_equal(r["pts"], pts_o)
                sums.append(r["sums"])
                distinct[(lattice, share)] = (tiles, fv, cf)
            # the device and the host build: the same tables and the same remapped records, byte for byte
            assert sums[0] == sums[1] and any(sums[0]), (kind, lattice, share)
    if kind == "hex":      # aligned bricks share their blocks; ragged tiles of the bounding-box keys do not
        tiles, fv, cf = distinct[(1, 1)]
        assert fv <= tiles // 4 and cf <= tiles // 4, distinct      # the CPU build (tests/native/tile_sharing_check.cpp): 27 and 27 of 158
        assert distinct[(0, 1)][1] > distinct[(1, 1)][1], distinct
