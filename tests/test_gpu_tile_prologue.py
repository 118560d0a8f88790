"""The tile kernels' prologue -- the launch record (TileLaunch: meta table, tile list, stop word, tile count, XCD map), the scalar
batches and the branch-free first staging round of the geometry tiles (csrc/kernels_tiled.hpp) -- bit for bit against the
oracle: coordinates, residuals and frozen-point counts with np.array_equal, over 4 iterations.  The cases are the smallest at
which that code can go wrong: launches that are mostly padding workgroups, tile counts that are no multiple of 8 with and
without the XCD map, mixed tiles on the general paths, tiles beyond the fixed staging rounds, a run that stops (the stop word
through the record's pointer), and launches that pass a tile list or fill the record in per role (two sub-domains on one GPU)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 4
_TILES = re.compile(r"\[smgpu\] tiles: geom T=(\d+) n=(\d+) LDS=\d+ B \(maxP (\d+) maxF (\d+);.*smooth T=(\d+) n=(\d+) LDS=\d+ B \(maxC (\d+) maxN (\d+)\)")
_ORACLE = {}


def _mesh(kind):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    if kind == "hex6":
        return hex_block(6, 6, 6, jitter=0.3, seed=5)
    if kind == "hex12":
        return hex_block(12, 12, 12, jitter=0.3, seed=5)
    if kind == "hex12calm":
        return hex_block(12, 12, 12, jitter=0.1, seed=5)      # its residual falls below 1 after the first iteration
    if kind == "cavity10":
        return cavity_mesh(10, jitter=0.2, seed=3)
    raise ValueError(kind)


def _oracle(oracle_lib, kind, constraints=False, iters=ITERS, relTol=0.0):
    """(mesh, params, the oracle's run), computed once per module and left unchanged"""
    key = (kind, constraints, iters, relTol)
    if key not in _ORACLE:
        from smoothmesh_amd import default_params
        mesh = _mesh(kind)
        o = oracle_lib.Oracle(mesh)
        prm = default_params(o.mesh_stats()[0], edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
        o.set_params(prm)
        n, res, frz = o.iterate(iters, relTol)
        _ORACLE[key] = (mesh, prm, dict(n=n, res=np.array(res), frz=np.array(frz), pts=np.array(o.points())))
    return _ORACLE[key]


def _engine(mesh, prm, env, monkeypatch, capfd, iters=ITERS, relTol=0.0):
    from smoothmesh_amd import SmoothEngine
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        mp.setenv("SMGPU_VERBOSE", "1")
        capfd.readouterr()
        e = SmoothEngine(mesh)
        e.set_params(prm)
        e.enable_timing(True)
        n, res, frz = e.iterate(iters, relTol)
        r = dict(n=n, res=np.array(res), frz=np.array(frz), pts=np.array(e.get_points()), cnt={c["name"]: c["launches"] for c in e.counters()})
        e.close()
        r["err"] = capfd.readouterr().err
    m = _TILES.search(r["err"])
    assert m, r["err"]      # the tiled kernels ran, not the direct-gather ones
    r["tiles"] = dict(zip(("geomT", "nGeom", "maxP", "maxF", "smoothT", "nSmooth", "maxC", "maxN"), map(int, m.groups())))
    assert r["cnt"]["k_geom_tile"] > 0 and r["cnt"]["k_face_geom"] == 0
    return r


def _same_bits(run, orc):
    assert run["n"] == orc["n"], (run["n"], orc["n"])
    assert np.array_equal(run["frz"], orc["frz"]), (run["frz"], orc["frz"])
    assert np.array_equal(run["res"], orc["res"]), (run["res"], orc["res"])
    assert np.array_equal(run["pts"], orc["pts"]), float(np.max(np.abs(run["pts"] - orc["pts"])))


def test_launch_of_mostly_padding_workgroups(oracle_lib, monkeypatch, capfd):
    """hex_block(6): fewer than eight geometry tiles, so most workgroups of the XCD-mapped grid find no tile (launchedTile -> -1)"""
    mesh, prm, orc = _oracle(oracle_lib, "hex6")
    run = _engine(mesh, prm, {}, monkeypatch, capfd)
    assert 0 < run["tiles"]["nGeom"] < 8 and 0 < run["tiles"]["nSmooth"] < 8, run["tiles"]
    _same_bits(run, orc)


@pytest.mark.parametrize("xcdMap", [1, 0])
def test_tile_count_no_multiple_of_eight(oracle_lib, monkeypatch, capfd, xcdMap):
    """hex_block(12): several workgroups per XCD and a ragged last one; SMGPU_XCD_MAP=0: the workgroup's index is its tile"""
    mesh, prm, orc = _oracle(oracle_lib, "hex12")
    run = _engine(mesh, prm, {"SMGPU_XCD_MAP": xcdMap}, monkeypatch, capfd)
    assert run["tiles"]["nGeom"] > 8 and run["tiles"]["nGeom"] % 8 != 0, run["tiles"]
    _same_bits(run, orc)


@pytest.mark.parametrize("constraints", [False, True])
def test_mixed_tiles_on_the_general_paths(oracle_lib, monkeypatch, capfd, constraints):
    """cavity_mesh(10): tiles that are neither all quadrilaterals nor all six-faced cells (no rows read ahead: every lane reads
    entry 0 of the tables and discards it); constraints on: the proposal form k_smooth_tile<false> and the face averages"""
    mesh, prm, orc = _oracle(oracle_lib, "cavity10", constraints)
    run = _engine(mesh, prm, {}, monkeypatch, capfd)
    _same_bits(run, orc)


def test_tiles_beyond_the_fixed_staging_rounds(oracle_lib, monkeypatch, capfd):
    """64-thread tiles of 64 cells / 64 points under caps far above 2 T, in the mesh's own order (on the Z-curve a 64-cell tile of
    this block is a 4 x 4 x 4 brick of 125 points; five and a half rows of 12 cells hold 192): more than 2 T points per geometry
    tile (the staging loop behind the two fixed rounds) and more than 2 T cell centres per smoothing tile (the set-by-set
    branch of smoothStage).  The tile maxima of the set-up line are the evidence"""
    mesh, prm, orc = _oracle(oracle_lib, "hex12")
    env = {"SMGPU_GEOM_T": 64, "SMGPU_SMOOTH_T": 64, "SMGPU_GEOM_CELLS": 64, "SMGPU_GEOM_CAPP": 768, "SMGPU_GEOM_CAPF": 512,
           "SMGPU_SMOOTH_CAPC": 256, "SMGPU_SMOOTH_CAPN": 512, "SMGPU_SMOOTH_CAPTOTAL": 768, "SMGPU_TILE_MORTON": 0}
    run = _engine(mesh, prm, env, monkeypatch, capfd)
    t = run["tiles"]
    assert (t["geomT"], t["smoothT"]) == (64, 64), t
    assert t["maxP"] > 2 * 64, t                              # geomStorePoints' loop
    assert t["maxC"] > 2 * 64 or t["maxN"] > 3 * 64, t        # smoothStage: not `fast`
    _same_bits(run, orc)


def test_a_run_that_stops(oracle_lib, monkeypatch, capfd):
    """relTol = 0.09 on the calm block: the oracle's residual series is 1.0, 0.285, 0.175, 0.109, 0.069, ... so the loop stops after
    iteration 5 of 8.  The engine reads the stop word through TileLaunch::stop and tests it after the staging: the iteration count and the
    coordinates are the oracle's"""
    mesh, prm, orc = _oracle(oracle_lib, "hex12calm", iters=8, relTol=0.09)
    assert 2 < orc["n"] < 8, orc["n"]
    run = _engine(mesh, prm, {}, monkeypatch, capfd, iters=8, relTol=0.09)
    _same_bits(run, orc)


@pytest.mark.parametrize("form", ["one kernel per step", "one kernel per step, exchange stream", "multi-role launches"])
def test_two_subdomains_with_tile_lists(oracle_lib, monkeypatch, form):
    """hex_subdomain((8, 8, 8), (2, 1, 1), r) as two engines on one GPU against MultiOracle: k_pack_tile on the list of the tiles with
    shared points; with an exchange stream k_geom_tile / k_smooth_tile on the interior / shared lists; the multi-role launches
    (k_geom_halo, k_smooth_halo), whose roles fill the record in themselves"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import shared_point_table
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    subs = [hex_subdomain((8, 8, 8), (2, 1, 1), r, jitter=0.3, seed=9) for r in range(2)]
    orcs = [oracle_lib.Oracle(s.mesh) for s in subs]
    prm = default_params(min(o.mesh_stats()[0] for o in orcs), edgeAngleConstraint=False, faceAngleConstraint=False)
    for o in orcs:
        o.set_params(prm)
    n_o, res_o, frz_o = oracle_lib.MultiOracle(orcs, *shared_point_table(subs)).iterate(ITERS, 0.0)
    merged = form == "multi-role launches"
    with monkeypatch.context() as mp:
        mp.setenv("SMGPU_HALO_MERGED", "1" if merged else "0")
        ms = LocalMultiSmoother(subs, device=0, overlap=form.endswith("exchange stream"))
        ms.set_params(prm)
        for st in ms.states:
            st.eng.enable_timing(True)
        n_g, res_g, frz_g = ms.iterate(ITERS, 0.0)
        pts = ms.get_points()
        cnt = {c["name"]: c["launches"] for c in ms.states[0].eng.counters()}
        mode = ms.states[0].eng.debug_halo_mode()
        for st in ms.states:
            st.eng.close()
    assert cnt["k_geom_tile"] > 0 and cnt["k_face_geom"] == 0, cnt
    assert mode["multi_role"] == merged, mode
    assert n_g == n_o
    assert np.array_equal(np.array(frz_g), np.array(frz_o))
    assert np.array_equal(np.array(res_g), np.array(res_o)), (res_g, res_o)
    for o, p in zip(orcs, pts):
        assert np.array_equal(np.array(p), np.array(o.points()))
