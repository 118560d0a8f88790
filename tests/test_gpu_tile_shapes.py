"""The tile kernels at every tile shape and cap the engine can be set to (SMGPU_GEOM_T / SMGPU_SMOOTH_T, the LDS caps,
SMGPU_DEFER_FINISH): against the oracle as test_gpu_edge_cases does, and bit for bit against the same engine at the default shape
(the summation order does not depend on the tiling).  Every tiled case also reads the SMGPU_VERBOSE=1 line of
the tile set-up, so that a silent fall-back to the direct-gather kernels cannot pass as a pass; the cap cases one below an element's
need check that the fall-back is what ran."""
import re

import numpy as np
import pytest

from conftest import rel_linf

pytestmark = pytest.mark.gpu

_TILES = re.compile(r"\[smgpu\] tiles: geom T=(\d+) .* smooth T=(\d+) ")
_EDGE_TILES = "[smgpu] edge tiles: n="
_CACHE = {}


def _mesh(kind):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    from test_gpu_edge_cases import _fan_mesh
    if kind == "hex":
        return hex_block(24, 20, 18, jitter=0.25, seed=8)      # quadrilateral-only tiles
    if kind == "cavity":
        return cavity_mesh(16, jitter=0.2, seed=3)             # mixed tiles
    if kind == "fan22":
        return _fan_mesh(20)                                   # valence 22: no pair masks, wide rows
    if kind == "block":
        return hex_block(9, 8, 7, jitter=0.47, seed=21)        # residuals equal to the oracle's bit for bit (test_gpu_parity)
    raise ValueError(kind)


_ITERS = {"hex": 4, "cavity": 3, "fan22": 8, "block": 6}


def _engine(mesh, prm, iters, env, monkeypatch, capfd, org=False):
    """one engine under `env` (set through the run: some knobs are read per iteration) -> its results, counters and set-up log"""
    from smoothmesh_amd import SmoothEngine
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        mp.setenv("SMGPU_VERBOSE", "1")
        capfd.readouterr()
        e = SmoothEngine(mesh)
        if org:
            e.set_foam_variant("org")
        e.set_params(prm)
        e.enable_timing(True)
        n, res, frz = e.iterate(iters, 0.0)
        r = dict(n=n, res=res, frz=frz, pts=e.get_points(), cnt={c["name"]: c["launches"] for c in e.counters()})
        e.close()
        r["err"] = capfd.readouterr().err
    return r


def _shape(run):
    m = _TILES.search(run["err"])
    return (int(m.group(1)), int(m.group(2))) if m else None


def _reference(kind, constraints, oracle_lib, monkeypatch, capfd, org=False):
    """(mesh, params, oracle run, default-shape engine run), once per module"""
    key = (kind, constraints, org)
    if key not in _CACHE:
        from smoothmesh_amd import default_params
        mesh = _mesh(kind)
        o = oracle_lib.Oracle(mesh)
        if org:
            o.set_foam_variant("org")
        prm = default_params(o.mesh_stats()[0], edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
        o.set_params(prm)
        n, res, frz = o.iterate(_ITERS[kind], 0.0)
        orc = dict(n=n, res=res, frz=frz, pts=o.points())
        base = _engine(mesh, prm, _ITERS[kind], {}, monkeypatch, capfd, org=org)
        assert _shape(base) == (256, 256), base["err"]
        _CACHE[key] = (mesh, prm, orc, base)
    return _CACHE[key]


def _check(run, orc, base=None, shape=None):
    assert run["n"] == orc["n"] and np.array_equal(run["frz"], orc["frz"])
    assert np.max(np.abs(orc["res"] - run["res"]) / np.maximum(orc["res"], 1e-300)) <= 1e-10
    assert rel_linf(run["pts"], orc["pts"]) <= 1e-13
    if base is not None:
        assert np.array_equal(run["pts"], base["pts"]) and np.array_equal(run["res"], base["res"]) and np.array_equal(run["frz"], base["frz"])
    if shape is not None:
        assert _shape(run) == shape, run["err"]
        assert run["cnt"]["k_geom_tile"] > 0 and run["cnt"]["k_face_geom"] == 0


def _needs(mesh):
    """the largest single element's need per cap, from the mesh (what a tile of one cell / point / edge stages)"""
    fo, fp, own, nei = mesh.faceOffsets, mesh.facePoints, mesh.owner, mesh.neighbour
    cellPts = [set() for _ in range(mesh.nCells)]
    cellFcs = [0] * mesh.nCells
    ptCells = [set() for _ in range(mesh.nPoints)]
    ptNbs = [set() for _ in range(mesh.nPoints)]
    edge = {}
    for f in range(mesh.nFaces):
        vs = fp[fo[f]:fo[f + 1]].tolist()
        cs = [int(own[f])] + ([int(nei[f])] if f < mesh.nInternalFaces else [])
        for c in cs:
            cellPts[c].update(vs)
            cellFcs[c] += 1
        for j, p in enumerate(vs):
            q = vs[(j + 1) % len(vs)]
            ptCells[p].update(cs); ptCells[q].update(cs)
            ptNbs[p].add(q); ptNbs[q].add(p)
            fs, ce = edge.setdefault((min(p, q), max(p, q)), (set(), set()))
            fs.add(f); ce.update(cs)
    gp = max(len(s) for s in cellPts)
    return dict(gp=gp, gf=max(cellFcs), gw=max(3 * len(s) + 6 * n for s, n in zip(cellPts, cellFcs)),
                sc=max(len(s) for s in ptCells), sn=max(1 + len(s) for s in ptNbs), st=max(len(c) + 1 + len(n) for c, n in zip(ptCells, ptNbs)),
                ep=2, ef=max(len(fs) for fs, _ in edge.values()), ec=max(len(c) for _, c in edge.values()),
                et=max(2 + len(fs) + len(c) for fs, c in edge.values()))


def _cap_env(need):
    return {"SMGPU_GEOM_CAPP": need["gp"], "SMGPU_GEOM_CAPF": need["gf"], "SMGPU_GEOM_CAPWEIGHTED": need["gw"],
            "SMGPU_SMOOTH_CAPC": need["sc"], "SMGPU_SMOOTH_CAPN": need["sn"], "SMGPU_SMOOTH_CAPTOTAL": need["st"],
            "SMGPU_EDGE_CAPP": need["ep"], "SMGPU_EDGE_CAPF": need["ef"], "SMGPU_EDGE_CAPC": need["ec"], "SMGPU_EDGE_CAPTOTAL": need["et"]}


@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("kind", ["hex", "cavity", "fan22"])
@pytest.mark.parametrize("geomT,smoothT", [(64, 64), (128, 128), (64, 256), (256, 64)])
def test_tile_shapes_match_the_oracle_and_the_default_shape(oracle_lib, monkeypatch, capfd, geomT, smoothT, kind, constraints):
    """k_geom_tile<T>, k_smooth_tile<FINAL, T>, and with SMGPU_SMOOTH_T != 256 the untiled edge-angle filter"""
    mesh, prm, orc, base = _reference(kind, constraints, oracle_lib, monkeypatch, capfd)
    run = _engine(mesh, prm, _ITERS[kind], {"SMGPU_GEOM_T": geomT, "SMGPU_SMOOTH_T": smoothT}, monkeypatch, capfd)
    _check(run, orc, base, (geomT, smoothT))


@pytest.mark.parametrize("T", [64, 128])
def test_openfoam_org_instances(oracle_lib, monkeypatch, capfd, T):
    """k_geom_tile<T, ORG>: the OpenFOAM.org geometry at the smaller tiles"""
    mesh, prm, orc, base = _reference("cavity", True, oracle_lib, monkeypatch, capfd, org=True)
    run = _engine(mesh, prm, _ITERS["cavity"], {"SMGPU_GEOM_T": T, "SMGPU_SMOOTH_T": T}, monkeypatch, capfd, org=True)
    _check(run, orc, base, (T, T))


@pytest.mark.parametrize("T", [64, 128])
def test_boundary_smoothing_at_small_tiles(oracle_lib, monkeypatch, capfd, T):
    """k_geom_tile_bnd<T> and k_bnd_fix behind the smaller smoothing tiles (the small case of test_gpu_boundary)"""
    from bnd_cases import boundary_inputs, make_pair, tangential_jitter
    from smoothmesh_amd.meshgen import hex_block
    m = tangential_jitter(hex_block(12, 10, 9, jitter=0.25, seed=11), 0.02, seed=3)
    init, target, surf = boundary_inputs(7, 5)
    runs = []
    for env in ({}, {"SMGPU_GEOM_T": T, "SMGPU_SMOOTH_T": T}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, str(v))
            mp.setenv("SMGPU_VERBOSE", "1")
            capfd.readouterr()
            o, e, prm, on = make_pair(m, oracle_lib, init, target, surf)
            assert on
            n_o, res_o, frz_o = o.iterate(12, 0.0)
            n_g, res_g, frz_g = e.iterate(12, 0.0)
            runs.append(dict(n=n_g, res=res_g, frz=frz_g, pts=e.get_points(), err=capfd.readouterr().err))
            e.close()
        orc = dict(n=n_o, res=res_o, frz=frz_o, pts=o.points())
        assert _shape(runs[-1]) == ((T, T) if env else (256, 256)), runs[-1]["err"]
        _check(runs[-1], orc, runs[0])


def test_layers_at_128_thread_tiles(oracle_lib, monkeypatch, capfd):
    from test_gpu_layers import _pair
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(12, 10, 9, jitter=0.25, seed=11)
    runs = []
    for env in ({}, {"SMGPU_GEOM_T": 128, "SMGPU_SMOOTH_T": 128}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, str(v))
            mp.setenv("SMGPU_VERBOSE", "1")
            capfd.readouterr()
            o, e, on = _pair(m, oracle_lib, ["xmin", "ymax"], False, layerExpansionRatio=1.2)
            assert on
            n_o, res_o, frz_o = o.iterate(10, 0.0)
            n_g, res_g, frz_g = e.iterate(10, 0.0)
            runs.append(dict(n=n_g, res=res_g, frz=frz_g, pts=e.get_points(), err=capfd.readouterr().err))
            e.close()
        assert _shape(runs[-1]) == ((128, 128) if env else (256, 256)), runs[-1]["err"]
        _check(runs[-1], dict(n=n_o, res=res_o, frz=frz_o, pts=o.points()), runs[0])


@pytest.mark.parametrize("kind", ["hex", "cavity"])
def test_caps_on_and_below_one_elements_need(oracle_lib, monkeypatch, capfd, kind):
    """one element per tile; every cap exactly at the largest element's need (the greedy passes close a tile on '>': such an element
    still fits); a hard cap one below it -- a builder refuses, and the engine runs the direct-gather kernels (geometry /
    smoothing caps) or the untiled face-angle filter (edge caps), still matching the oracle"""
    mesh, prm, orc, base = _reference(kind, True, oracle_lib, monkeypatch, capfd)
    need = _needs(mesh)
    it = _ITERS[kind]
    # (SMGPU_GEOM_CELLS=1 alone would derive point / face caps below one hex cell's need: those stay at the defaults' values)
    one = {"SMGPU_GEOM_CELLS": 1, "SMGPU_GEOM_CAPP": 768, "SMGPU_GEOM_CAPF": 512, "SMGPU_SMOOTH_CAPTOTAL": 1, "SMGPU_EDGE_CAPTOTAL": 1}
    run = _engine(mesh, prm, it, one, monkeypatch, capfd)
    _check(run, orc, base, (256, 256))
    assert re.search(r"tiles: geom T=256 n=%d " % mesh.nCells, run["err"]) and re.search(r"smooth T=256 n=%d " % mesh.nPoints, run["err"]), run["err"]
    assert _EDGE_TILES in run["err"]
    run = _engine(mesh, prm, it, _cap_env(need), monkeypatch, capfd)
    _check(run, orc, base, (256, 256))
    assert _EDGE_TILES in run["err"]
    for key, what in (("SMGPU_GEOM_CAPP", "gp"), ("SMGPU_SMOOTH_CAPC", "sc")):
        run = _engine(mesh, prm, it, {key: need[what] - 1}, monkeypatch, capfd)
        _check(run, orc)
        assert _shape(run) is None and run["cnt"]["k_geom_tile"] == 0 and run["cnt"]["k_face_geom"] > 0, (key, run["err"])
    run = _engine(mesh, prm, it, {"SMGPU_EDGE_CAPF": need["ef"] - 1}, monkeypatch, capfd)
    _check(run, orc, base, (256, 256))
    assert _EDGE_TILES not in run["err"]


def test_deferred_finish_at_every_geometry_shape(oracle_lib, monkeypatch, capfd):
    """SMGPU_DEFER_FINISH=0 gives the default's bits; with relTol <= 0 and 64-thread geometry tiles the deferred end-of-iteration
    reduction (finishPartials<64>) gives the oracle's residual and frozen-point series exactly"""
    mesh, prm, orc, base = _reference("block", True, oracle_lib, monkeypatch, capfd)
    assert np.array_equal(base["res"], orc["res"]) and np.array_equal(base["frz"], orc["frz"])
    run = _engine(mesh, prm, _ITERS["block"], {"SMGPU_DEFER_FINISH": 0}, monkeypatch, capfd)
    _check(run, orc, base, (256, 256))
    for geomT in (64, 128):
        run = _engine(mesh, prm, _ITERS["block"], {"SMGPU_GEOM_T": geomT}, monkeypatch, capfd)
        _check(run, orc, base, (geomT, 256))
        assert np.array_equal(run["res"], orc["res"]) and np.array_equal(run["frz"], orc["frz"])


def test_local_multi_smoother_at_128_thread_tiles(oracle_lib, monkeypatch, capfd):
    """k_pack_tile<128> and the one-kernel-per-step path the shape forces (the merged launches need 256-thread tiles)"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import shared_point_table
    from smoothmesh_amd.halo import LocalMultiSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    grid, sub = (2, 2, 1), (16, 12, 12)
    subs = [hex_subdomain(sub, grid, r, jitter=0.3, seed=9) for r in range(4)]
    orcs = [oracle_lib.Oracle(s.mesh) for s in subs]
    mn = min(o.mesh_stats()[0] for o in orcs)
    prm = default_params(mn, edgeAngleConstraint=True, faceAngleConstraint=True)
    for o in orcs:
        o.set_params(prm)
    off, dom, loc = shared_point_table(subs)
    n_o, res_o, frz_o = oracle_lib.MultiOracle(orcs, off, dom, loc).iterate(8, 0.0)
    out = []
    for env in ({}, {"SMGPU_GEOM_T": "128", "SMGPU_SMOOTH_T": "128"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            mp.setenv("SMGPU_VERBOSE", "1")
            capfd.readouterr()
            ms = LocalMultiSmoother(subs, device=0, overlap=False)
            shapes = [(int(a), int(b)) for a, b in _TILES.findall(capfd.readouterr().err)]
            assert shapes == [(128, 128) if env else (256, 256)] * 4, shapes
            ms.set_params(prm)
            n_g, res_g, frz_g = ms.iterate(8, 0.0)
            assert n_o == n_g and np.array_equal(frz_o, frz_g)
            assert np.max(np.abs(res_o - res_g) / np.maximum(res_o, 1e-300)) <= 1e-10
            pts = ms.get_points()
            for o, p in zip(orcs, pts):
                assert rel_linf(p, o.points()) <= 1e-13
            out.append((res_g, frz_g, pts))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    for a, b in zip(out[0][2], out[1][2]):
        assert np.array_equal(a, b)
