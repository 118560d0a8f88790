"""Mesh quality report on the GPU (include/smgpu.h smgpu_mesh_quality / smgpu_quality_field, csrc/kernels_quality.hpp) against
the numpy restatement of its definitions (tests/test_quality_reference.py), its freedom from side effects, its repeatability,
what it says about smoothing, and the `smoothMesh -checkQuality` report."""
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_quality_reference import (DEFAULTS, VSMALL, cell_faces, quality_reference, reference_of, tangled_block, two_cells,
                                    uniform_block)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
FIELDS = ("cellVolume", "cellOpenness", "cellAspectRatio", "faceNonOrthogonality", "faceSkewness")
EXACT = ("nCells", "nFaces", "nInternalFaces", "nNonPositiveVolume", "minVolumeCell", "nZeroAreaFaces", "nSevereNonOrth",
         "nErrorNonOrth", "maxNonOrthFace", "nSkewFaces", "maxSkewFace", "nWrongOrientedFaces", "nOpenCells", "nHighAspectCells")


def _engine(mesh, variant="com"):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    return e


def _assert_report(q, rep, scale_v, tol=1e-12):
    """counts and ids exactly, values to tol relative (volumes against scale_v: sum |pyramid| / 3 of the mesh)"""
    got = dataclasses.asdict(q)
    for k in EXACT:
        assert got[k] == rep[k], (k, got[k], rep[k])
    for k in ("minVolume", "maxVolume", "totalVolume"):
        assert abs(got[k] - rep[k]) <= tol * scale_v, (k, got[k], rep[k])
    for k in ("minFaceArea", "maxFaceArea", "maxNonOrth", "avgNonOrth", "maxSkewness", "maxOpenness", "maxAspectRatio"):
        assert abs(got[k] - rep[k]) <= tol * max(abs(rep[k]), 1e-300) or (k == "maxOpenness" and abs(got[k] - rep[k]) <= 1e-14), \
            (k, got[k], rep[k])


def _assert_fields(e, f, tol=1e-13):
    absPyr = f["cellAbsPyramids"]
    for name in FIELDS:
        g, r = e.quality_field(name), f[name]
        assert g.shape == r.shape, name
        if name == "cellVolume":
            err = np.max(np.abs(g - r) / absPyr)
        elif name == "cellOpenness":          # ~1e-16 values of closed cells: absolute
            err = np.max(np.abs(g - r))
        else:
            err = np.max(np.abs(g - r) / np.maximum(np.abs(r), 1.0))
        assert err <= tol, (name, err)


def _assert_well_posed(rep, f):
    """no reference element within 1e-9 of a threshold: counts and ids are then well defined"""
    cosT = math.cos(math.radians(DEFAULTS["nonOrthThreshold"]))
    o = f["faceOrtho"][:rep["nInternalFaces"]]
    assert np.min(np.abs(o - cosT)) > 1e-9 and np.min(np.abs(o)) > 1e-9
    assert np.min(np.abs(f["faceSkewness"] - DEFAULTS["skewThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellOpenness"] - DEFAULTS["closedThreshold"])) > 1e-9 * DEFAULTS["closedThreshold"]
    assert np.min(np.abs(f["cellAspectRatio"] - DEFAULTS["aspectThreshold"])) > 1e-9
    assert np.min(np.abs(f["cellVolume"]) / f["cellAbsPyramids"]) > 1e-9
    for name in ("faceNonOrthogonality", "faceSkewness"):            # no second element within 1e-9 of the maximum (ids)
        v = np.sort(f[name])
        assert v[-1] - v[-2] > 1e-9 * max(v[-1], 1.0) or v[-1] == 0.0 or rep["maxSkewness"] <= 1e-12
    v = np.sort(f["cellVolume"])
    assert v[1] - v[0] > 1e-9 * np.max(f["cellAbsPyramids"]) or np.ptp(v) <= 1e-12 * np.max(f["cellAbsPyramids"])


# ---- known answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["uniform", "two_cells_0.5", "two_cells_1", "tangled"])
def test_known_answers(oracle_lib, which):
    m = {"uniform": uniform_block, "tangled": tangled_block}[which]() if not which.startswith("two") else two_cells(float(which.split("_")[-1]))
    rep, f = reference_of(oracle_lib, m)
    e = _engine(m)
    q = e.mesh_quality()
    got = dataclasses.asdict(q)
    if which == "uniform":
        assert q.maxNonOrth == 0.0 and q.maxSkewness <= 1e-12
        assert abs(q.totalVolume - 0.96) <= 1e-13
        # ties everywhere: the lowest id wins
        assert q.maxNonOrthFace == 0
        for k in EXACT[3:]:
            if k.startswith("n"):
                assert got[k] == 0, k
    elif which == "tangled":
        assert q.nNonPositiveVolume >= 1 and q.nWrongOrientedFaces >= 1
        assert abs(q.totalVolume - 1.0) <= 1e-12
    else:
        s = float(which.split("_")[-1])
        assert abs(e.quality_field("faceNonOrthogonality")[0] - math.degrees(math.atan(s / 2))) <= 1e-12
        assert abs(e.quality_field("faceSkewness")[0] - s / 2) <= 1e-12
    for k in EXACT:
        if which == "uniform" and k in ("minVolumeCell", "maxSkewFace"):
            # equal volumes / skewness within rounding: the reference's id is a matter of the last bit, the engine's is the lowest
            # id among the elements that share the extreme of its own field
            from quality_fold_reference import engine_lowest_id
            assert got[k] == engine_lowest_id(e, m, k), (k, got[k])
            continue
        assert got[k] == rep[k], (k, got[k], rep[k])
    _assert_fields(e, f)


# ---- parity with the numpy reference ---------------------------------------------------------------------------------
CASES = [(8, 8, 8, 0.2, 1), (12, 9, 7, 0.3, 2), (5, 16, 6, 0.25, 3)]


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("nx,ny,nz,jit,seed", CASES)
def test_parity_jittered_blocks(oracle_lib, variant, nx, ny, nz, jit, seed):
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(nx, ny, nz, jitter=jit, seed=seed)
    rep, f = reference_of(oracle_lib, m, variant)
    _assert_well_posed(rep, f)
    e = _engine(m, variant)
    _assert_report(e.mesh_quality(), rep, float(f["cellAbsPyramids"].sum()))
    _assert_fields(e, f)


@pytest.mark.parametrize("variant", ["com", "org"])
def test_parity_cavity_mesh(oracle_lib, variant):
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(54, jitter=0.2, seed=9)
    assert 150_000 < m.nCells < 300_000
    rep, f = reference_of(oracle_lib, m, variant)
    _assert_well_posed(rep, f)
    e = _engine(m, variant)
    _assert_report(e.mesh_quality(), rep, float(f["cellAbsPyramids"].sum()))
    _assert_fields(e, f)


def test_parity_million_cell_block():
    """1 M cells: the reference's geometry inputs are the engine's own published fields (bit-identical to the oracle's:
    tests/test_gpu_parity.py), which keeps the oracle's set-up of a 1 M-cell mesh out of the suite's time"""
    from smoothmesh_amd import default_params
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(100, jitter=0.3, seed=11)
    e = _engine(m)
    q = e.mesh_quality()
    g = _engine(m)
    g.set_params(default_params(g.mesh_stats()[0]))
    g.debug_propose()
    fc, fa, cc = (g.debug_field(k).reshape(-1, 3) for k in ("faceCentres", "faceAreas", "cellCentres"))
    rep, f = quality_reference(m, fc, fa, cc, *cell_faces(m))
    _assert_well_posed(rep, f)
    _assert_report(q, rep, float(f["cellAbsPyramids"].sum()))
    _assert_fields(e, f)


# ---- no side effects, repeatability ----------------------------------------------------------------------------------
def test_report_leaves_the_loop_untouched():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(16, jitter=0.2, seed=3)
    runs = []
    for with_report in (False, True):
        e = _engine(m)
        e.set_params(default_params(e.mesh_stats()[0]))            # constraints on: the face-angle walk runs
        if with_report:
            n1, r1, f1 = e.iterate(5, 0.0)
            walk = e.debug_walk_mode()
            e.mesh_quality()
            for name in FIELDS:
                e.quality_field(name)
            assert e.debug_walk_mode() == walk
            n2, r2, f2 = e.iterate(5, 0.0)
            n, res, frz = n1 + n2, np.concatenate([r1, r2]), np.concatenate([f1, f2])
        else:
            n, res, frz = e.iterate(10, 0.0)
        runs.append((n, res, frz, e.get_points(), e.near_ties()))
    (na, ra, fa_, pa, ta), (nb, rb, fb, pb, tb) = runs
    assert na == nb == 10
    assert np.array_equal(ra, rb) and np.array_equal(fa_, fb)
    assert np.array_equal(pa, pb)
    assert ta == tb
    assert fa_.max() > 0                                             # the constraints did freeze points


def test_report_is_bitwise_repeatable():
    from smoothmesh_amd.polymesh import cavity_mesh
    m = cavity_mesh(30, jitter=0.2, seed=5)
    e1, e2 = _engine(m), _engine(m)
    a, b, c = e1.mesh_quality(), e1.mesh_quality(), e2.mesh_quality()
    assert a == b == c
    for name in FIELDS:
        x, y, z = e1.quality_field(name), e1.quality_field(name), e2.quality_field(name)
        assert x.tobytes() == y.tobytes() == z.tobytes(), name


# ---- what the report says about smoothing ----------------------------------------------------------------------------
def test_smoothing_lowers_average_non_orthogonality():
    from smoothmesh_amd import default_params
    from smoothmesh_amd.meshgen import hex_block
    e = _engine(hex_block(20, 20, 20, jitter=0.3))
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    before = e.mesh_quality()
    assert e.iterate(30, 0.0)[0] == 30
    after = e.mesh_quality()
    assert after.avgNonOrth < before.avgNonOrth, (before.avgNonOrth, after.avgNonOrth)


def _parse_blocks(out):
    """{"initial mesh": {...}, "final mesh": {...}} of the -checkQuality report blocks"""
    names = {"cells": "nCells", "faces": "nFaces", "internalFaces": "nInternalFaces",
             "cellVolume": dict(min="minVolume", max="maxVolume", total="totalVolume", nonPositive="nNonPositiveVolume", minCell="minVolumeCell"),
             "faceArea": dict(min="minFaceArea", max="maxFaceArea", zero="nZeroAreaFaces"),
             "nonOrthogonality": dict(max="maxNonOrth", average="avgNonOrth", severe="nSevereNonOrth", error="nErrorNonOrth", maxFace="maxNonOrthFace"),
             "skewness": dict(max="maxSkewness", severe="nSkewFaces", maxFace="maxSkewFace"),
             "facePyramids": dict(wrongOriented="nWrongOrientedFaces"),
             "cellOpenness": dict(max="maxOpenness", open="nOpenCells"),
             "cellAspectRatio": dict(max="maxAspectRatio", high="nHighAspectCells")}
    blocks = {}
    lines = out.splitlines()
    for i, line in enumerate(lines):
        mt = re.fullmatch(r"Mesh quality \((.*)\):", line)
        if not mt:
            continue
        d = {}
        for body in lines[i + 1:i + 9]:
            t = body.split()
            if t[0] == "cells":
                for k, v in zip(t[0::2], t[1::2]):
                    d[names[k]] = int(v)
                continue
            for k, v in zip(t[1::2], t[2::2]):
                key = names[t[0]][k]
                d[key] = int(v) if key.startswith("n") or key.endswith(("Face", "Cell")) else float(v)
        extra = lines[i + 9].strip() if i + 9 < len(lines) else ""
        d["_warning"] = extra if extra.startswith("***") else None
        blocks[mt.group(1)] = d
    return blocks


def _run(case, opts, check=True):
    r = subprocess.run([BIN, "-case", str(case)] + opts, capture_output=True, text=True, timeout=900)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.mark.parametrize("case", ["testcase7", "testcase2", "testcase3", "testcase4", "testcase5"])
def test_reference_command_lines_leave_no_tangled_cells(tmp_path, case):
    """the reference's testcase command lines (run_serial, verbatim options) on the stand-in meshes of
    tests/test_gpu_reference_commands.py: the final mesh has no non-positive volume and no wrongly oriented face"""
    from bnd_cases import scale_about_centre, tangential_jitter
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh, write_case
    from test_gpu_reference_commands import _geometry, _one_patch, _rename
    if case == "testcase7":
        m, opts, geo = _one_patch(hex_block(30, jitter=0.3, seed=7), "walls"), ["-centroidalIters", "100", "-layerPatches", "(walls)"], None
    elif case == "testcase2":
        m = _rename(cavity_mesh(12, jitter=0.2, seed=2), cavity="wall_sphere")
        opts, geo = ["-centroidalIters", "100", "-minEdgeLength", "0.05", "-maxStepLength", "0.05", "-layerExpansionRatio", "1.2",
                     "-maxLayers", "10", "-layerPatches", "(wall_sphere)"], None
    elif case == "testcase3":
        m = tangential_jitter(hex_block(12, jitter=0.25, seed=3), 0.02, seed=5)
        opts, geo = ["-relTol", "1e-8", "-centroidalIters", "200", "-minAngle", "15"], (12, 4, 1.03)
    elif case == "testcase4":
        m = _one_patch(tangential_jitter(hex_block(12, 12, 13, jitter=0.25, seed=4), 0.02, seed=6), "walls")
        opts = ["-centroidalIters", "200", "-layerExpansionRatio", "1.2", "-layerEdgeLength", "0.05", "-maxLayers", "3",
                "-layerPatches", "(walls)", "-smoothingPatches", '(".*")']
        geo = (10, 3, 1.02)
    else:
        m = _rename(tangential_jitter(hex_block(10, 10, 10, jitter=0.25, seed=5), 0.02, seed=7), zmax="top")
        opts = ["-centroidalIters", "500", "-minAngle", "15", "-layerExpansionRatio", "1.2", "-layerEdgeLength", "0.05", "-maxLayers", "3",
                "-layerPatches", '("top")', "-smoothingPatches", '(".*")']
        geo = (10, 3, 1.02)
    write_case(str(tmp_path), m, binary=True, writeFormat="binary")
    if geo:
        _geometry(tmp_path, geo[0], geo[1], warp=scale_about_centre(geo[2]))
    out = _run(tmp_path, opts + ["-checkQuality", "true"]).stdout
    b = _parse_blocks(out)
    assert set(b) == {"initial mesh", "final mesh"}
    assert b["final mesh"]["nNonPositiveVolume"] == 0, b["final mesh"]
    assert b["final mesh"]["nWrongOrientedFaces"] == 0, b["final mesh"]
    assert b["final mesh"]["_warning"] is None


# ---- refusal on a halo engine ----------------------------------------------------------------------------------------
def test_halo_engine_refuses():
    import socket
    import torch.distributed as dist
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        ds = DistributedSmoother(hex_subdomain((8, 7, 6), (1, 1, 1), 0, jitter=0.3, seed=5), device=0)
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.mesh_quality()
        with pytest.raises(SmgpuError, match="halo"):
            ds.engine.quality_field("cellVolume")
    finally:
        dist.destroy_process_group()


# ---- command line ----------------------------------------------------------------------------------------------------
def test_cli_check_quality(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    m = hex_block(9, 8, 7, jitter=0.3, seed=4)
    write_case(str(tmp_path / "a"), m, binary=True, writeFormat="binary")
    write_case(str(tmp_path / "b"), m, binary=True, writeFormat="binary")
    out = _run(tmp_path / "a", ["-centroidalIters", "8", "-relTol", "0", "-checkQuality", "true"]).stdout
    b = _parse_blocks(out)
    assert list(b) == ["initial mesh", "final mesh"]
    assert out.index("Mesh includes a total of") < out.index("Mesh quality (initial mesh):") < out.index("Smoothing iteration=1 ")
    assert out.index("Writing new mesh to time 8") < out.index("Mesh quality (final mesh):") < out.index("ClockTime")
    q = dataclasses.asdict(_engine(m).mesh_quality())
    for k, v in b["initial mesh"].items():
        if k == "_warning":
            assert v is None
        elif isinstance(v, int):
            assert v == q[k], (k, v, q[k])
        else:
            assert float(f"{q[k]:.9g}") == v, (k, v, q[k])
    plain = _run(tmp_path / "b", ["-centroidalIters", "8", "-relTol", "0"]).stdout
    assert "Mesh quality" not in plain
    r = _run(tmp_path / "b", ["-parallel", "-checkQuality", "true"], check=False)
    assert r.returncode != 0
    assert "-checkQuality is not available with -parallel" in r.stdout + r.stderr
