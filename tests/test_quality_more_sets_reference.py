"""The findings of the -allGeometry checks and of the motion criteria as sets (include/smgpu.h smgpu_quality_geometry_sets /
smgpu_quality_motion_sets; DESIGN.md "Mesh quality", 10.9): numpy restatements of set membership on top of
test_quality_geometry_reference.quality_geometry_reference and test_quality_motion_reference.quality_motion_reference, pinned by
hand-derived answers, and the tables, the set writer and the command-line handling that need no GPU.
tests/test_gpu_quality_more_sets*.py hold the engine to these restatements."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from test_quality_geometry_reference import (GEOMETRY_DEFAULTS, SMALL, cube27, dented_slab, quality_geometry_reference, saddle_cell)
from test_quality_motion_reference import MOTION_DEFAULTS, quality_motion_reference
from test_quality_reference import cell_faces, oracle_geometry, tangled_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
GEOMETRY_NAMES = ("concaveFaces", "warpedFaces", "lowWeightFaces", "lowVolRatioFaces", "underdeterminedCells")
MOTION_NAMES = ("lowQualityTetFaces", "noBasePointFaces", "twistedFaces", "lowTriangleTwistFaces")


def _ids(member):
    return np.flatnonzero(member).astype(np.int32)


def geometry_sets_of_fields(mesh, f, **thr):
    """{name: ascending ids} from the fields of quality_geometry_reference: the predicates of the report's counts"""
    thr = {**GEOMETRY_DEFAULTS, **thr}
    internal = np.arange(mesh.nFaces) < mesh.nInternalFaces
    sets = dict(
        concaveFaces=_ids(f["faceConcavity"] > SMALL),
        warpedFaces=_ids(f["_summed"] & (f["faceFlatness"] < thr["flatnessThreshold"])),
        lowWeightFaces=_ids(internal & (f["faceWeight"] < thr["weightThreshold"])),
        lowVolRatioFaces=_ids(internal & (f["faceVolumeRatio"] < thr["volRatioThreshold"])),
        underdeterminedCells=_ids(f["cellDeterminant"] < thr["determinantThreshold"]),
    )
    return {k: sets[k] for k in GEOMETRY_NAMES}


def motion_sets_of_fields(f, **thr):
    """{name: ascending ids} from the fields of quality_motion_reference: the predicates of the report's counts"""
    thr = {**MOTION_DEFAULTS, **thr}
    sets = dict(
        lowQualityTetFaces=_ids(f["faceTetQuality"] < thr["tetThreshold"]),
        noBasePointFaces=_ids(f["faceBaseTetQuality"] < thr["tetThreshold"]),
        twistedFaces=_ids(f["_summed"] & (f["faceTwist"] < thr["twistThreshold"])),
        lowTriangleTwistFaces=_ids(f["_summed"] & (f["faceTriangleTwist"] < thr["triangleTwistThreshold"])),
    )
    return {k: sets[k] for k in MOTION_NAMES}


def quality_geometry_sets_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr):
    """(report, fields, {name: ascending ids}); the concavity field is the one under thr's concaveThreshold"""
    rep, f = quality_geometry_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr)
    return rep, f, geometry_sets_of_fields(mesh, f, **thr)


def quality_motion_sets_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr):
    """(report, fields, {name: ascending ids})"""
    rep, f = quality_motion_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr)
    return rep, f, motion_sets_of_fields(f, **thr)


def geometry_sets_reference_of(oracle_lib, mesh, variant="com", **thr):
    fc, fa, cc = oracle_geometry(oracle_lib, mesh, variant)
    return quality_geometry_sets_reference(mesh, fc, fa, cc, *cell_faces(mesh), **thr)


def motion_sets_reference_of(oracle_lib, mesh, variant="com", **thr):
    fc, fa, cc = oracle_geometry(oracle_lib, mesh, variant)
    return quality_motion_sets_reference(mesh, fc, fa, cc, *cell_faces(mesh), **thr)


def assert_sizes_are_counts(sets, rep, table):
    """every set of `table` (QUALITY_GEOMETRY_SETS / QUALITY_MOTION_SETS) has the size of the report's count(s)"""
    assert list(sets) == [name for name, *_ in table]
    for name, _, counts, _ in table:
        assert len(sets[name]) == sum(int(rep[c]) for c in counts), name


def _both(oracle_lib, mesh, variant="com", gthr=None, mthr=None):
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS
    grep, _, g = geometry_sets_reference_of(oracle_lib, mesh, variant, **(gthr or {}))
    mrep, _, t = motion_sets_reference_of(oracle_lib, mesh, variant, **(mthr or {}))
    assert_sizes_are_counts(g, grep, QUALITY_GEOMETRY_SETS)
    assert_sizes_are_counts(t, mrep, QUALITY_MOTION_SETS)
    for s in list(g.values()) + list(t.values()):
        assert s.dtype == np.int32 and np.all(np.diff(s) > 0)
    return g, t


# ---- hand-derived answers ----------------------------------------------------------------------------------------------
def test_uniform_cube_has_nine_empty_sets(oracle_lib):
    g, t = _both(oracle_lib, cube27())
    assert all(len(v) == 0 for v in g.values()) and all(len(v) == 0 for v in t.values())


def test_dented_slab_concave_faces_are_the_set(oracle_lib):
    m, faces = dented_slab()
    g, _ = _both(oracle_lib, m)
    assert g["concaveFaces"].tolist() == sorted(faces)


@pytest.mark.parametrize("variant", ["com", "org"])
def test_saddle_top_face_is_warped_and_twisted(oracle_lib, variant):
    m, top = saddle_cell(0.5)                      # flatness and twist 1 / sqrt 2, triangle twist 1 / 2
    g, t = _both(oracle_lib, m, variant)
    assert g["warpedFaces"].tolist() == [top]
    assert len(t["twistedFaces"]) == 0 and len(t["lowTriangleTwistFaces"]) == 0          # 0.707 > 0.02; triangle twist is off
    _, t = _both(oracle_lib, m, variant, mthr=dict(twistThreshold=0.75, triangleTwistThreshold=0.6))
    assert t["twistedFaces"].tolist() == [top] and t["lowTriangleTwistFaces"].tolist() == [top]
    _, t = _both(oracle_lib, m, variant, mthr=dict(twistThreshold=0.70, triangleTwistThreshold=0.49))
    assert top not in t["twistedFaces"] and top not in t["lowTriangleTwistFaces"]


def test_tangled_block_sets(oracle_lib):
    g, t = _both(oracle_lib, tangled_block())
    assert len(g["lowVolRatioFaces"]) > 0
    assert len(t["lowQualityTetFaces"]) > 0 and len(t["noBasePointFaces"]) > 0
    assert np.all(g["lowVolRatioFaces"] < tangled_block().nInternalFaces)


def test_sizes_equal_the_counts_at_other_thresholds(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(7, 6, 5, jitter=0.45, seed=11)
    g, t = _both(oracle_lib, m, gthr=dict(flatnessThreshold=0.99, weightThreshold=0.45, volRatioThreshold=0.8, determinantThreshold=0.3),
                 mthr=dict(tetThreshold=0.3, twistThreshold=0.95, triangleTwistThreshold=0.95))
    for k in GEOMETRY_NAMES[1:]:
        assert len(g[k]) > 0, k
    for k in MOTION_NAMES:
        assert len(t[k]) > 0, k


# ---- the public names ----------------------------------------------------------------------------------------------
def test_tables_name_fields_of_their_dataclasses():
    from smoothmesh_amd.engine import (MeshQualityGeometry, MeshQualityMotion, QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS, QUALITY_SETS)
    from smoothmesh_amd import quality
    assert quality.QUALITY_GEOMETRY_SETS is QUALITY_GEOMETRY_SETS and quality.QUALITY_MOTION_SETS is QUALITY_MOTION_SETS
    assert tuple(n for n, *_ in QUALITY_GEOMETRY_SETS) == GEOMETRY_NAMES
    assert tuple(n for n, *_ in QUALITY_MOTION_SETS) == MOTION_NAMES
    assert [c for _, c, *_ in QUALITY_GEOMETRY_SETS] == ["faceSet"] * 4 + ["cellSet"]
    assert [c for _, c, *_ in QUALITY_MOTION_SETS] == ["faceSet"] * 4
    assert [c for _, _, c, _ in QUALITY_GEOMETRY_SETS] == [("nConcaveFaces",), ("nWarpedFaces",), ("nLowWeightFaces",),
                                                          ("nLowVolRatioFaces",), ("nUnderdeterminedCells",)]
    assert [c for _, _, c, _ in QUALITY_MOTION_SETS] == [("nLowTetFaces",), ("nNoBasePointFaces",), ("nLowTwistFaces",),
                                                        ("nLowTriangleTwistFaces",)]
    for table, cls in ((QUALITY_GEOMETRY_SETS, MeshQualityGeometry), (QUALITY_MOTION_SETS, MeshQualityMotion)):
        names = {f.name for f in dataclasses.fields(cls)}
        for row in table:
            assert len(row) == 4 and set(row[2]) <= names and isinstance(row[3], str) and row[3]
    every = [n for n, *_ in QUALITY_SETS + QUALITY_GEOMETRY_SETS + QUALITY_MOTION_SETS]
    assert len(set(every)) == 16                                       # one sets/ directory holds all three tables


def test_symbols_are_declared_and_exported():
    from smoothmesh_amd import _ffi
    header = open(os.path.join(ROOT, "include", "smgpu.h")).read()
    for name in ("smgpu_quality_geometry_sets", "smgpu_quality_motion_sets", "smgpu_quality_coupled_geometry_sets",
                 "smgpu_quality_coupled_motion_sets"):
        assert re.search(r"\bint " + name + r"\(smgpu_handle\*", header), name
        assert name in _ffi.SYMBOLS
        assert hasattr(_ffi.lib(), name)
    # the seven-set declarations are as they were
    assert "int smgpu_quality_sets(smgpu_handle* h, const smgpu_quality_params* p, int64_t counts[7], int32_t* ids, int64_t cap);" in header
    from smoothmesh_amd import SmoothEngine
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    for cls in (SmoothEngine, DistributedSmoother, LocalMultiSmoother):
        assert hasattr(cls, "quality_geometry_sets") and hasattr(cls, "quality_motion_sets")
    assert hasattr(SmoothEngine, "quality_coupled_geometry_sets") and hasattr(SmoothEngine, "quality_coupled_motion_sets")


# ---- the set writer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary,compressed", [(False, False), (True, False), (False, True)])
def test_write_quality_sets_round_trips_the_new_tables(tmp_path, binary, compressed):
    from smoothmesh_amd.polymesh import read_label_list, set_write_compression
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS, write_quality_sets
    pm = tmp_path / "3" / "polyMesh"
    os.makedirs(pm)
    g = {k: np.zeros(0, np.int32) for k in GEOMETRY_NAMES}
    g["warpedFaces"] = np.array([2, 9, 70000], np.int32)
    g["underdeterminedCells"] = np.arange(1, 200, 3, dtype=np.int32)
    t = {k: np.zeros(0, np.int32) for k in MOTION_NAMES}
    t["noBasePointFaces"] = np.array([5], np.int32)
    set_write_compression(compressed)
    try:
        wg = write_quality_sets(str(pm), "3/polyMesh", g, binary=binary, table=QUALITY_GEOMETRY_SETS)
        wt = write_quality_sets(str(pm), "3/polyMesh", t, binary, QUALITY_MOTION_SETS)
        # the default table ignores names it does not hold
        assert write_quality_sets(str(pm), "3/polyMesh", g, binary) == []
    finally:
        set_write_compression(False)
    assert wg == [("warpedFaces", 3), ("underdeterminedCells", len(g["underdeterminedCells"]))]
    assert wt == [("noBasePointFaces", 1)]
    sfx = ".gz" if compressed else ""
    assert sorted(os.listdir(pm / "sets")) == sorted(n + sfx for n in ("warpedFaces", "underdeterminedCells", "noBasePointFaces"))
    from test_quality_sets_reference import _header
    for name, cls, want in (("warpedFaces", "faceSet", g), ("underdeterminedCells", "cellSet", g), ("noBasePointFaces", "faceSet", t)):
        h = " ".join(_header(str(pm / "sets" / name) + sfx).split())
        assert f"class {cls};" in h and "3/polyMesh/sets" in h and name in h and ("binary" in h) == binary
        assert np.array_equal(read_label_list(str(pm / "sets" / name)), want[name])


def test_write_quality_sets_writes_nothing_for_empty_new_sets(tmp_path):
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS, write_quality_sets
    pm = tmp_path / "constant" / "polyMesh"
    os.makedirs(pm)
    assert write_quality_sets(str(pm), "constant/polyMesh", {k: np.zeros(0, np.int32) for k in GEOMETRY_NAMES}, table=QUALITY_GEOMETRY_SETS) == []
    assert write_quality_sets(str(pm), "constant/polyMesh", {k: np.zeros(0, np.int32) for k in MOTION_NAMES}, table=QUALITY_MOTION_SETS) == []
    assert not os.path.exists(pm / "sets")


def test_sets_written_lines_of_the_new_tables():
    from smoothmesh_amd.check_quality import format_written
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS, format_sets_written
    gw = {n: w for n, _, _, w in QUALITY_GEOMETRY_SETS}
    mw = {n: w for n, _, _, w in QUALITY_MOTION_SETS}
    assert format_sets_written([("warpedFaces", 412)], QUALITY_GEOMETRY_SETS) == f"    <<Writing 412 {gw['warpedFaces']} to set warpedFaces\n"
    assert format_sets_written([("twistedFaces", 2), ("lowTriangleTwistFaces", 1)], table=QUALITY_MOTION_SETS) == (
        f"    <<Writing 2 {mw['twistedFaces']} to set twistedFaces\n"
        f"    <<Writing 1 {mw['lowTriangleTwistFaces']} to set lowTriangleTwistFaces\n")
    assert format_sets_written([("zeroVolumeCells", 3)]) == "    <<Writing 3 zero or negative volume cells to set zeroVolumeCells\n"
    assert format_written([(None, "skewFaces", 2), (None, "underdeterminedCells", 7), (1, "lowQualityTetFaces", 37)]) == (
        "    <<Writing 2 skew faces to set skewFaces\n"
        f"    <<Writing 7 {gw['underdeterminedCells']} to set underdeterminedCells\n"
        f"    <<Writing 37 {mw['lowQualityTetFaces']} to set lowQualityTetFaces in processor1\n")


def test_front_end_words_match_the_tables():
    """smoothMesh prints the same names and words as the Python tables"""
    from smoothmesh_amd.quality import QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS
    src = open(os.path.join(ROOT, "smoothmesh_amd", "csrc", "host", "smoothMesh_main.cpp")).read()
    for name, _, _, words in QUALITY_GEOMETRY_SETS + QUALITY_MOTION_SETS:
        assert f'"{name}"' in src and f'"{words}"' in src, name


# ---- refusals that stay ------------------------------------------------------------------------------------------------
def test_cli_parallel_refusals_stay(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))
    r = subprocess.run([BIN, "-case", str(tmp_path / "a"), "-parallel", "-writeSets", "true", "-allGeometry", "true"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "-writeSets is not available with -parallel: it writes the sets of the -checkQuality report, which is serial only" in r.stdout + r.stderr
    r = subprocess.run([BIN, "-case", str(tmp_path / "a"), "-parallel", "-meshQuality", "true"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-meshQuality is not available with -parallel" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    assert "with -allGeometry / -meshQuality also the sets of those reports" in h.stdout


def test_check_quality_parallel_spellings_stay_refused():
    from smoothmesh_amd import check_quality
    for opt, msg in (("-allGeometry", check_quality.ALL_GEOMETRY_PARALLEL_REFUSAL), ("-meshQuality", check_quality.MESH_QUALITY_PARALLEL_REFUSAL)):
        with pytest.raises(SystemExit) as e:
            check_quality.main(["-case", "c", "-parallel", "-writeSets", opt])
        assert str(e.value) == msg
