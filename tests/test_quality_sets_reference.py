"""The failing elements of the quality report as sets (include/smgpu.h smgpu_quality_sets; DESIGN.md "Mesh quality", 10.5): a numpy
restatement of set membership on top of test_quality_reference.quality_reference, pinned by hand-derived answers, and the set
writer and the command-line handling that need no GPU.  tests/test_gpu_quality_sets*.py hold the engine to this restatement."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from test_quality_reference import (DEFAULTS, VSMALL, _dot, _mag, cell_faces, oracle_geometry, quality_reference, shared_face,
                                    tangled_block, two_cells, uniform_block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")
NAMES = ("nonOrthoFaces", "skewFaces", "wrongOrientedFaces", "zeroAreaFaces", "zeroVolumeCells", "nonClosedCells",
         "highAspectRatioCells")


def quality_sets_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr):
    """(report, fields, {name: ascending ids}) with the membership predicates of the report's counts"""
    thr = {**DEFAULTS, **thr}
    rep, f = quality_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr)
    Fi = mesh.nInternalFaces
    own, nei = mesh.owner.astype(np.int64), mesh.neighbour.astype(np.int64)
    ortho = f["faceOrtho"][:Fi]
    cosT = math.cos(math.radians(thr["nonOrthThreshold"]))
    wrong = _dot(fa, fc - cc[own]) <= 0.0
    wrong[:Fi] |= _dot(fa[:Fi], cc[nei] - fc[:Fi]) <= 0.0
    member = dict(
        nonOrthoFaces=((ortho > 0.0) & (ortho < cosT)) | (ortho <= 0.0),
        skewFaces=f["faceSkewness"] > thr["skewThreshold"],
        wrongOrientedFaces=wrong,
        zeroAreaFaces=_mag(fa) <= VSMALL,
        zeroVolumeCells=f["cellVolume"] <= VSMALL,
        nonClosedCells=f["cellOpenness"] > thr["closedThreshold"],
        highAspectRatioCells=f["cellAspectRatio"] > thr["aspectThreshold"],
    )
    return rep, f, {k: np.flatnonzero(member[k]).astype(np.int32) for k in NAMES}


def sets_reference_of(oracle_lib, mesh, variant="com", **thr):
    fc, fa, cc = oracle_geometry(oracle_lib, mesh, variant)
    off, val = cell_faces(mesh)
    return quality_sets_reference(mesh, fc, fa, cc, off, val, **thr)


def assert_sizes_are_counts(sets, rep):
    from smoothmesh_amd.quality import QUALITY_SETS
    for name, _, counts, _ in QUALITY_SETS:
        assert len(sets[name]) == sum(int(rep[c]) for c in counts), name


def _cell_centres_of(mesh):
    """vertex mean of every cell (enough to locate the cells of a hex block)"""
    out = np.zeros((mesh.nCells, 3)); n = np.zeros(mesh.nCells)
    fo = mesh.faceOffsets
    for f in range(mesh.nFaces):
        p = mesh.points[mesh.facePoints[fo[f]:fo[f + 1]]].mean(axis=0)
        for c in ([mesh.owner[f]] + ([mesh.neighbour[f]] if f < mesh.nInternalFaces else [])):
            out[c] += p; n[c] += 1
    return out / n[:, None]


# ---- hand-derived answers ----------------------------------------------------------------------------------------------
def test_uniform_block_has_empty_sets(oracle_lib):
    m = uniform_block()
    rep, _, sets = sets_reference_of(oracle_lib, m)
    assert all(len(sets[k]) == 0 for k in NAMES)
    assert_sizes_are_counts(sets, rep)


def test_tangled_block_sets(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    m = tangled_block()
    rep, _, sets = sets_reference_of(oracle_lib, m)
    assert_sizes_are_counts(sets, rep)
    folded = int(np.argmin(np.abs(_cell_centres_of(hex_block(4)) - 0.375).sum(axis=1)))
    assert folded in sets["zeroVolumeCells"]
    # the moved point: the only one that differs from the uniform block
    p = int(np.flatnonzero(np.any(m.points != hex_block(4).points, axis=1))[0])
    fo = m.faceOffsets
    touching = {int(f) for f in range(m.nFaces) if p in m.facePoints[fo[f]:fo[f + 1]]}
    cells = {int(m.owner[f]) for f in touching} | {int(m.neighbour[f]) for f in touching if f < m.nInternalFaces}
    faces_of_cells = {f for f in range(m.nFaces) if m.owner[f] in cells or (f < m.nInternalFaces and m.neighbour[f] in cells)}
    assert len(sets["wrongOrientedFaces"]) > 0
    assert set(sets["wrongOrientedFaces"].tolist()) <= faces_of_cells
    assert set(sets["zeroVolumeCells"].tolist()) <= cells


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_two_cells_threshold_edges(oracle_lib, s):
    m = two_cells(s)
    fs = shared_face(m)
    theta, skew = math.degrees(math.atan(s / 2)), s / 2
    _, _, below = sets_reference_of(oracle_lib, m, nonOrthThreshold=theta - 1e-6, skewThreshold=skew - 1e-9)
    _, _, above = sets_reference_of(oracle_lib, m, nonOrthThreshold=theta + 1e-6, skewThreshold=skew + 1e-9)
    assert fs in below["nonOrthoFaces"] and fs in below["skewFaces"]
    assert fs not in above["nonOrthoFaces"] and fs not in above["skewFaces"]
    assert len(above["nonOrthoFaces"]) == 0                       # the only internal face
    assert len(below["wrongOrientedFaces"]) == 0 and len(below["zeroVolumeCells"]) == 0


def test_sets_are_ascending_and_equal_the_counts_at_other_thresholds(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(7, 6, 5, jitter=0.45, seed=11)
    thr = dict(nonOrthThreshold=20.0, skewThreshold=0.3, aspectThreshold=2.0, closedThreshold=1e-18)
    rep, _, sets = sets_reference_of(oracle_lib, m, **thr)
    assert_sizes_are_counts(sets, rep)
    assert len(sets["nonOrthoFaces"]) > 0 and len(sets["skewFaces"]) > 0 and len(sets["highAspectRatioCells"]) > 0
    for k in NAMES:
        assert np.all(np.diff(sets[k]) > 0), k


# ---- the public names ----------------------------------------------------------------------------------------------
def test_quality_sets_table_and_symbols():
    from smoothmesh_amd import _ffi
    from smoothmesh_amd.quality import QUALITY_SETS
    assert tuple(n for n, *_ in QUALITY_SETS) == NAMES
    assert [c for _, c, *_ in QUALITY_SETS] == ["faceSet"] * 4 + ["cellSet"] * 3
    assert QUALITY_SETS[0][2] == ("nSevereNonOrth", "nErrorNonOrth")
    for name in ("smgpu_quality_sets", "smgpu_quality_coupled_sets"):
        assert name in _ffi.SYMBOLS
        assert hasattr(_ffi.lib(), name)


# ---- the set writer --------------------------------------------------------------------------------------------------
def _header(path):
    raw = open(path, "rb").read()
    if path.endswith(".gz"):
        raw = gzip.decompress(raw)
    return raw[:raw.index(b"}") + 1].decode()


@pytest.mark.parametrize("binary,compressed", [(False, False), (True, False), (False, True), (True, True)])
def test_write_quality_sets_round_trip(tmp_path, binary, compressed):
    from smoothmesh_amd.polymesh import read_label_list, set_write_compression
    from smoothmesh_amd.quality import write_quality_sets
    pm = tmp_path / "0.5" / "polyMesh"
    os.makedirs(pm / "sets")
    (pm / "sets" / "mySet").write_text("keep me")
    sets = {k: np.zeros(0, np.int32) for k in NAMES}
    sets["skewFaces"] = np.array([3, 17, 40000], np.int32)
    sets["highAspectRatioCells"] = np.arange(0, 300, 7, dtype=np.int32)
    set_write_compression(compressed)
    try:
        written = write_quality_sets(str(pm), "0.5/polyMesh", sets, binary=binary)
    finally:
        set_write_compression(False)
    assert written == [("skewFaces", 3), ("highAspectRatioCells", len(sets["highAspectRatioCells"]))]
    sfx = ".gz" if compressed else ""
    assert sorted(os.listdir(pm / "sets")) == sorted(["mySet", "skewFaces" + sfx, "highAspectRatioCells" + sfx])
    assert (pm / "sets" / "mySet").read_text() == "keep me"
    for name, cls in (("skewFaces", "faceSet"), ("highAspectRatioCells", "cellSet")):
        path = str(pm / "sets" / name) + sfx
        h = _header(path)
        assert f"class       {cls};" in h or f"class {cls};" in " ".join(h.split()).replace(" ;", ";"), h
        assert "0.5/polyMesh/sets" in h and f"object" in h and name in h
        assert ("binary" in h) == binary
        assert np.array_equal(read_label_list(str(pm / "sets" / name)), sets[name])


def test_write_quality_sets_writes_nothing_for_empty_sets(tmp_path):
    from smoothmesh_amd.quality import write_quality_sets
    pm = tmp_path / "constant" / "polyMesh"
    os.makedirs(pm)
    assert write_quality_sets(str(pm), "constant/polyMesh", {k: np.zeros(0, np.int32) for k in NAMES}) == []
    assert not os.path.exists(pm / "sets")


def test_sets_written_lines():
    from smoothmesh_amd.check_quality import format_written
    from smoothmesh_amd.quality import format_sets_written
    assert format_sets_written([("zeroVolumeCells", 3)]) == "    <<Writing 3 zero or negative volume cells to set zeroVolumeCells\n"
    assert format_written([(None, "skewFaces", 2), (1, "nonOrthoFaces", 5)]) == (
        "    <<Writing 2 skew faces to set skewFaces\n"
        "    <<Writing 5 non-orthogonal faces to set nonOrthoFaces in processor1\n")


# ---- check_quality -writeSets argument handling ------------------------------------------------------------------------
def test_check_quality_write_sets_arguments(monkeypatch, capsys):
    from smoothmesh_amd import check_quality
    from smoothmesh_amd.engine import MeshQuality
    import dataclasses
    q = MeshQuality(**{f.name: 0 for f in dataclasses.fields(MeshQuality)})
    calls = []

    def fake(case, parallel=False, time=None, device=0, write_sets=False):
        calls.append((case, parallel, time, write_sets))
        return (q, [(None, "skewFaces", 4)]) if write_sets else q

    monkeypatch.setattr(check_quality, "case_quality", fake)
    assert check_quality.main(["-case", "c", "-writeSets"]) == 0
    out = capsys.readouterr().out
    assert calls[-1] == ("c", False, None, True)
    block, tail = out.split("\n\n", 1)
    assert block.startswith("Mesh quality (mesh):") and len(block.splitlines()) == 9
    assert tail == "    <<Writing 4 skew faces to set skewFaces\n"
    assert check_quality.main(["-case", "c", "-parallel", "-time", "2"]) == 0
    assert calls[-1] == ("c", True, "2", False)
    assert "<<Writing" not in capsys.readouterr().out


def test_check_quality_control_dict(tmp_path):
    from smoothmesh_amd.check_quality import _control
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(2, 2, 2), writeFormat="binary", writeCompression=True)
    write_case(str(tmp_path / "b"), hex_block(2, 2, 2))
    assert _control(str(tmp_path / "a")) == (True, True)
    assert _control(str(tmp_path / "b")) == (False, False)
    assert _control(str(tmp_path / "missing")) == (False, False)


# ---- smoothMesh -writeSets: refusals before any device work ------------------------------------------------------------
def test_cli_write_sets_refusals(tmp_path):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    write_case(str(tmp_path / "a"), hex_block(3, 3, 3))
    before = sorted(os.listdir(tmp_path / "a"))
    r = subprocess.run([BIN, "-case", str(tmp_path / "a"), "-writeSets", "true"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-writeSets needs -checkQuality true" in r.stdout + r.stderr
    r = subprocess.run([BIN, "-case", str(tmp_path / "a"), "-parallel", "-writeSets", "true"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-writeSets is not available with -parallel" in r.stdout + r.stderr
    r = subprocess.run([BIN, "-case", str(tmp_path / "a"), "-writeSets", "maybe"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Bad bool value for option -writeSets" in r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "a")) == before
    h = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=120)
    assert "-writeSets" in h.stdout
