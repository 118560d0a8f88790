"""The checks `checkMesh -allGeometry` adds to the quality report (include/smgpu.h smgpu_mesh_quality_geometry; definitions:
DESIGN.md "Mesh quality", 10.6): a numpy restatement of the definitions, pinned here by hand-derived answers.  Inputs as
tests/test_quality_reference.py (the oracle's face centres / area vectors / cell centres, the host build's cell -> face rows), so it
runs without a GPU; tests/test_gpu_quality_geometry.py holds the engine to it."""
import dataclasses
import math

import numpy as np
import pytest

from test_quality_reference import (ROOTVSMALL, VSMALL, _dot, _mag, cell_faces, oracle_geometry, quality_reference, tangled_block,
                                    uniform_block)

SMALL = 1e-15
GEOMETRY_DEFAULTS = dict(concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05, volRatioThreshold=0.01,
                         determinantThreshold=0.001)
COUNTS = ("nConcaveFaces", "nWarpedFaces", "nLowWeightFaces", "nLowVolRatioFaces", "nUnderdeterminedCells")


def quality_geometry_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr):
    """(report dict with the smgpu_quality_geometry field names, per-element fields dict: the five fields of
    smgpu_quality_geometry_field, plus what the well-posedness checks of the GPU test need: "_cornerSin" the sine of every corner with
    two edges longer than SMALL, "_cornerSide" (c/s).n of those, "_summed" the faces whose flatness is summed)"""
    thr = {**GEOMETRY_DEFAULTS, **thr}
    F, Fi, C = mesh.nFaces, mesh.nInternalFaces, mesh.nCells
    own, nei = mesh.owner.astype(np.int64), mesh.neighbour.astype(np.int64)[:Fi]
    magSf = _mag(fa)
    nHat = fa / (magSf + ROOTVSMALL)[:, None]
    # the corners of every face: entry j of facePoints is corner (j - faceOffsets[f]) of its face f
    fo = mesh.faceOffsets.astype(np.int64)
    nv = np.diff(fo)
    rowOf = np.repeat(np.arange(F), nv)
    first = fo[:-1][rowOf]
    local = np.arange(fo[-1]) - first
    P = mesh.points[mesh.facePoints]
    eNext = P[first + (local + 1) % nv[rowOf]] - P
    ePrev = P - P[first + (local - 1) % nv[rowOf]]
    lenN, lenP = _mag(eNext), _mag(ePrev)
    c = np.cross(ePrev / (lenP + ROOTVSMALL)[:, None], eNext / (lenN + ROOTVSMALL)[:, None])
    s = _mag(c)
    valid = (lenN > SMALL) & (lenP > SMALL)
    sinT = math.sin(math.radians(thr["concaveThreshold"]))
    side = _dot(c / np.where(s > 0, s, 1.0)[:, None], nHat[rowOf])
    concave = valid & (s >= sinT) & (side < SMALL)
    conc = np.maximum.reduceat(np.where(concave, s, 0.0), fo[:-1])
    isConcave = conc > SMALL
    # flatness
    tri = 0.5 * _mag(np.cross(eNext, fc[rowOf] - P))
    a = np.add.reduceat(tri, fo[:-1])
    summed = (nv > 3) & (magSf > ROOTVSMALL)
    flat = np.where(summed, magSf / (a + ROOTVSMALL), 1.0)
    # weight and volume ratio, internal faces
    V = quality_reference(mesh, fc, fa, cc, cfOff, cfVal)[1]["cellVolume"]
    w, r = np.ones(F), np.ones(F)
    dO = np.abs(_dot(fa[:Fi], fc[:Fi] - cc[own[:Fi]]))
    dN = np.abs(_dot(fa[:Fi], cc[nei] - fc[:Fi]))
    w[:Fi] = np.minimum(dO, dN) / ((dO + dN) + VSMALL)
    vO, vN = V[own[:Fi]], V[nei]
    r[:Fi] = np.minimum(vO, vN) / (np.maximum(vO, vN) + VSMALL)
    # cell determinant over the internal faces of every cell
    cfOff = cfOff.astype(np.int64)
    cellOf = np.repeat(np.arange(C), np.diff(cfOff))
    fid = (cfVal & 0x7fffffff).astype(np.int64)
    internal = fid < Fi
    nInt = np.add.reduceat(internal.astype(np.int64), cfOff[:-1])
    sumA = np.add.reduceat(np.where(internal, magSf[fid], 0.0), cfOff[:-1])
    avgA = sumA / np.maximum(nInt, 1)
    ok = (nInt > 0) & (avgA >= ROOTVSMALL)
    sn = np.where(internal[:, None], fa[fid], 0.0) / np.where(ok, avgA, 1.0)[cellOf][:, None]
    T = {k: np.add.reduceat(sn[:, i] * sn[:, j], cfOff[:-1]) for k, (i, j) in
         dict(xx=(0, 0), xy=(0, 1), xz=(0, 2), yy=(1, 1), yz=(1, 2), zz=(2, 2)).items()}
    det = np.abs((T["xx"] * (T["yy"] * T["zz"] - T["yz"] * T["yz"]) - T["xy"] * (T["xy"] * T["zz"] - T["yz"] * T["xz"]))
                 + T["xz"] * (T["xy"] * T["yz"] - T["yy"] * T["xz"])) / 8.0
    det = np.where(ok, det, 0.0)

    nConc, nFlat = int(isConcave.sum()), int(summed.sum())
    maxSin = float(conc.max()) if nConc else 0.0
    flatIn = np.where(summed, flat, np.inf)
    rep = dict(
        nConcaveFaces=nConc, maxConcaveSin=maxSin, maxConcaveAngle=math.degrees(np.arcsin(min(1.0, maxSin))) if nConc else 0.0,
        maxConcaveFace=int(np.argmax(np.where(isConcave, conc, -1.0))) if nConc else -1,
        minFlatness=float(flatIn.min()) if nFlat else 1.0, avgFlatness=float(flat[summed].sum() / nFlat) if nFlat else 1.0,
        nFlatnessFaces=nFlat, nWarpedFaces=int((summed & (flat < thr["flatnessThreshold"])).sum()),
        minFlatnessFace=int(np.argmin(flatIn)) if nFlat else -1,
        minFaceWeight=float(w[:Fi].min()) if Fi else 1.0, avgFaceWeight=float(w[:Fi].sum() / Fi) if Fi else 1.0,
        nLowWeightFaces=int((w[:Fi] < thr["weightThreshold"]).sum()), minFaceWeightFace=int(np.argmin(w[:Fi])) if Fi else -1,
        minVolRatio=float(r[:Fi].min()) if Fi else 1.0, avgVolRatio=float(r[:Fi].sum() / Fi) if Fi else 1.0,
        nLowVolRatioFaces=int((r[:Fi] < thr["volRatioThreshold"]).sum()), minVolRatioFace=int(np.argmin(r[:Fi])) if Fi else -1,
        minDeterminant=float(det.min()) if C else 0.0, avgDeterminant=float(det.sum() / C) if C else 0.0,
        nUnderdeterminedCells=int((det < thr["determinantThreshold"]).sum()), minDeterminantCell=int(np.argmin(det)) if C else -1,
    )
    fields = dict(faceConcavity=conc, faceFlatness=flat, faceWeight=w, faceVolumeRatio=r, cellDeterminant=det,
                  _cornerSin=s[valid], _cornerSide=side[valid], _summed=summed)
    return rep, fields


def geometry_reference_of(oracle_lib, mesh, variant="com", **thr):
    fc, fa, cc = oracle_geometry(oracle_lib, mesh, variant)
    off, val = cell_faces(mesh)
    return quality_geometry_reference(mesh, fc, fa, cc, off, val, **thr)


# ---- the meshes with hand-derived answers (also used by tests/test_gpu_quality_geometry.py) -----------------------------
def cube27():
    from smoothmesh_amd.meshgen import hex_block
    return hex_block(3)


def cube27_determinants(cc):
    """1, 0.5, 0.25, 0.125 by the number of the cell's indices that are the middle one (6, 5, 4, 3 internal faces)"""
    mid = (np.abs(cc - 0.5) < 1e-9).sum(axis=1)
    return np.array([0.125, 0.25, 0.5, 1.0])[mid]


def split_pair(a):
    """two cells [0, a] x [0, 1]^2 and [a, 2] x [0, 1]^2 (cell 0 owns the shared face, face 0)"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(2, 1, 1, lengths=(2.0, 1.0, 1.0))
    m.points = m.points.copy()
    m.points[np.isclose(m.points[:, 0], 1.0), 0] = a
    assert m.nInternalFaces == 1
    return m


def saddle_cell(h):
    """one unit cube whose top face's corners are alternately lifted and lowered by h -> (mesh, the top face)"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(1)
    m.points = m.points.copy()
    top = np.isclose(m.points[:, 2], 1.0)
    up = (np.rint(m.points[:, 0] + m.points[:, 1]).astype(int) % 2) == 0
    m.points[top & up, 2] += h
    m.points[top & ~up, 2] -= h
    fo = m.faceOffsets
    faces = [f for f in range(m.nFaces) if top[m.facePoints[fo[f]:fo[f + 1]]].all()]
    assert len(faces) == 1
    return m, faces[0]


def dented_slab():
    """hex_block(2, 2, 1), the centre column (both z levels) moved from (0.5, 0.5) to (0.9, 0.9) -> (mesh, the two z-faces of cell (1, 1))"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(2, 2, 1)
    m.points = m.points.copy()
    col = np.isclose(m.points[:, 0], 0.5) & np.isclose(m.points[:, 1], 0.5)
    assert col.sum() == 2
    m.points[col, 0] = 0.9
    m.points[col, 1] = 0.9
    fo = m.faceOffsets
    faces = []
    for f in range(m.nFaces):
        p = m.points[m.facePoints[fo[f]:fo[f + 1]]]
        if np.ptp(p[:, 2]) == 0.0 and sorted(map(tuple, np.round(p[:, :2], 9))) == [(0.5, 1.0), (0.9, 0.9), (1.0, 0.5), (1.0, 1.0)]:
            faces.append(f)
    assert len(faces) == 2
    return m, faces


# ---- known answers -------------------------------------------------------------------------------------------------
def test_uniform_cube_known_answers(oracle_lib):
    m = cube27()
    fc, fa, cc = oracle_geometry(oracle_lib, m)
    rep, f = quality_geometry_reference(m, fc, fa, cc, *cell_faces(m))
    assert np.max(np.abs(f["cellDeterminant"] - cube27_determinants(cc))) <= 1e-13
    assert sorted(np.round(f["cellDeterminant"], 6).tolist()) == [0.125] * 8 + [0.25] * 12 + [0.5] * 6 + [1.0]
    Fi = m.nInternalFaces
    assert np.max(np.abs(f["faceWeight"][:Fi] - 0.5)) <= 1e-13 and np.all(f["faceWeight"][Fi:] == 1.0)
    assert np.max(np.abs(f["faceVolumeRatio"] - 1.0)) <= 1e-13
    assert np.max(np.abs(f["faceFlatness"] - 1.0)) <= 1e-13
    assert np.all(f["faceConcavity"] == 0.0)
    assert rep["maxConcaveSin"] == 0.0 and rep["maxConcaveAngle"] == 0.0 and rep["maxConcaveFace"] == -1
    assert rep["nFlatnessFaces"] == m.nFaces
    for k in COUNTS:
        assert rep[k] == 0, k


@pytest.mark.parametrize("a", [0.5, 0.05])
def test_split_pair_known_answers(oracle_lib, a):
    m = split_pair(a)
    rep, f = geometry_reference_of(oracle_lib, m)
    w, r = min(a, 2 - a) / 2, min(a, 2 - a) / max(a, 2 - a)
    assert abs(f["faceWeight"][0] - w) <= 1e-13 and abs(rep["minFaceWeight"] - w) <= 1e-13
    assert abs(f["faceVolumeRatio"][0] - r) <= 1e-13 and abs(rep["minVolRatio"] - r) <= 1e-13
    assert rep["minFaceWeightFace"] == 0 and rep["minVolRatioFace"] == 0
    assert rep["nLowWeightFaces"] == (1 if a == 0.05 else 0)
    assert rep["nLowVolRatioFaces"] == 0
    # one internal face per cell: a rank-one tensor
    assert np.all(f["cellDeterminant"] <= 1e-30) and rep["nUnderdeterminedCells"] == 2 and rep["minDeterminantCell"] == 0


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("h", [0.5, 0.1])
def test_saddle_face_flatness(oracle_lib, variant, h):
    m, top = saddle_cell(h)
    rep, f = geometry_reference_of(oracle_lib, m, variant)
    assert abs(f["faceFlatness"][top] - 1.0 / math.sqrt(1.0 + 4.0 * h * h)) <= 1e-13
    others = np.delete(f["faceFlatness"], top)
    assert np.max(np.abs(others - 1.0)) <= 1e-13           # the side faces stay in their planes
    assert rep["nFlatnessFaces"] == 6
    if h == 0.5:
        assert abs(f["faceFlatness"][top] - 0.7071) <= 1e-4
        assert rep["nWarpedFaces"] >= 1 and rep["minFlatnessFace"] == top
    else:
        assert rep["nWarpedFaces"] == 0


def test_dented_slab_concave_faces(oracle_lib):
    m, faces = dented_slab()
    rep, f = geometry_reference_of(oracle_lib, m)
    for face in faces:
        assert abs(f["faceConcavity"][face] - 15.0 / 17.0) <= 1e-12
    assert np.all(np.delete(f["faceConcavity"], faces) == 0.0)        # no other concave face: the column's side faces are planar quads
    assert rep["nConcaveFaces"] == 2
    assert rep["maxConcaveFace"] in faces
    assert abs(rep["maxConcaveSin"] - 15.0 / 17.0) <= 1e-12
    assert abs(rep["maxConcaveAngle"] - math.degrees(math.asin(15.0 / 17.0))) <= 1e-12


def test_tangled_block_has_low_volume_ratio(oracle_lib):
    rep, f = geometry_reference_of(oracle_lib, tangled_block())
    assert rep["minVolRatio"] <= 0.0
    assert rep["nLowVolRatioFaces"] >= 1


def test_uniform_block_of_the_quality_tests(oracle_lib):
    """the 6 x 5 x 4 block of tests/test_quality_reference.py: anisotropic spacing leaves weights and ratios what they are"""
    m = uniform_block()
    rep, f = geometry_reference_of(oracle_lib, m)
    assert abs(rep["minFaceWeight"] - 0.5) <= 1e-13 and abs(rep["avgFaceWeight"] - 0.5) <= 1e-13
    assert abs(rep["minVolRatio"] - 1.0) <= 1e-12 and abs(rep["minFlatness"] - 1.0) <= 1e-13
    for k in COUNTS:
        assert rep[k] == 0, k


def test_python_mirror():
    """MeshQualityGeometry, the ctypes struct and the reference carry the same quantities; the library exports both calls"""
    from smoothmesh_amd import MeshQualityGeometry, _ffi
    from smoothmesh_amd.engine import QUALITY_GEOMETRY_FIELDS
    names = [f.name for f in dataclasses.fields(MeshQualityGeometry)]
    assert names == [n for n, _ in _ffi.QualityGeometry._fields_]
    assert [n for n, _ in _ffi.QualityGeometryParams._fields_] == list(GEOMETRY_DEFAULTS)
    m = split_pair(0.5)
    fo = m.faceOffsets
    fc = np.array([m.points[m.facePoints[fo[f]:fo[f + 1]]].mean(axis=0) for f in range(m.nFaces)])
    fa = np.array([0.5 * np.cross(p[2] - p[0], p[3] - p[1]) for p in (m.points[m.facePoints[fo[f]:fo[f + 1]]] for f in range(m.nFaces))])
    cc = np.array([[0.25, 0.5, 0.5], [1.25, 0.5, 0.5]])
    rep, f = quality_geometry_reference(m, fc, fa, cc, *cell_faces(m))
    assert sorted(names) == sorted(rep)
    assert set(QUALITY_GEOMETRY_FIELDS) == {k for k in f if not k.startswith("_")}
    assert abs(rep["minFaceWeight"] - 0.25) <= 1e-15 and abs(rep["minVolRatio"] - 1.0 / 3.0) <= 1e-15
    assert "smgpu_mesh_quality_geometry" in _ffi.SYMBOLS and "smgpu_quality_geometry_field" in _ffi.SYMBOLS
    l = _ffi.lib()                                              # the library exports both
    assert hasattr(l, "smgpu_mesh_quality_geometry") and hasattr(l, "smgpu_quality_geometry_field")


def test_formatter_lines():
    """the five lines of -allGeometry, and the block they go into: before the block's blank line, after the warning line"""
    from smoothmesh_amd import MeshQuality, MeshQualityGeometry
    from smoothmesh_amd.quality import format_geometry_lines, format_report
    g = MeshQualityGeometry(2, 15 / 17, 61.927513064147, 7, 0.25, 0.875, 20, 3, 11, 0.025, 0.4, 1, 0, 1 / 3, 0.9, 0, 0, 0.0, 0.5, 2, 0)
    lines = format_geometry_lines(g).splitlines()
    assert lines == ["    faceConcavity maxAngle 61.9275131 concave 2 maxFace 7",
                     "    faceFlatness min 0.25 average 0.875 warped 3 minFace 11",
                     "    faceWeight min 0.025 average 0.4 low 1 minFace 0",
                     "    volumeRatio min 0.333333333 average 0.9 low 0 minFace 0",
                     "    cellDeterminant min 0 average 0.5 underdetermined 2 minCell 0"]
    q = MeshQuality(*([1] * len(dataclasses.fields(MeshQuality))))
    plain, full = format_report(q, "final mesh"), format_report(q, "final mesh", g)
    assert full == plain[:-1] + format_geometry_lines(g) + "\n"
    assert plain.endswith("\n\n") and full.endswith("minCell 0\n\n")
