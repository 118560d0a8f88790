"""Mesh quality report (include/smgpu.h smgpu_mesh_quality; definitions: DESIGN.md "Mesh quality"): a numpy restatement of the
definitions, pinned here by hand-derived answers.  It takes the face centres / area vectors and cell centres from the oracle and
the cell -> face rows from the host addressing build, so it runs without a GPU; tests/test_gpu_quality.py holds the engine to it."""
import math

import numpy as np
import pytest

VSMALL = 1e-300
ROOTVSMALL = 1e-150
DEFAULTS = dict(nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _mag(a):
    return np.sqrt(_dot(a, a))


def oracle_geometry(oracle_lib, mesh, variant="com"):
    """(C_f, S_f, C_c) of the mesh's points as the oracle's restatement of the loop computes them"""
    from smoothmesh_amd import default_params
    o = oracle_lib.Oracle(mesh)
    o.set_foam_variant(variant)
    o.set_params(default_params(o.mesh_stats()[0]))
    o.phaseA()
    return tuple(o.field(k).reshape(-1, 3) for k in ("faceCentres", "faceAreas", "cellCentres"))


def cell_faces(mesh):
    from smoothmesh_amd.engine import HostTopology
    t = HostTopology(mesh)
    off, val = t.addressing("cellFacesGeom")
    t.close()
    return off, val


def quality_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr):
    """(report dict with the smgpu_quality field names, per-element fields dict incl. "cellAbsPyramids" = sum |pyramid| / 3)"""
    thr = {**DEFAULTS, **thr}
    F, Fi, C = mesh.nFaces, mesh.nInternalFaces, mesh.nCells
    own, nei = mesh.owner.astype(np.int64), mesh.neighbour.astype(np.int64)
    pts = mesh.points
    magSf = _mag(fa)
    CO = cc[own]
    Cpf = fc - CO
    # non-orthogonality, internal faces
    d = np.empty((F, 3))
    d[:Fi] = cc[nei] - CO[:Fi]
    Sfi = fa[:Fi]
    ortho = _dot(d[:Fi], Sfi) / (_mag(d[:Fi]) * magSf[:Fi] + VSMALL)
    theta = np.degrees(np.arccos(np.clip(ortho, -1.0, 1.0)))
    faceNO = np.zeros(F)
    faceNO[:Fi] = theta
    # skewness
    n = fa[Fi:] / (magSf[Fi:] + ROOTVSMALL)[:, None]
    d[Fi:] = _dot(n, Cpf[Fi:])[:, None] * n
    sv = Cpf - (_dot(fa, Cpf) / (_dot(fa, d) + ROOTVSMALL))[:, None] * d
    magSv = _mag(sv)
    sHat = sv / (magSv + ROOTVSMALL)[:, None]
    fo = mesh.faceOffsets.astype(np.int64)
    rowOf = np.repeat(np.arange(F), np.diff(fo))
    proj = np.abs(_dot(np.repeat(sHat, np.diff(fo), axis=0), pts[mesh.facePoints] - fc[rowOf]))
    fd = np.maximum(0.2 * _mag(d) + ROOTVSMALL, np.maximum.reduceat(proj, fo[:-1]))
    skew = magSv / fd
    # face pyramids
    pO = _dot(fa, Cpf)
    wrong = pO <= 0.0
    wrong[:Fi] |= _dot(Sfi, cc[nei] - fc[:Fi]) <= 0.0
    # cells
    cfOff = cfOff.astype(np.int64)
    cnt = np.diff(cfOff)
    cellOf = np.repeat(np.arange(C), cnt)
    fid = (cfVal & 0x7fffffff).astype(np.int64)
    sgn = np.where(cfVal < 0, -1.0, 1.0)
    cEst = np.add.reduceat(fc[fid], cfOff[:-1], axis=0) / cnt[:, None]
    pyr = sgn * _dot(fa[fid], fc[fid] - cEst[cellOf])
    V = (1.0 / 3.0) * np.add.reduceat(pyr, cfOff[:-1])
    absPyr = (1.0 / 3.0) * np.add.reduceat(np.abs(pyr), cfOff[:-1])
    sumS = np.add.reduceat(sgn[:, None] * fa[fid], cfOff[:-1], axis=0)
    M = np.add.reduceat(np.abs(fa[fid]), cfOff[:-1], axis=0)
    openness = np.max(np.abs(sumS) / (M + ROOTVSMALL), axis=1)
    ar = np.maximum(M.max(axis=1) / (M.min(axis=1) + ROOTVSMALL),
                    ((1.0 / 6.0) * ((M[:, 0] + M[:, 1]) + M[:, 2])) / np.maximum(V, ROOTVSMALL) ** (2.0 / 3.0))
    cosT = math.cos(math.radians(thr["nonOrthThreshold"]))
    rep = dict(
        nCells=C, nFaces=F, nInternalFaces=Fi,
        minVolume=float(V.min()), maxVolume=float(V.max()), totalVolume=float(V.sum()),
        nNonPositiveVolume=int((V <= VSMALL).sum()), minVolumeCell=int(np.argmin(V)),
        minFaceArea=float(magSf.min()), maxFaceArea=float(magSf.max()), nZeroAreaFaces=int((magSf <= VSMALL).sum()),
        maxNonOrth=float(theta.max()) if Fi else 0.0, avgNonOrth=float(theta.sum() / Fi) if Fi else 0.0,
        nSevereNonOrth=int(((ortho > 0) & (ortho < cosT)).sum()), nErrorNonOrth=int((ortho <= 0).sum()),
        maxNonOrthFace=int(np.argmax(theta)) if Fi else -1,
        maxSkewness=float(skew.max()), nSkewFaces=int((skew > thr["skewThreshold"]).sum()), maxSkewFace=int(np.argmax(skew)),
        nWrongOrientedFaces=int(wrong.sum()),
        maxOpenness=float(openness.max()), nOpenCells=int((openness > thr["closedThreshold"]).sum()),
        maxAspectRatio=float(ar.max()), nHighAspectCells=int((ar > thr["aspectThreshold"]).sum()),
    )
    fields = dict(cellVolume=V, cellOpenness=openness, cellAspectRatio=ar, faceNonOrthogonality=faceNO, faceSkewness=skew,
                  cellAbsPyramids=absPyr, faceOrtho=np.concatenate([ortho, np.ones(F - Fi)]))
    return rep, fields


def reference_of(oracle_lib, mesh, variant="com", **thr):
    fc, fa, cc = oracle_geometry(oracle_lib, mesh, variant)
    off, val = cell_faces(mesh)
    return quality_reference(mesh, fc, fa, cc, off, val, **thr)


# ---- the three meshes with hand-derived answers (also used by tests/test_gpu_quality.py) -------------------------------
def uniform_block():
    from smoothmesh_amd.meshgen import hex_block
    return hex_block(6, 5, 4, lengths=(1.2, 1.0, 0.8))


def two_cells(s):
    """a unit cube [0,1]^3 (cell 0, owner of the face x = 1) and a parallelepiped whose x = 2 face is shifted by s in y"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(2, 1, 1, lengths=(2.0, 1.0, 1.0))
    m.points = m.points.copy()
    m.points[np.isclose(m.points[:, 0], 2.0), 1] += s
    return m


def shared_face(m):
    """the internal face x = 1 of two_cells"""
    assert m.nInternalFaces == 1
    return 0


def tangled_block():
    """uniform 4^3 block, the interior point (0.25, 0.25, 0.25) pushed past the opposite faces x, y, z = 0.5 of its cell [0.25, 0.5]^3
    (a push past the face x = 0.5 alone folds the cell without turning its volume negative)"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(4)
    m.points = m.points.copy()
    p = int(np.argmin(np.abs(m.points - 0.25).sum(axis=1)))
    assert np.array_equal(m.points[p], [0.25, 0.25, 0.25]) and m.find_internal_points()[p]
    m.points[p] = [0.6, 0.6, 0.6]
    return m


def test_uniform_block_known_answers(oracle_lib):
    m = uniform_block()
    hx, hy, hz = 1.2 / 6, 1.0 / 5, 0.8 / 4
    rep, f = reference_of(oracle_lib, m)
    assert np.allclose(f["cellVolume"], hx * hy * hz, rtol=1e-13, atol=0)
    assert abs(rep["totalVolume"] - 1.2 * 1.0 * 0.8) <= 1e-13
    assert rep["maxNonOrth"] == 0.0
    assert rep["maxSkewness"] <= 1e-12
    Mx, My, Mz = 2 * hy * hz, 2 * hx * hz, 2 * hx * hy
    V = hx * hy * hz
    ar = max(max(Mx, My, Mz) / min(Mx, My, Mz), (Mx + My + Mz) / 6 / V ** (2 / 3))
    assert np.allclose(f["cellAspectRatio"], ar, rtol=1e-13, atol=0)
    for k in ("nNonPositiveVolume", "nZeroAreaFaces", "nSevereNonOrth", "nErrorNonOrth", "nSkewFaces", "nWrongOrientedFaces",
              "nOpenCells", "nHighAspectCells"):
        assert rep[k] == 0, k


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_two_cells_shared_face_known_answers(oracle_lib, s):
    m = two_cells(s)
    rep, f = reference_of(oracle_lib, m)
    fs = shared_face(m)
    assert abs(f["faceNonOrthogonality"][fs] - math.degrees(math.atan(s / 2))) <= 1e-12
    assert abs(f["faceSkewness"][fs] - s / 2) <= 1e-12
    assert np.allclose(f["cellVolume"], 1.0, rtol=1e-13)
    assert rep["maxNonOrthFace"] == fs and rep["nWrongOrientedFaces"] == 0 and rep["nNonPositiveVolume"] == 0


def test_tangled_block_is_reported(oracle_lib):
    m = tangled_block()
    rep, f = reference_of(oracle_lib, m)
    assert rep["nNonPositiveVolume"] >= 1
    assert rep["nWrongOrientedFaces"] >= 1
    assert abs(rep["totalVolume"] - 1.0) <= 1e-12          # the signed sum still telescopes to the box


def test_report_fields_match_the_reference():
    """the Python report (MeshQuality, the ctypes mirror of smgpu_quality) carries exactly the quantities this reference defines"""
    import dataclasses
    from smoothmesh_amd import MeshQuality, _ffi
    names = [f.name for f in dataclasses.fields(MeshQuality)]
    assert names == [n for n, _ in _ffi.Quality._fields_]
    m = two_cells(0.5)
    rep, _ = quality_reference(m, *_two_cells_geometry(m), *cell_faces(m))
    assert sorted(names) == sorted(rep)
    assert "smgpu_mesh_quality" in _ffi.SYMBOLS and "smgpu_quality_field" in _ffi.SYMBOLS
    _ffi.lib()                                              # the library exports both


def _two_cells_geometry(m):
    """exact geometry of two_cells(s), written out by hand: face centres / areas of the planar faces, cell centres"""
    fc = np.zeros((m.nFaces, 3)); fa = np.zeros((m.nFaces, 3))
    fo = m.faceOffsets
    for f in range(m.nFaces):
        p = m.points[m.facePoints[fo[f]:fo[f + 1]]]
        fc[f] = p.mean(axis=0)                                  # parallelograms: centroid = vertex mean
        fa[f] = 0.5 * np.cross(p[2] - p[0], p[3] - p[1])
    cc = np.zeros((m.nCells, 3))
    for c in range(m.nCells):
        cc[c] = m.points[np.unique(np.concatenate([m.facePoints[fo[f]:fo[f + 1]] for f in range(m.nFaces)
                                                    if m.owner[f] == c or (f < m.nInternalFaces and m.neighbour[f] == c)]))].mean(axis=0)
    return fc, fa, cc
