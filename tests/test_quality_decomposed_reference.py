"""Mesh quality of a decomposed mesh (DESIGN.md "Mesh quality", 10.4) without a GPU: a numpy restatement of the coupled per-rank
record (processor faces take the internal-face definitions with the neighbour's cell centre and count on the lower rank's side),
combined by smoothmesh_amd.quality.combine_quality, equals the numpy reference of the undecomposed mesh
(tests/test_quality_reference.py).  Also the combine's tie and empty-rank rules."""
import math

import numpy as np
import pytest

from test_quality_reference import DEFAULTS, VSMALL, ROOTVSMALL, _dot, _mag, cell_faces, oracle_geometry, quality_reference

EXACT = ("nCells", "nFaces", "nInternalFaces", "nNonPositiveVolume", "minVolumeCell", "nZeroAreaFaces", "nSevereNonOrth",
         "nErrorNonOrth", "maxNonOrthFace", "nSkewFaces", "maxSkewFace", "nWrongOrientedFaces", "nOpenCells", "nHighAspectCells")


def coupling_of(mesh, rank):
    return rank, [(p.startFace, p.nFaces, p.neighbProcNo) for p in mesh.patches if p.type == "processor"]


def send_reference(mesh, cc, coupling):
    f = np.concatenate([np.arange(s, s + n) for s, n, _ in coupling[1]]) if coupling[1] else np.zeros(0, np.int64)
    return cc[mesh.owner[f].astype(np.int64)].reshape(-1, 3)


def coupled_part_reference(mesh, fc, fa, cc, cfOff, cfVal, recvCc, coupling, **thr):
    """smgpu_quality_part of one sub-domain, restated in numpy"""
    thr = {**DEFAULTS, **thr}
    rank, pats = coupling
    F, Fi = mesh.nFaces, mesh.nInternalFaces
    own = mesh.owner.astype(np.int64)
    inner = np.zeros(F, bool); inner[:Fi] = True
    counted = np.ones(F, bool)
    CN = np.zeros((F, 3))
    CN[:Fi] = cc[mesh.neighbour]
    k = 0
    for s, n, o in pats:
        inner[s:s + n] = True
        CN[s:s + n] = recvCc[k:k + n]
        counted[s:s + n] = rank < o
        k += n
    magSf = _mag(fa)
    CO = cc[own]
    Cpf = fc - CO
    d = CN - CO
    ortho = _dot(d, fa) / (_mag(d) * magSf + VSMALL)
    theta = np.where(inner, np.degrees(np.arccos(np.clip(ortho, -1.0, 1.0))), 0.0)
    nb = fa / (magSf + ROOTVSMALL)[:, None]
    d = np.where(inner[:, None], d, _dot(nb, Cpf)[:, None] * nb)
    sv = Cpf - (_dot(fa, Cpf) / (_dot(fa, d) + ROOTVSMALL))[:, None] * d
    magSv = _mag(sv)
    sHat = sv / (magSv + ROOTVSMALL)[:, None]
    fo = mesh.faceOffsets.astype(np.int64)
    rowOf = np.repeat(np.arange(F), np.diff(fo))
    proj = np.abs(_dot(np.repeat(sHat, np.diff(fo), axis=0), mesh.points[mesh.facePoints] - fc[rowOf]))
    skew = magSv / np.maximum(0.2 * _mag(d) + ROOTVSMALL, np.maximum.reduceat(proj, fo[:-1]))
    wrong = (_dot(fa, Cpf) <= 0.0) | (inner & (_dot(fa, CN - fc) <= 0.0))
    _, cf = quality_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr)       # (the cell pass does not change)
    V = cf["cellVolume"]
    ci = counted & inner
    cosT = math.cos(math.radians(thr["nonOrthThreshold"]))
    th, sk = np.where(ci, theta, -np.inf), np.where(counted, skew, -np.inf)
    part = dict(
        nCells=mesh.nCells, nFaces=int(counted.sum()), nInternalFaces=int(ci.sum()),
        minVolume=float(V.min()) if len(V) else 0.0, maxVolume=float(V.max()) if len(V) else 0.0, totalVolume=float(V.sum()),
        nNonPositiveVolume=int((V <= VSMALL).sum()), minVolumeCell=int(np.argmin(V)) if len(V) else -1,
        minFaceArea=float(magSf[counted].min()), maxFaceArea=float(magSf[counted].max()), nZeroAreaFaces=int((counted & (magSf <= VSMALL)).sum()),
        maxNonOrth=float(th.max()) if ci.any() else 0.0, sumNonOrth=float(theta[ci].sum()),
        nSevereNonOrth=int((ci & (ortho > 0) & (ortho < cosT)).sum()), nErrorNonOrth=int((ci & (ortho <= 0)).sum()),
        maxNonOrthFace=int(np.argmax(th)) if ci.any() else -1,
        maxSkewness=float(sk.max()), nSkewFaces=int((counted & (skew > thr["skewThreshold"])).sum()), maxSkewFace=int(np.argmax(sk)),
        nWrongOrientedFaces=int((counted & wrong).sum()),
        maxOpenness=float(cf["cellOpenness"].max()), nOpenCells=int((cf["cellOpenness"] > thr["closedThreshold"]).sum()),
        maxAspectRatio=float(cf["cellAspectRatio"].max()), nHighAspectCells=int((cf["cellAspectRatio"] > thr["aspectThreshold"]).sum()))
    return part, dict(faceNonOrthogonality=theta, faceSkewness=skew)


def decomposed_reference(oracle_lib, subs, variant):
    """combine_quality of the numpy records of every sub-domain"""
    from smoothmesh_amd.quality import combine_quality, paired_offsets
    geo = [oracle_geometry(oracle_lib, s.mesh, variant) for s in subs]
    couplings = [coupling_of(s.mesh, s.rank) for s in subs]
    send = [send_reference(s.mesh, g[2], c) for s, g, c in zip(subs, geo, couplings)]
    recv = [np.zeros_like(x) for x in send]
    for i, off, j, ooff, n in paired_offsets(couplings):
        recv[i][off:off + n] = send[j][ooff:ooff + n]
    parts = [coupled_part_reference(s.mesh, *g, *cell_faces(s.mesh), r, c)[0] for s, g, r, c in zip(subs, geo, recv, couplings)]
    return combine_quality(parts, [s.cellProcAddressing for s in subs], [s.faceProcAddressing for s in subs])


def assert_combined(q, rep, scale_v, tol=1e-12):
    import dataclasses
    got = dataclasses.asdict(q)
    for k in EXACT:
        assert got[k] == rep[k], (k, got[k], rep[k])
    for k in ("minVolume", "maxVolume", "totalVolume"):
        assert abs(got[k] - rep[k]) <= tol * scale_v, (k, got[k], rep[k])
    for k in ("minFaceArea", "maxFaceArea", "maxNonOrth", "avgNonOrth", "maxSkewness", "maxOpenness", "maxAspectRatio"):
        assert abs(got[k] - rep[k]) <= tol * max(abs(rep[k]), 1e-300) or (k == "maxOpenness" and abs(got[k] - rep[k]) <= 1e-14), \
            (k, got[k], rep[k])


def partitions(mesh, kind):
    from smoothmesh_amd.decompose import bfs_partition, grid_partition, random_partition
    if kind == "grid":
        return grid_partition(mesh, (2, 2, 1)), 4
    if kind == "bfs":
        return bfs_partition(mesh, 5, seed=3), 5
    return random_partition(mesh, 4, seed=4), 4


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random"])
def test_decomposed_reference_equals_serial(oracle_lib, variant, kind):
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality import _assert_well_posed
    m = hex_block(9, 8, 7, jitter=0.3, seed=21)
    fc, fa, cc = oracle_geometry(oracle_lib, m, variant)
    rep, f = quality_reference(m, fc, fa, cc, *cell_faces(m))
    _assert_well_posed(rep, f)
    cellRank, n = partitions(m, kind)
    q = decomposed_reference(oracle_lib, decompose(m, cellRank, n), variant)
    assert_combined(q, rep, float(f["cellAbsPyramids"].sum()))


def _part(**kw):
    base = dict(nCells=1, nFaces=1, nInternalFaces=1, minVolume=1.0, maxVolume=1.0, totalVolume=1.0, nNonPositiveVolume=0, minVolumeCell=0,
                minFaceArea=1.0, maxFaceArea=1.0, nZeroAreaFaces=0, maxNonOrth=10.0, sumNonOrth=10.0, nSevereNonOrth=0, nErrorNonOrth=0,
                maxNonOrthFace=0, maxSkewness=0.5, nSkewFaces=0, maxSkewFace=0, nWrongOrientedFaces=0, maxOpenness=0.0, nOpenCells=0,
                maxAspectRatio=1.0, nHighAspectCells=0)
    base.update(kw)
    return base


def test_combine_ties_go_to_the_lowest_global_id():
    from smoothmesh_amd.quality import combine_quality
    a = _part(minVolumeCell=0, maxNonOrthFace=2, maxSkewFace=1)
    b = _part(minVolumeCell=1, maxNonOrthFace=0, maxSkewFace=3)
    cells = [np.array([7, 9]), np.array([4, 3])]             # rank 1's cell 1 is global 3 < rank 0's cell 0 (global 7)
    faces = [np.array([0, 1, 20, 5]), np.array([11, 12, 13, 2])]
    q = combine_quality([a, b], cells, faces)
    assert (q.minVolumeCell, q.minVolumeRank, q.minVolumeLocal) == (3, 1, 1)
    assert (q.maxNonOrthFace, q.maxNonOrthRank, q.maxNonOrthLocal) == (11, 1, 0)
    assert (q.maxSkewFace, q.maxSkewRank, q.maxSkewLocal) == (1, 0, 1)
    # without addressing: ids -1, the lowest (rank, local id) wins
    q = combine_quality([a, b])
    assert (q.minVolumeCell, q.minVolumeRank, q.minVolumeLocal) == (-1, 0, 0)
    assert (q.maxNonOrthFace, q.maxNonOrthRank, q.maxNonOrthLocal) == (-1, 0, 2)
    # a strictly larger value wins whatever its id
    q = combine_quality([a, _part(maxNonOrth=10.5, maxNonOrthFace=3)], cells, [faces[0], np.array([11, 12, 13, 50])])
    assert (q.maxNonOrthFace, q.maxNonOrth) == (50, 10.5)


def test_combine_sums_in_rank_order_and_skips_empty_ranks():
    from smoothmesh_amd.quality import combine_quality
    empty = _part(nCells=0, nFaces=0, nInternalFaces=0, minVolume=0.0, maxVolume=0.0, totalVolume=0.0, minVolumeCell=-1, minFaceArea=0.0,
                  maxFaceArea=0.0, maxNonOrth=0.0, sumNonOrth=0.0, maxNonOrthFace=-1, maxSkewness=0.0, maxSkewFace=-1, maxOpenness=0.0,
                  maxAspectRatio=0.0)
    a = _part(nCells=3, nFaces=10, nInternalFaces=4, totalVolume=0.1, sumNonOrth=0.1, minVolume=2.0, maxVolume=3.0, minFaceArea=0.5, nSkewFaces=2)
    b = _part(nCells=2, nFaces=6, nInternalFaces=2, totalVolume=0.2, sumNonOrth=0.2, minVolume=1.5, maxVolume=2.5, minFaceArea=0.7, nSkewFaces=1)
    q = combine_quality([empty, a, b, empty])
    assert (q.nCells, q.nFaces, q.nInternalFaces, q.nSkewFaces) == (5, 16, 6, 3)
    assert q.totalVolume == 0.1 + 0.2 and q.avgNonOrth == (0.1 + 0.2) / 6
    assert (q.minVolume, q.maxVolume, q.minFaceArea) == (1.5, 3.0, 0.5)
    assert q.minVolumeRank == 2
    z = combine_quality([empty, empty])
    assert (z.nCells, z.minVolumeCell, z.maxNonOrthFace, z.maxSkewFace, z.avgNonOrth, z.minFaceArea) == (0, -1, -1, -1, 0.0, 0.0)
    assert z.minVolumeRank == -1


def test_paired_offsets_refuses_unpaired_patches():
    from smoothmesh_amd.quality import paired_offsets
    assert sorted(paired_offsets([(0, [(10, 3, 1)]), (1, [(5, 3, 0)])])) == [(0, 0, 1, 0, 3), (1, 0, 0, 0, 3)]
    with pytest.raises(ValueError):
        paired_offsets([(0, [(10, 3, 1)]), (1, [])])
    with pytest.raises(ValueError):
        paired_offsets([(0, [(10, 3, 1)]), (1, [(5, 2, 0)])])


def test_coupled_symbols_are_exported():
    from smoothmesh_amd import _ffi
    for s in ("smgpu_quality_coupled_pack", "smgpu_quality_coupled_report", "smgpu_quality_coupled_field"):
        assert s in _ffi.SYMBOLS
    _ffi.lib()
    names = [n for n, _ in _ffi.QualityPart._fields_]
    assert names == [("sumNonOrth" if n == "avgNonOrth" else n) for n, _ in _ffi.Quality._fields_]
