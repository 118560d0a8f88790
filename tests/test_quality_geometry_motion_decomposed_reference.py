"""The -allGeometry checks and the motion criteria of a decomposed mesh (DESIGN.md "Mesh quality", 10.8) without a GPU: a numpy
restatement of the per-rank part records (smgpu_quality_geometry_part / smgpu_quality_motion_part) from the oracle's geometry of
each sub-domain -- processor faces take the internal-face branch with the neighbour rank's cell centre and volume, a cell's
determinant runs over its internal and processor faces, a processor face counts on the lower rank's side -- combined by
smoothmesh_amd.quality.combine_quality_geometry / _motion, equals the serial numpy references of the undecomposed mesh
(tests/test_quality_geometry_reference.py, tests/test_quality_motion_reference.py).  Also the combines' tie, empty-rank and
empty-case rules, and the exported symbols.  tests/test_gpu_quality_geometry_motion_decomposed.py holds the engine to it."""
import dataclasses
import math

import numpy as np
import pytest

from test_quality_decomposed_reference import coupling_of, partitions, send_reference
from test_quality_geometry_reference import GEOMETRY_DEFAULTS, quality_geometry_reference
from test_quality_motion_reference import MOTION_DEFAULTS, _cross, base_minima, _side_min, quality_motion_reference
from test_quality_reference import ROOTVSMALL, VSMALL, _dot, _mag, cell_faces, oracle_geometry, quality_reference

# The formulas new to a decomposed comparison cube a circumradius (tet quality), take a 3 x 3 determinant, or divide two volumes.
# MEASURED_DIFF: the largest decomposed-versus-serial difference of the numpy references below, over the meshes of this file and
# of the GPU test (_case("grid" | "bfs" | "random" | "cavity"), both foam variants), per-element fields and report values, relative
# to max(|serial|, 1): 6.3e-14, on the cavity mesh (measured on the CPU; this file's block alone gives 1.2e-14, printed by
# test_decomposed_reference_equals_serial).  ALLOWED_DIFF: 8 x that,
# since the device sums a sub-domain's cell faces in another order than numpy.  test_decomposed_reference_equals_serial asserts
# that the reference itself stays inside ALLOWED_DIFF.
MEASURED_DIFF = 6.3e-14
ALLOWED_DIFF = 8 * MEASURED_DIFF
NEW_FORMULA_VALUES = ("minVolRatio", "avgVolRatio", "minDeterminant", "avgDeterminant", "minTetQuality", "avgTetQuality", "minBaseTetQuality")
NEW_FORMULA_FIELDS = ("faceVolumeRatio", "cellDeterminant", "faceTetQuality", "faceBaseTetQuality")

GEOMETRY_EXACT = ("nConcaveFaces", "nFlatnessFaces", "nWarpedFaces", "nLowWeightFaces", "nLowVolRatioFaces", "nUnderdeterminedCells",
                  "maxConcaveFace", "minFlatnessFace", "minFaceWeightFace", "minVolRatioFace", "minDeterminantCell")
MOTION_EXACT = ("nLowTetFaces", "nNoBasePointFaces", "nTwistFaces", "nLowTwistFaces", "nLowTriangleTwistFaces", "minTetFace",
                "minBaseTetFace", "minTwistFace", "minTriangleTwistFace")


def coupled_rows(mesh, cc, V, recvCc, recvVc, coupling):
    """(inner, counted, CN, VN) by face: the widened internal-face rule, the counted-once rule, the neighbour's centre and volume"""
    rank, pats = coupling
    F, Fi = mesh.nFaces, mesh.nInternalFaces
    inner = np.arange(F) < Fi
    counted = np.ones(F, bool)
    CN, VN = np.zeros((F, 3)), np.zeros(F)
    nei = mesh.neighbour.astype(np.int64)[:Fi]
    CN[:Fi], VN[:Fi] = cc[nei], V[nei]
    k = 0
    for s, n, o in pats:
        inner[s:s + n] = True
        CN[s:s + n], VN[s:s + n] = recvCc[k:k + n], recvVc[k:k + n]
        counted[s:s + n] = rank < o
        k += n
    return inner, counted, CN, VN


def _argmin_in(v, mask):
    return int(np.argmin(np.where(mask, v, np.inf))) if mask.any() else -1


def geometry_part_reference(mesh, fc, fa, cc, cfOff, cfVal, recvCc, recvVc, coupling, **thr):
    """(smgpu_quality_geometry_part of one sub-domain, its five fields), restated in numpy"""
    thr = {**GEOMETRY_DEFAULTS, **thr}
    serial = quality_geometry_reference(mesh, fc, fa, cc, cfOff, cfVal, **thr)[1]      # concavity and flatness read the face alone
    conc, flat, summed = serial["faceConcavity"], serial["faceFlatness"], serial["_summed"]
    V = quality_reference(mesh, fc, fa, cc, cfOff, cfVal)[1]["cellVolume"]
    inner, counted, CN, VN = coupled_rows(mesh, cc, V, recvCc, recvVc, coupling)
    own = mesh.owner.astype(np.int64)
    dO, dN = np.abs(_dot(fa, fc - cc[own])), np.abs(_dot(fa, CN - fc))
    w = np.where(inner, np.minimum(dO, dN) / ((dO + dN) + VSMALL), 1.0)
    vO = V[own]
    r = np.where(inner, np.minimum(vO, VN) / (np.maximum(vO, VN) + VSMALL), 1.0)
    # the determinant over the internal and the processor faces of every cell (the sums of quality_geometry_reference)
    C = mesh.nCells
    cfOff = cfOff.astype(np.int64)
    cellOf = np.repeat(np.arange(C), np.diff(cfOff))
    fid = (cfVal & 0x7fffffff).astype(np.int64)
    magSf = _mag(fa)
    inn = inner[fid]
    nInt = np.add.reduceat(inn.astype(np.int64), cfOff[:-1])
    avgA = np.add.reduceat(np.where(inn, magSf[fid], 0.0), cfOff[:-1]) / np.maximum(nInt, 1)
    ok = (nInt > 0) & (avgA >= ROOTVSMALL)
    sn = np.where(inn[:, None], fa[fid], 0.0) / np.where(ok, avgA, 1.0)[cellOf][:, None]
    T = {k: np.add.reduceat(sn[:, i] * sn[:, j], cfOff[:-1]) for k, (i, j) in
         dict(xx=(0, 0), xy=(0, 1), xz=(0, 2), yy=(1, 1), yz=(1, 2), zz=(2, 2)).items()}
    det = np.abs((T["xx"] * (T["yy"] * T["zz"] - T["yz"] * T["yz"]) - T["xy"] * (T["xy"] * T["zz"] - T["yz"] * T["xz"]))
                 + T["xz"] * (T["xy"] * T["yz"] - T["yy"] * T["xz"])) / 8.0
    det = np.where(ok, det, 0.0)

    isConc, fl, ci = counted & (conc > 1e-15), counted & summed, counted & inner
    maxSin = float(conc[isConc].max()) if isConc.any() else 0.0
    part = dict(
        nCells=C, nFaces=int(counted.sum()), nInternalFaces=int(ci.sum()),
        nConcaveFaces=int(isConc.sum()), maxConcaveSin=maxSin, maxConcaveAngle=math.degrees(math.asin(min(1.0, maxSin))),
        maxConcaveFace=int(np.argmax(np.where(isConc, conc, -1.0))) if isConc.any() else -1,
        minFlatness=float(flat[fl].min()) if fl.any() else 1.0, sumFlatness=float(flat[fl].sum()), nFlatnessFaces=int(fl.sum()),
        nWarpedFaces=int((fl & (flat < thr["flatnessThreshold"])).sum()), minFlatnessFace=_argmin_in(flat, fl),
        minFaceWeight=float(w[ci].min()) if ci.any() else 1.0, sumFaceWeight=float(w[ci].sum()),
        nLowWeightFaces=int((ci & (w < thr["weightThreshold"])).sum()), minFaceWeightFace=_argmin_in(w, ci),
        minVolRatio=float(r[ci].min()) if ci.any() else 1.0, sumVolRatio=float(r[ci].sum()),
        nLowVolRatioFaces=int((ci & (r < thr["volRatioThreshold"])).sum()), minVolRatioFace=_argmin_in(r, ci),
        minDeterminant=float(det.min()) if C else 0.0, sumDeterminant=float(det.sum()),
        nUnderdeterminedCells=int((det < thr["determinantThreshold"]).sum()), minDeterminantCell=int(np.argmin(det)) if C else -1)
    return part, dict(faceConcavity=conc, faceFlatness=flat, faceWeight=w, faceVolumeRatio=r, cellDeterminant=det)


def motion_fields(mesh, fc, cc, internal, CN):
    """the four fields of quality_motion_reference with `internal` and C_N by face given (its statements, in its order) -> also "_summed" """
    F = mesh.nFaces
    CO = cc[mesh.owner.astype(np.int64)]
    fo = mesh.faceOffsets.astype(np.int64)
    nv = np.diff(fo)
    rowOf = np.repeat(np.arange(F), nv)
    first = fo[:-1][rowOf]
    local = np.arange(fo[-1]) - first
    P = mesh.points[mesh.facePoints]
    Pn = P[first + (local + 1) % nv[rowOf]]
    tet = np.minimum.reduceat(_side_min(P, Pn, fc[rowOf], CO[rowOf], CN[rowOf], internal[rowOf]), fo[:-1])
    base = np.empty(F)
    for n in np.unique(nv):
        idx = np.nonzero(nv == n)[0]
        m = base_minima(P[fo[idx][:, None] + np.arange(n)[None, :]], CO[idx], CN[idx], internal[idx])
        best = m[:, 0].copy()
        for b in range(1, n):
            best = np.where(m[:, b] > best, m[:, b], best)
        base[idx] = best
    summed = nv > 3
    d = np.where(internal[:, None], CN, fc) - CO
    nHat = d / (_mag(d) + VSMALL)[:, None]
    t = 0.5 * _cross(Pn - P, fc[rowOf] - P)
    mt = _mag(t)
    valid = (mt > VSMALL) & summed[rowOf]
    h = t / np.where(valid, mt, 1.0)[:, None]
    tw = np.minimum.reduceat(np.where(valid, _dot(nHat[rowOf], h), np.inf), fo[:-1])
    nValid = np.add.reduceat(valid.astype(np.int64), fo[:-1])
    tw = np.where(nValid > 0, tw, 1.0)
    allValid = nValid == nv
    hp = h[first + (local - 1) % nv[rowOf]]
    tri = np.minimum.reduceat(np.where(allValid[rowOf], _dot(hp, h), np.inf), fo[:-1])
    for f in np.nonzero(~allValid)[0]:
        hv = h[fo[f]:fo[f + 1]][valid[fo[f]:fo[f + 1]]]
        tri[f] = min(float(_dot(hv[i - 1:i] if i else hv[-1:], hv[i:i + 1])[0]) for i in range(len(hv))) if len(hv) >= 2 else 1.0
    tri = np.where(nValid >= 2, tri, 1.0)
    return dict(faceTetQuality=tet, faceBaseTetQuality=base, faceTwist=tw, faceTriangleTwist=tri, _summed=summed)


def motion_part_reference(mesh, fc, fa, cc, cfOff, cfVal, recvCc, coupling, **thr):
    """(smgpu_quality_motion_part of one sub-domain, its four fields), restated in numpy"""
    thr = {**MOTION_DEFAULTS, **thr}
    inner, counted, CN, _ = coupled_rows(mesh, cc, np.zeros(mesh.nCells), recvCc, np.zeros(len(recvCc)), coupling)
    f = motion_fields(mesh, fc, cc, inner, CN)
    tet, base, tw, tri = f["faceTetQuality"], f["faceBaseTetQuality"], f["faceTwist"], f["faceTriangleTwist"]
    cs = counted & f["_summed"]
    part = dict(
        nFaces=int(counted.sum()),
        minTetQuality=float(tet[counted].min()) if counted.any() else 1.0, sumTetQuality=float(tet[counted].sum()),
        nLowTetFaces=int((counted & (tet < thr["tetThreshold"])).sum()), minTetFace=_argmin_in(tet, counted),
        minBaseTetQuality=float(base[counted].min()) if counted.any() else 1.0,
        nNoBasePointFaces=int((counted & (base < thr["tetThreshold"])).sum()), minBaseTetFace=_argmin_in(base, counted),
        minTwist=float(tw[cs].min()) if cs.any() else 1.0, sumTwist=float(tw[cs].sum()), nTwistFaces=int(cs.sum()),
        nLowTwistFaces=int((cs & (tw < thr["twistThreshold"])).sum()), minTwistFace=_argmin_in(tw, cs),
        minTriangleTwist=float(tri[cs].min()) if cs.any() else 1.0, sumTriangleTwist=float(tri[cs].sum()),
        nLowTriangleTwistFaces=int((cs & (tri < thr["triangleTwistThreshold"])).sum()), minTriangleTwistFace=_argmin_in(tri, cs))
    return part, {k: v for k, v in f.items() if not k.startswith("_")}


def decomposed_references(oracle_lib, subs, variant, geometry_thr=None, motion_thr=None):
    """(combined geometry report, combined motion report, per-rank geometry parts, motion parts, geometry fields, motion fields) of
    the numpy records of every sub-domain: the volume slices move by the same paired_offsets as the centres"""
    from smoothmesh_amd.quality import combine_quality_geometry, combine_quality_motion, paired_offsets
    geo = [oracle_geometry(oracle_lib, s.mesh, variant) for s in subs]
    cfs = [cell_faces(s.mesh) for s in subs]
    couplings = [coupling_of(s.mesh, s.rank) for s in subs]
    vols = [quality_reference(s.mesh, *g, *cf)[1]["cellVolume"] for s, g, cf in zip(subs, geo, cfs)]
    send = [send_reference(s.mesh, g[2], c) for s, g, c in zip(subs, geo, couplings)]
    sendV = [send_reference(s.mesh, np.repeat(v[:, None], 3, axis=1), c)[:, 0] for s, v, c in zip(subs, vols, couplings)]
    recv, recvV = [np.zeros_like(x) for x in send], [np.zeros_like(x) for x in sendV]
    for i, off, j, ooff, n in paired_offsets(couplings):
        recv[i][off:off + n] = send[j][ooff:ooff + n]
        recvV[i][off:off + n] = sendV[j][ooff:ooff + n]
    g = [geometry_part_reference(s.mesh, *x, *cf, r, rv, c, **(geometry_thr or {})) for s, x, cf, r, rv, c in zip(subs, geo, cfs, recv, recvV, couplings)]
    t = [motion_part_reference(s.mesh, *x, *cf, r, c, **(motion_thr or {})) for s, x, cf, r, c in zip(subs, geo, cfs, recv, couplings)]
    ids = [s.cellProcAddressing for s in subs], [s.faceProcAddressing for s in subs]
    return (combine_quality_geometry([p[0] for p in g], *ids), combine_quality_motion([p[0] for p in t], *ids),
            [p[0] for p in g], [p[0] for p in t], [p[1] for p in g], [p[1] for p in t])


def reference_difference(q, rep, exact, fields, serialFields, subs):
    """the largest decomposed-versus-serial difference relative to max(|serial|, 1): (of the report's values, of the fields), after
    asserting the counts and ids equal"""
    got = dataclasses.asdict(q)
    for k in exact:
        assert got[k] == rep[k], (k, got[k], rep[k])
    dv = max(abs(got[k] - v) / max(abs(v), 1.0) for k, v in rep.items() if k not in exact)
    df = 0.0
    for s, f in zip(subs, fields):
        for name, v in f.items():
            a = s.cellProcAddressing if name.startswith("cell") else s.faceProcAddressing
            ref = serialFields[name][a]
            df = max(df, float(np.max(np.abs(v - ref) / np.maximum(np.abs(ref), 1.0))))
    return dv, df


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("kind", ["grid", "bfs", "random"])
def test_decomposed_reference_equals_serial(oracle_lib, variant, kind):
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(12, 10, 8, jitter=0.3, seed=31)
    fc, fa, cc = oracle_geometry(oracle_lib, m, variant)
    cf = cell_faces(m)
    grep, gf = quality_geometry_reference(m, fc, fa, cc, *cf)
    mrep, mf = quality_motion_reference(m, fc, fa, cc, *cf)
    cellRank, n = partitions(m, kind)
    subs = decompose(m, cellRank, n)
    qg, qm, _, _, fg, fm = decomposed_references(oracle_lib, subs, variant)
    d = reference_difference(qg, grep, GEOMETRY_EXACT, fg, gf, subs) + reference_difference(qm, mrep, MOTION_EXACT, fm, mf, subs)
    print(f"    decomposed-versus-serial difference of the references: {max(d):.3e}")
    assert max(d) <= ALLOWED_DIFF, d


def test_motion_restatement_is_the_serial_reference(oracle_lib):
    """with internal = f < nInternalFaces and the local neighbour centres, motion_fields is quality_motion_reference bit for bit"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(5, 4, 3, jitter=0.3, seed=2)
    fc, fa, cc = oracle_geometry(oracle_lib, m)
    cf = cell_faces(m)
    part, f = motion_part_reference(m, fc, fa, cc, *cf, np.zeros((0, 3)), (0, []))
    rep, ref = quality_motion_reference(m, fc, fa, cc, *cf)
    for k, v in f.items():
        assert v.tobytes() == ref[k].tobytes(), k
    part2, f2 = geometry_part_reference(m, fc, fa, cc, *cf, np.zeros((0, 3)), np.zeros(0), (0, []))
    rep2, ref2 = quality_geometry_reference(m, fc, fa, cc, *cf)
    for k, v in f2.items():
        assert v.tobytes() == ref2[k].tobytes(), k
    from smoothmesh_amd.quality import combine_quality_geometry, combine_quality_motion
    ids = [np.arange(m.nCells)], [np.arange(m.nFaces)]
    got = dataclasses.asdict(combine_quality_motion([part], *ids))
    assert all(got[k] == v for k, v in rep.items()), (got, rep)
    got = dataclasses.asdict(combine_quality_geometry([part2], *ids))
    assert all(got[k] == v for k, v in rep2.items() if k != "maxConcaveAngle"), (got, rep2)


def test_processor_boundary_cell_keeps_its_determinant(oracle_lib):
    """a cell on a processor boundary of the uniform block: det = 1 with the widened rule; the serial-only rule sees a missing face"""
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(6, 6, 6)
    subs = decompose(m, grid_partition(m, (2, 1, 1)), 2)
    _, _, _, _, fg, _ = decomposed_references(oracle_lib, subs, "com")
    serial = quality_geometry_reference(m, *oracle_geometry(oracle_lib, m), *cell_faces(m))[1]["cellDeterminant"]
    inner = np.nonzero(np.abs(serial - 1.0) <= 1e-13)[0]
    assert len(inner) == 64
    seen = 0
    for s, f in zip(subs, fg):
        sm = s.mesh
        local = quality_geometry_reference(sm, *oracle_geometry(oracle_lib, sm), *cell_faces(sm))[1]["cellDeterminant"]
        onProc = np.zeros(sm.nCells, bool)
        for p in sm.patches:
            if p.type == "processor":
                onProc[sm.owner[p.startFace:p.startFace + p.nFaces]] = True
        pick = onProc & np.isin(s.cellProcAddressing, inner)
        seen += int(pick.sum())
        assert np.max(np.abs(f["cellDeterminant"][pick] - 1.0)) <= 1e-13
        assert np.max(local[pick]) <= 0.5 + 1e-13              # the sub-domain's own internal faces alone: five faces, det 0.5
        assert np.max(np.abs(f["cellDeterminant"] - serial[s.cellProcAddressing])) <= 1e-13
    assert seen == 32


# ---- the combines ------------------------------------------------------------------------------------------------------
def _gpart(**kw):
    base = dict(nCells=1, nFaces=2, nInternalFaces=1, nConcaveFaces=1, maxConcaveSin=0.5, maxConcaveAngle=30.0, maxConcaveFace=0,
                minFlatness=0.9, sumFlatness=0.9, nFlatnessFaces=1, nWarpedFaces=0, minFlatnessFace=0, minFaceWeight=0.4, sumFaceWeight=0.4,
                nLowWeightFaces=0, minFaceWeightFace=0, minVolRatio=0.7, sumVolRatio=0.7, nLowVolRatioFaces=0, minVolRatioFace=0,
                minDeterminant=0.25, sumDeterminant=0.25, nUnderdeterminedCells=0, minDeterminantCell=0)
    base.update(kw)
    return base


def _mpart(**kw):
    base = dict(nFaces=2, minTetQuality=0.3, sumTetQuality=0.7, nLowTetFaces=0, minTetFace=0, minBaseTetQuality=0.2, nNoBasePointFaces=0,
                minBaseTetFace=0, minTwist=0.9, sumTwist=0.9, nTwistFaces=1, nLowTwistFaces=0, minTwistFace=0, minTriangleTwist=0.8,
                sumTriangleTwist=0.8, nLowTriangleTwistFaces=0, minTriangleTwistFace=0)
    base.update(kw)
    return base


GEOMETRY_EMPTY = dict(nCells=0, nFaces=0, nInternalFaces=0, nConcaveFaces=0, maxConcaveSin=0.0, maxConcaveAngle=0.0, maxConcaveFace=-1,
                      minFlatness=1.0, sumFlatness=0.0, nFlatnessFaces=0, minFlatnessFace=-1, minFaceWeight=1.0, sumFaceWeight=0.0,
                      minFaceWeightFace=-1, minVolRatio=1.0, sumVolRatio=0.0, minVolRatioFace=-1, minDeterminant=0.0, sumDeterminant=0.0,
                      minDeterminantCell=-1)
MOTION_EMPTY = dict(nFaces=0, minTetQuality=1.0, sumTetQuality=0.0, minTetFace=-1, minBaseTetQuality=1.0, minBaseTetFace=-1, minTwist=1.0,
                    sumTwist=0.0, nTwistFaces=0, minTwistFace=-1, minTriangleTwist=1.0, sumTriangleTwist=0.0, minTriangleTwistFace=-1)


def test_combine_ties_go_to_the_lowest_global_id():
    from smoothmesh_amd.quality import combine_quality_geometry, combine_quality_motion
    cells = [np.array([7, 9]), np.array([4, 3])]
    faces = [np.array([0, 1, 20, 5]), np.array([11, 12, 13, 2])]
    a = _gpart(maxConcaveFace=2, minFlatnessFace=1, minFaceWeightFace=2, minVolRatioFace=0, minDeterminantCell=0)
    b = _gpart(maxConcaveFace=0, minFlatnessFace=3, minFaceWeightFace=3, minVolRatioFace=1, minDeterminantCell=1, maxConcaveAngle=31.0)
    q = combine_quality_geometry([a, b], cells, faces)
    assert (q.maxConcaveFace, q.maxConcaveRank, q.maxConcaveLocal, q.maxConcaveAngle) == (11, 1, 0, 31.0)     # the winner's pair
    assert (q.minFlatnessFace, q.minFlatnessRank, q.minFlatnessLocal) == (1, 0, 1)
    assert (q.minFaceWeightFace, q.minFaceWeightRank) == (2, 1)
    assert (q.minVolRatioFace, q.minVolRatioRank) == (0, 0)
    assert (q.minDeterminantCell, q.minDeterminantRank, q.minDeterminantLocal) == (3, 1, 1)
    q = combine_quality_geometry([a, b])                     # without addressing: ids -1, the lowest (rank, local id) wins
    assert (q.maxConcaveFace, q.maxConcaveRank, q.maxConcaveLocal, q.maxConcaveAngle) == (-1, 0, 2, 30.0)
    assert (q.minDeterminantCell, q.minDeterminantRank, q.minDeterminantLocal) == (-1, 0, 0)
    q = combine_quality_geometry([a, _gpart(minVolRatio=0.65, minVolRatioFace=2)], cells, faces)      # a strictly smaller value wins
    assert (q.minVolRatioFace, q.minVolRatio) == (13, 0.65)
    ma, mb = _mpart(minTetFace=2, minBaseTetFace=1, minTwistFace=0, minTriangleTwistFace=2), _mpart(minTetFace=0, minBaseTetFace=3,
                                                                                                      minTwistFace=1, minTriangleTwistFace=3)
    t = combine_quality_motion([ma, mb], cells, faces)
    assert (t.minTetFace, t.minTetRank, t.minTetLocal) == (11, 1, 0)
    assert (t.minBaseTetFace, t.minBaseTetRank, t.minBaseTetLocal) == (1, 0, 1)
    assert (t.minTwistFace, t.minTwistRank) == (0, 0) and (t.minTriangleTwistFace, t.minTriangleTwistRank) == (2, 1)
    t = combine_quality_motion([ma, mb])
    assert (t.minTetFace, t.minTetRank, t.minTetLocal) == (-1, 0, 2)


def test_combine_sums_in_rank_order_and_skips_empty_ranks():
    from smoothmesh_amd.quality import combine_quality_geometry, combine_quality_motion
    e = _gpart(**GEOMETRY_EMPTY)
    a = _gpart(nCells=3, nInternalFaces=4, nFlatnessFaces=5, sumFlatness=0.1, sumFaceWeight=0.1, sumVolRatio=0.1, sumDeterminant=0.1,
               nWarpedFaces=2, minFlatness=0.95)
    b = _gpart(nCells=2, nInternalFaces=2, nFlatnessFaces=2, sumFlatness=0.2, sumFaceWeight=0.2, sumVolRatio=0.2, sumDeterminant=0.2,
               nWarpedFaces=1, minFlatness=0.85, minFaceWeight=0.3)
    c = _gpart(nCells=1, nInternalFaces=1, nFlatnessFaces=1, sumFlatness=0.3, sumFaceWeight=0.3, sumVolRatio=0.3, sumDeterminant=0.3)
    q = combine_quality_geometry([e, a, b, e, c])
    assert (q.nFlatnessFaces, q.nWarpedFaces, q.nConcaveFaces) == (8, 3, 3)
    s = (0.0 + 0.1 + 0.2) + 0.0 + 0.3                                  # left to right in rank order
    assert s != 0.1 + (0.2 + 0.3)
    assert q.avgFlatness == s / 8 and q.avgFaceWeight == s / 7 and q.avgVolRatio == s / 7 and q.avgDeterminant == s / 6
    assert (q.minFlatness, q.minFlatnessRank) == (0.85, 2) and (q.minFaceWeight, q.minFaceWeightRank) == (0.3, 2)
    # a rank without internal faces or concave faces does not take part, whatever its neutral values are
    q = combine_quality_geometry([_gpart(nInternalFaces=0, minFaceWeight=0.0, minVolRatio=0.0, nConcaveFaces=0, maxConcaveSin=9.0), a])
    assert (q.minFaceWeight, q.minFaceWeightRank, q.minVolRatioRank, q.maxConcaveSin, q.maxConcaveRank) == (0.4, 1, 1, 0.5, 1)
    me = _mpart(**MOTION_EMPTY)
    ta, tb = _mpart(nFaces=3, sumTetQuality=0.1, sumTwist=0.1, sumTriangleTwist=0.1, nTwistFaces=2), \
        _mpart(nFaces=2, sumTetQuality=0.2, sumTwist=0.2, sumTriangleTwist=0.2, nTwistFaces=1, minTwist=0.5, nLowTwistFaces=1)
    tc = _mpart(nFaces=4, sumTetQuality=0.3, sumTwist=0.3, sumTriangleTwist=0.3, nTwistFaces=0, minTwist=-5.0, minTwistFace=-1)
    t = combine_quality_motion([me, ta, tb, tc])
    assert t.avgTetQuality == s / 9 and t.avgTwist == s / 3 and t.avgTriangleTwist == s / 3
    assert (t.nTwistFaces, t.nLowTwistFaces, t.minTwist, t.minTwistRank) == (3, 1, 0.5, 2)       # tc has no face with more than 3 vertices


def test_combine_empty_case_values():
    """every empty-case value of the serial reports: 1, the concavity figures 0, the determinant's 0; ids and ranks -1"""
    from smoothmesh_amd.quality import combine_quality_geometry, combine_quality_motion
    for parts in ([], [_gpart(**GEOMETRY_EMPTY)] * 2):
        q = dataclasses.asdict(combine_quality_geometry(parts))
        for k, v in q.items():
            want = (-1 if k.endswith(("Face", "Cell", "Rank", "Local")) else 0 if k.startswith("n")
                    else 0.0 if k.startswith("maxConcave") or "Determinant" in k else 1.0)
            assert v == want and type(v) is type(want), (k, v)
    for parts in ([], [_mpart(**MOTION_EMPTY)] * 2):
        t = dataclasses.asdict(combine_quality_motion(parts))
        for k, v in t.items():
            want = -1 if k.endswith(("Face", "Rank", "Local")) else 0 if k.startswith("n") else 1.0
            assert v == want and type(v) is type(want), (k, v)
    # faces but none with more than 3 vertices, cells but no internal face: the serial values of those cases
    q = combine_quality_geometry([_gpart(nInternalFaces=0, nFlatnessFaces=0, nConcaveFaces=0, minFaceWeightFace=-1, minVolRatioFace=-1)])
    assert (q.avgFaceWeight, q.minVolRatio, q.avgFlatness, q.maxConcaveAngle, q.minDeterminant, q.avgDeterminant) == (1.0, 1.0, 1.0, 0.0, 0.25, 0.25)
    t = combine_quality_motion([_mpart(nTwistFaces=0)])
    assert (t.minTwist, t.avgTwist, t.avgTriangleTwist, t.minTwistFace, t.avgTetQuality) == (1.0, 1.0, 1.0, -1, 0.35)


def test_coupled_geometry_and_motion_symbols_are_exported():
    from smoothmesh_amd import _ffi
    names = ("smgpu_quality_coupled_pack_volumes", "smgpu_quality_coupled_geometry_report", "smgpu_quality_coupled_geometry_field",
             "smgpu_quality_coupled_motion_report", "smgpu_quality_coupled_motion_field")
    l = _ffi.lib()
    for s in names:
        assert s in _ffi.SYMBOLS and hasattr(l, s), s
    sums = lambda fs: [("sum" + n[3:] if n.startswith("avg") else n) for n, _ in fs]  # noqa: E731
    assert [n for n, _ in _ffi.QualityGeometryPart._fields_] == ["nCells", "nFaces", "nInternalFaces"] + sums(_ffi.QualityGeometry._fields_)
    assert [n for n, _ in _ffi.QualityMotionPart._fields_] == ["nFaces"] + sums(_ffi.QualityMotion._fields_)
    assert sorted(_gpart()) == sorted(n for n, _ in _ffi.QualityGeometryPart._fields_)
    assert sorted(_mpart()) == sorted(n for n, _ in _ffi.QualityMotionPart._fields_)
