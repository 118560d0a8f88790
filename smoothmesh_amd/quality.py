"""Mesh quality report of a decomposed mesh (DESIGN.md "Mesh quality", 10.4).

Every sub-domain's engine reports a partial record (include/smgpu.h smgpu_quality_coupled_pack / _report): its processor faces
take the internal-face definitions with the neighbour rank's cell centre, and count only on the side with the lower rank.
combine_quality folds the records in a fixed order into the report the serial engine gives for the undecomposed mesh.
Drivers: decomposed_mesh_quality (sub-domains without a point halo, one process), LocalMultiSmoother.mesh_quality and
DistributedSmoother.mesh_quality (smoothmesh_amd/halo.py); the shell tool is smoothmesh_amd/check_quality.py.
The failing elements as sets: decomposed_quality_sets, the drivers' quality_sets, write_quality_sets.
The -allGeometry checks and the motion criteria of a decomposed mesh: combine_quality_geometry,
combine_quality_motion, decomposed_mesh_quality_geometry, decomposed_mesh_quality_motion and the drivers' methods of those names.
Their findings as sets: decomposed_quality_geometry_sets, decomposed_quality_motion_sets, the drivers'
quality_geometry_sets / quality_motion_sets; write_quality_sets and format_sets_written take the table of the report.
The quality history of a run is the engine's (SmoothEngine.set_quality_trace / quality_trace); format_trace_line
and format_trace_warning give the front-end's lines of a record.  The guard on it is the engine's as well
(SmoothEngine.set_quality_guard / quality_guard / quality_guard_restore); format_guard_lines gives the front-end's two lines.
"""
from dataclasses import dataclass, fields

import numpy as np

from .engine import (MeshQuality, MeshQualityGeometry, MeshQualityMotion, QualityGuardState, QualityTraceRecord, TangleRecord, TangleState, QualityConstraintRecord, QualityConstraintState, QualityConstraintRecordFull, QualityConstraintStateFull, QualityConstraintRecordAll, QualityConstraintStateAll, QUALITY_FIELDS,  # noqa: F401
                     QUALITY_GEOMETRY_FIELDS, QUALITY_MOTION_FIELDS, QUALITY_SETS, QUALITY_GEOMETRY_SETS, QUALITY_MOTION_SETS)

QUALITY_DEFAULTS = dict(nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0)
_COUNTS = ("nNonPositiveVolume", "nZeroAreaFaces", "nSevereNonOrth", "nErrorNonOrth", "nSkewFaces", "nWrongOrientedFaces",
           "nOpenCells", "nHighAspectCells")


@dataclass
class DecomposedMeshQuality(MeshQuality):
    """MeshQuality of a decomposed mesh.  minVolumeCell, maxNonOrthFace, maxSkewFace are GLOBAL ids where every sub-domain
    carries cell / face addressing, else -1; (rank, local id) of the same elements are always filled (-1 where there is none)."""
    minVolumeRank: int = -1
    minVolumeLocal: int = -1
    maxNonOrthRank: int = -1
    maxNonOrthLocal: int = -1
    maxSkewRank: int = -1
    maxSkewLocal: int = -1


def _pick(parts, present, value, lid, ids, larger):
    """(value, global id or -1, rank, local id) of the winner: the larger (or smaller) value; a tie goes to the lowest global id
    when ids is given, else to the lowest (rank, local id)"""
    best = None
    for r, p in enumerate(parts):
        if p[present] <= 0:
            continue
        v, loc = float(p[value]), int(p[lid])
        gid = int(ids[r][loc]) if ids is not None else -1
        key = (gid,) if ids is not None else (r, loc)
        if best is None or (v > best[0] if larger else v < best[0]) or (v == best[0] and key < best[1]):
            best = (v, key, gid, r, loc)
    if best is None:
        return 0.0, -1, -1, -1
    return best[0], best[2], best[3], best[4]


def combine_quality(parts, cellIds=None, faceIds=None) -> DecomposedMeshQuality:
    """One report from the per-rank records `parts` (ascending rank; dicts with the smgpu_quality_part field names, local ids).
    cellIds[r] / faceIds[r]: local -> global id of rank r (cellProcAddressing / faceProcAddressing); the ids of the report are
    global only when every rank has both.  Rules: totals and Σθ are summed in ascending rank order, the average
    is Σθ / the global nInternalFaces; min / max ties go to the lowest global id, or to the lowest (rank, local id)."""
    parts = [dict(p) for p in parts]
    glob = (cellIds is not None and faceIds is not None and len(cellIds) == len(parts) == len(faceIds)
            and all(c is not None for c in cellIds) and all(f is not None for f in faceIds))
    cids, fids = (cellIds, faceIds) if glob else (None, None)
    out = {k: sum(int(p[k]) for p in parts) for k in ("nCells", "nFaces", "nInternalFaces") + _COUNTS}

    def ordered_sum(k):
        acc = None
        for p in parts:
            acc = float(p[k]) if acc is None else acc + float(p[k])
        return 0.0 if acc is None else acc

    def extreme(k, present, larger):
        vals = [float(p[k]) for p in parts if p[present] > 0]
        return (max(vals) if larger else min(vals)) if vals else 0.0

    out["totalVolume"] = ordered_sum("totalVolume")
    sumTh = ordered_sum("sumNonOrth")
    out["avgNonOrth"] = sumTh / out["nInternalFaces"] if out["nInternalFaces"] else 0.0
    out["maxVolume"] = extreme("maxVolume", "nCells", True)
    out["minFaceArea"] = extreme("minFaceArea", "nFaces", False)
    out["maxFaceArea"] = extreme("maxFaceArea", "nFaces", True)
    out["maxOpenness"] = extreme("maxOpenness", "nCells", True)
    out["maxAspectRatio"] = extreme("maxAspectRatio", "nCells", True)
    (out["minVolume"], out["minVolumeCell"], out["minVolumeRank"], out["minVolumeLocal"]) = \
        _pick(parts, "nCells", "minVolume", "minVolumeCell", cids, False)
    (out["maxNonOrth"], out["maxNonOrthFace"], out["maxNonOrthRank"], out["maxNonOrthLocal"]) = \
        _pick(parts, "nInternalFaces", "maxNonOrth", "maxNonOrthFace", fids, True)
    (out["maxSkewness"], out["maxSkewFace"], out["maxSkewRank"], out["maxSkewLocal"]) = \
        _pick(parts, "nFaces", "maxSkewness", "maxSkewFace", fids, True)
    return DecomposedMeshQuality(**{f.name: out[f.name] for f in fields(DecomposedMeshQuality)})


GEOMETRY_DEFAULTS = dict(concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05, volRatioThreshold=0.01,
                         determinantThreshold=0.001)
MOTION_DEFAULTS = dict(tetThreshold=1e-15, twistThreshold=0.02, triangleTwistThreshold=-1.0)


@dataclass
class DecomposedMeshQualityGeometry(MeshQualityGeometry):
    """MeshQualityGeometry of a decomposed mesh.  The five ids are GLOBAL where every sub-domain carries cell / face
    addressing, else -1; (rank, local id) of the same elements are always filled (-1 where there is none)."""
    maxConcaveRank: int = -1
    maxConcaveLocal: int = -1
    minFlatnessRank: int = -1
    minFlatnessLocal: int = -1
    minFaceWeightRank: int = -1
    minFaceWeightLocal: int = -1
    minVolRatioRank: int = -1
    minVolRatioLocal: int = -1
    minDeterminantRank: int = -1
    minDeterminantLocal: int = -1


@dataclass
class DecomposedMeshQualityMotion(MeshQualityMotion):
    """MeshQualityMotion of a decomposed mesh; ids as DecomposedMeshQualityGeometry"""
    minTetRank: int = -1
    minTetLocal: int = -1
    minBaseTetRank: int = -1
    minBaseTetLocal: int = -1
    minTwistRank: int = -1
    minTwistLocal: int = -1
    minTriangleTwistRank: int = -1
    minTriangleTwistLocal: int = -1


def _combine_rows(parts, cellIds, faceIds, counts, rows):
    """the shared rules of combine_quality_geometry / _motion (those of combine_quality).  rows: (value, id field, "cell" | "face",
    present = the count that says a rank has qualifying elements, larger, empty value, (average, sum, denominator) or None,
    stem of the Rank / Local fields)"""
    parts = [dict(p) for p in parts]
    glob = (cellIds is not None and faceIds is not None and len(cellIds) == len(parts) == len(faceIds)
            and all(c is not None for c in cellIds) and all(f is not None for f in faceIds))
    out = {k: sum(int(p[k]) for p in parts) for k in counts}
    for value, lid, kind, present, larger, empty, avg, stem in rows:
        ids = (cellIds if kind == "cell" else faceIds) if glob else None
        v, gid, rank, loc = _pick(parts, present, value, lid, ids, larger)
        out[value] = v if rank >= 0 else empty
        out[lid], out[stem + "Rank"], out[stem + "Local"] = gid, rank, loc
        if avg is not None:
            name, sumName, den = avg
            acc = None
            for p in parts:                                   # left to right in ascending rank order
                acc = float(p[sumName]) if acc is None else acc + float(p[sumName])
            n = sum(int(p[den]) for p in parts)
            out[name] = acc / n if n else empty
    return out, parts


def combine_quality_geometry(parts, cellIds=None, faceIds=None) -> DecomposedMeshQualityGeometry:
    """One -allGeometry report from the per-rank records `parts` (ascending rank; dicts with the smgpu_quality_geometry_part field
    names, local ids), by the rules of combine_quality: counts and denominators are integer sums, float sums go
    left to right in rank order, an average is its global sum over its global denominator (the serial empty-case value when that
    is 0), minima / maxima are taken over the ranks that have qualifying elements, ties to the lowest global id (else the lowest
    (rank, local id)).  maxConcaveAngle is the winning rank's own: no acos on the host."""
    rows = (("maxConcaveSin", "maxConcaveFace", "face", "nConcaveFaces", True, 0.0, None, "maxConcave"),
            ("minFlatness", "minFlatnessFace", "face", "nFlatnessFaces", False, 1.0, ("avgFlatness", "sumFlatness", "nFlatnessFaces"), "minFlatness"),
            ("minFaceWeight", "minFaceWeightFace", "face", "nInternalFaces", False, 1.0, ("avgFaceWeight", "sumFaceWeight", "nInternalFaces"),
             "minFaceWeight"),
            ("minVolRatio", "minVolRatioFace", "face", "nInternalFaces", False, 1.0, ("avgVolRatio", "sumVolRatio", "nInternalFaces"), "minVolRatio"),
            ("minDeterminant", "minDeterminantCell", "cell", "nCells", False, 0.0, ("avgDeterminant", "sumDeterminant", "nCells"),
             "minDeterminant"))
    out, parts = _combine_rows(parts, cellIds, faceIds, ("nConcaveFaces", "nFlatnessFaces", "nWarpedFaces", "nLowWeightFaces",
                                                         "nLowVolRatioFaces", "nUnderdeterminedCells"), rows)
    r = out["maxConcaveRank"]
    out["maxConcaveAngle"] = float(parts[r]["maxConcaveAngle"]) if r >= 0 else 0.0
    return DecomposedMeshQualityGeometry(**{f.name: out[f.name] for f in fields(DecomposedMeshQualityGeometry)})


def combine_quality_motion(parts, cellIds=None, faceIds=None) -> DecomposedMeshQualityMotion:
    """One motion report from the per-rank records `parts` (smgpu_quality_motion_part field names), rules as combine_quality_geometry"""
    rows = (("minTetQuality", "minTetFace", "face", "nFaces", False, 1.0, ("avgTetQuality", "sumTetQuality", "nFaces"), "minTet"),
            ("minBaseTetQuality", "minBaseTetFace", "face", "nFaces", False, 1.0, None, "minBaseTet"),
            ("minTwist", "minTwistFace", "face", "nTwistFaces", False, 1.0, ("avgTwist", "sumTwist", "nTwistFaces"), "minTwist"),
            ("minTriangleTwist", "minTriangleTwistFace", "face", "nTwistFaces", False, 1.0,
             ("avgTriangleTwist", "sumTriangleTwist", "nTwistFaces"), "minTriangleTwist"))
    out, _ = _combine_rows(parts, cellIds, faceIds, ("nLowTetFaces", "nNoBasePointFaces", "nTwistFaces", "nLowTwistFaces",
                                                     "nLowTriangleTwistFaces"), rows)
    return DecomposedMeshQualityMotion(**{f.name: out[f.name] for f in fields(DecomposedMeshQualityMotion)})


def paired_offsets(couplings):
    """For couplings[i] = (rank, [(start, size, neighbour), ...]) of every rank: [(dst index, dst slot, src index, src slot, size)]
    copies that fill every rank's recvCc from its neighbours' sendCc (slot = first face of the patch in patch order)."""
    at = {}
    for i, (rank, pats) in enumerate(couplings):
        off = 0
        for _, size, o in pats:
            at[(int(rank), int(o))] = (i, off, size)
            off += size
    copies = []
    for (r, o), (i, off, size) in at.items():
        if (o, r) not in at:
            raise ValueError(f"processor patch {r} -> {o} has no partner patch {o} -> {r}")
        j, ooff, osize = at[(o, r)]
        if osize != size:
            raise ValueError(f"processor patches {r} -> {o} and {o} -> {r} differ in size ({size}, {osize})")
        copies.append((i, off, j, ooff, size))
    return copies


def local_exchange(engines, couplings, torch_device, volumes=False):
    """pack on every engine, then fill every recvCc from the partner patches by device-side copies (one process, one device)
    -> list of recvCc tensors.  volumes: also pack_volumes on every engine, its slices moved by the same paired_offsets
    -> (list of recvCc, list of recvVc)"""
    import torch
    send, sendV = [], []
    for e, c in zip(engines, couplings):
        n = sum(p[1] for p in c[1])
        t = torch.empty((max(n, 1), 3), dtype=torch.float64, device=torch_device)
        e.quality_coupled_pack(c, t.data_ptr() if n else 0)
        send.append(t)
        if volumes:
            v = torch.empty(max(n, 1), dtype=torch.float64, device=torch_device)
            e.quality_coupled_pack_volumes(v.data_ptr() if n else 0)
            sendV.append(v)
    recv = [torch.empty_like(t) for t in send]
    recvV = [torch.empty_like(v) for v in sendV]
    for i, off, j, ooff, size in paired_offsets(couplings):
        recv[i][off:off + size].copy_(send[j][ooff:ooff + size])
        if volumes:
            recvV[i][off:off + size].copy_(sendV[j][ooff:ooff + size])
    torch.cuda.synchronize(torch_device)
    return (recv, recvV) if volumes else recv


def _ids_of(sub):
    return getattr(sub, "cellProcAddressing", None), getattr(sub, "faceProcAddressing", None)


def _all_ids(subs):
    ids = [_ids_of(s) for s in subs]
    if len(subs) == 1 and any(x is None for x in ids[0]):            # one sub-domain is the whole mesh: its local ids are the global ones
        m = getattr(subs[0], "mesh", subs[0])
        ids = [(np.arange(m.nCells), np.arange(m.nFaces))]
    return [i[0] for i in ids], [i[1] for i in ids]


@dataclass(frozen=True)
class QualityKind:
    """one report kind: its default thresholds, whether the owner cells' volumes are exchanged too, the engine's coupled report
    and field methods, the combine of the per-rank records, the record's winning cell / face ids, the engine's coupled sets
    method and the table of its sets"""
    defaults: dict
    volumes: bool
    report: str
    field: str
    combine: object
    cellIds: tuple
    faceIds: tuple
    sets: str
    table: tuple


QUALITY_KINDS = dict(
    quality=QualityKind(QUALITY_DEFAULTS, False, "quality_coupled_report", "quality_coupled_field", combine_quality,
                        ("minVolumeCell",), ("maxNonOrthFace", "maxSkewFace"), "quality_coupled_sets", QUALITY_SETS),
    geometry=QualityKind(GEOMETRY_DEFAULTS, True, "quality_coupled_geometry_report", "quality_coupled_geometry_field", combine_quality_geometry,
                         ("minDeterminantCell",), ("maxConcaveFace", "minFlatnessFace", "minFaceWeightFace", "minVolRatioFace"),
                         "quality_coupled_geometry_sets", QUALITY_GEOMETRY_SETS),
    motion=QualityKind(MOTION_DEFAULTS, False, "quality_coupled_motion_report", "quality_coupled_motion_field", combine_quality_motion,
                       (), ("minTetFace", "minBaseTetFace", "minTwistFace", "minTriangleTwistFace"), "quality_coupled_motion_sets",
                       QUALITY_MOTION_SETS))


def _local(engines, torch_device, volumes, call):
    """the exchange between the engines of one process, then [call(engine, recvCc pointer[, recvVc pointer])] in rank order"""
    couplings = [e.quality_coupling(r) for r, e in enumerate(engines)]
    recv = local_exchange(engines, couplings, torch_device, volumes=volumes)
    bufs = zip(*recv) if volumes else ((t,) for t in recv)
    return [call(e, *(t.data_ptr() for t in b)) for e, b in zip(engines, bufs)]


def _local_report(kind, engines, subs, torch_device, thresholds):
    k = QUALITY_KINDS[kind]
    parts = _local(engines, torch_device, k.volumes, lambda e, *recv: getattr(e, k.report)(*recv, **{**k.defaults, **thresholds}))
    return k.combine(parts, *_all_ids(subs))


def _local_field(kind, engines, name, torch_device):
    k = QUALITY_KINDS[kind]
    return _local(engines, torch_device, k.volumes, lambda e, *recv: getattr(e, k.field)(name, *recv))


def local_quality(engines, subs, torch_device, thresholds):
    return _local_report("quality", engines, subs, torch_device, thresholds)


def local_quality_geometry(engines, subs, torch_device, thresholds):
    return _local_report("geometry", engines, subs, torch_device, thresholds)


def local_quality_motion(engines, subs, torch_device, thresholds):
    return _local_report("motion", engines, subs, torch_device, thresholds)


def local_quality_field(engines, name, torch_device):
    return _local_field("quality", engines, name, torch_device)


def local_quality_geometry_field(engines, name, torch_device):
    return _local_field("geometry", engines, name, torch_device)


def local_quality_motion_field(engines, name, torch_device):
    return _local_field("motion", engines, name, torch_device)


def _local_sets(kind, engines, torch_device, thresholds):
    k = QUALITY_KINDS[kind]
    return _local(engines, torch_device, k.volumes, lambda e, *recv: getattr(e, k.sets)(*recv, **{**k.defaults, **thresholds}))


def local_quality_sets(engines, torch_device, thresholds):
    """[per-rank {name: local ids}]: a processor face is a member only on the rank that counts it"""
    return _local_sets("quality", engines, torch_device, thresholds)


def local_quality_geometry_sets(engines, torch_device, thresholds):
    """local_quality_sets for the sets of the -allGeometry checks; the exchange also moves the volumes"""
    return _local_sets("geometry", engines, torch_device, thresholds)


def local_quality_motion_sets(engines, torch_device, thresholds):
    """local_quality_sets for the sets of the motion criteria"""
    return _local_sets("motion", engines, torch_device, thresholds)


def _with_engines(subs, device, foam_variant, run):
    """run(engines, torch device) on one plain engine per sub-domain (decompose.SubDomain or PolyMesh, rank = position in the
    list) on one device: sub-domains that need no point halo, coupled by their processor patches only"""
    import torch
    from .engine import SmoothEngine
    meshes = [getattr(s, "mesh", s) for s in subs]
    engines = []
    try:
        for m in meshes:
            e = SmoothEngine(m, device=device)
            if len(meshes) > 1:
                e.set_device_share(len(meshes))
            if foam_variant is not None:
                e.set_foam_variant(foam_variant)
            engines.append(e)
        return run(engines, torch.device("cuda", device))
    finally:
        for e in engines:
            e.close()


def decomposed_mesh_quality(subs, device=0, foam_variant=None, **thresholds) -> DecomposedMeshQuality:
    """Quality report of a decomposed mesh whose sub-domains need no point halo (_with_engines).  Ids are global where the
    sub-domains carry cell and face addressing (a single sub-domain is the whole mesh: its own ids)."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality(engines, subs, dev, thresholds))


def decomposed_mesh_quality_geometry(subs, device=0, foam_variant=None, **thresholds) -> DecomposedMeshQualityGeometry:
    """The -allGeometry report of a decomposed mesh: the serial mesh_quality_geometry of the undecomposed mesh.
    Sub-domains, engines and ids as decomposed_mesh_quality."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality_geometry(engines, subs, dev, thresholds))


def decomposed_mesh_quality_motion(subs, device=0, foam_variant=None, **thresholds) -> DecomposedMeshQualityMotion:
    """The motion criteria of a decomposed mesh: the serial mesh_quality_motion of the undecomposed mesh.
    Sub-domains, engines and ids as decomposed_mesh_quality."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality_motion(engines, subs, dev, thresholds))


def decomposed_quality_sets(subs, device=0, foam_variant=None, **thresholds) -> list:
    """The failing elements of decomposed_mesh_quality's report as sets: one {name: local ids} per rank.
    Mapped through cell / face addressing, the ranks' sets are disjoint and their union is the undecomposed mesh's set."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality_sets(engines, dev, thresholds))


def decomposed_quality_geometry_sets(subs, device=0, foam_variant=None, **thresholds) -> list:
    """The findings of decomposed_mesh_quality_geometry's report as sets: one {name: local ids} per rank, the names of
    QUALITY_GEOMETRY_SETS; disjoint between the ranks and complete as decomposed_quality_sets'."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality_geometry_sets(engines, dev, thresholds))


def decomposed_quality_motion_sets(subs, device=0, foam_variant=None, **thresholds) -> list:
    """The findings of decomposed_mesh_quality_motion's report as sets: as decomposed_quality_geometry_sets, the names of
    QUALITY_MOTION_SETS."""
    return _with_engines(subs, device, foam_variant, lambda engines, dev: local_quality_motion_sets(engines, dev, thresholds))


def write_quality_sets(polyMeshDir, location, sets, binary=False, table=QUALITY_SETS):
    """the non-empty sets as OpenFOAM topoSet files <polyMeshDir>/sets/<name> (class faceSet / cellSet, location
    "<location>/sets"), as checkMesh writes them; compressed when polymesh.set_write_compression is on.  Nothing else in the
    directory is touched.  table: the sets' table (QUALITY_SETS, QUALITY_GEOMETRY_SETS or QUALITY_MOTION_SETS).  Returns
    [(name, size)] of the files written, in the table's order."""
    import os
    from .polymesh import write_label_list
    d = os.path.join(polyMeshDir, "sets")
    written = []
    for name, cls, _, _ in table:
        ids = np.asarray(sets.get(name, ()), dtype=np.int32)
        if ids.size == 0:
            continue
        os.makedirs(d, exist_ok=True)
        write_label_list(os.path.join(d, name), ids, location.rstrip("/") + "/sets", name, cls, binary)
        written.append((name, int(ids.size)))
    return written


def format_sets_written(written, table=QUALITY_SETS):
    """the lines smoothMesh -writeSets prints after the report block, one per written set of `table`"""
    desc = {name: words for name, _, _, words in table}
    return "".join(f"    <<Writing {n} {desc[name]} to set {name}\n" for name, n in written)


def format_geometry_lines(g):
    """the five lines -allGeometry adds to the block (csrc/host/smoothMesh_main.cpp, reportQuality), of a MeshQualityGeometry"""
    f = lambda x: "%.9g" % x  # noqa: E731
    return (f"    faceConcavity maxAngle {f(g.maxConcaveAngle)} concave {g.nConcaveFaces} maxFace {g.maxConcaveFace}\n"
            f"    faceFlatness min {f(g.minFlatness)} average {f(g.avgFlatness)} warped {g.nWarpedFaces} minFace {g.minFlatnessFace}\n"
            f"    faceWeight min {f(g.minFaceWeight)} average {f(g.avgFaceWeight)} low {g.nLowWeightFaces} minFace {g.minFaceWeightFace}\n"
            f"    volumeRatio min {f(g.minVolRatio)} average {f(g.avgVolRatio)} low {g.nLowVolRatioFaces} minFace {g.minVolRatioFace}\n"
            f"    cellDeterminant min {f(g.minDeterminant)} average {f(g.avgDeterminant)} underdetermined {g.nUnderdeterminedCells} "
            f"minCell {g.minDeterminantCell}\n")


def format_motion_lines(t):
    """the four lines -meshQuality adds to the block (csrc/host/smoothMesh_main.cpp, reportQuality), of a MeshQualityMotion"""
    f = lambda x: "%.9g" % x  # noqa: E731
    return (f"    faceTets min {f(t.minTetQuality)} average {f(t.avgTetQuality)} low {t.nLowTetFaces} minFace {t.minTetFace}\n"
            f"    faceBaseTets min {f(t.minBaseTetQuality)} noBasePoint {t.nNoBasePointFaces} minFace {t.minBaseTetFace}\n"
            f"    faceTwist min {f(t.minTwist)} average {f(t.avgTwist)} low {t.nLowTwistFaces} minFace {t.minTwistFace}\n"
            f"    triangleTwist min {f(t.minTriangleTwist)} average {f(t.avgTriangleTwist)} low {t.nLowTriangleTwistFaces} "
            f"minFace {t.minTriangleTwistFace}\n")


def format_trace_line(rec):
    """the line smoothMesh -qualityInterval prints under the iteration line of a traced iteration (csrc/host/smoothMesh_main.cpp,
    printQualityTrace), of a QualityTraceRecord"""
    g = lambda x: "%.9g" % x  # noqa: E731
    return (f"    quality iteration={rec.iteration} minVolume {g(rec.minVolume)} nonPositive {rec.nNonPositiveVolume} "
            f"maxNonOrth {g(rec.maxNonOrth)} error {rec.nErrorNonOrth} maxSkewness {g(rec.maxSkewness)} "
            f"wrongOriented {rec.nWrongOrientedFaces} maxOpenness {g(rec.maxOpenness)} maxAspectRatio {g(rec.maxAspectRatio)}\n")


def format_trace_warning(rec, initial):
    """the line printed once per run, under the first traced iteration whose nNonPositiveVolume or nWrongOrientedFaces exceeds the
    initial mesh's (`initial`: its MeshQuality)"""
    return (f"    ***Iteration {rec.iteration}: {rec.nNonPositiveVolume} non-positive volume cells and {rec.nWrongOrientedFaces} "
            f"wrongly oriented faces (initial mesh: {initial.nNonPositiveVolume}, {initial.nWrongOrientedFaces})\n")


def format_tangle_line(rec):
    """the line smoothMesh -tangleConstraint prints under the iteration line of an iteration whose nBadCells > 0 (csrc/host/
    smoothMesh_main.cpp), of a TangleRecord"""
    return (f"    tangle iteration={rec.iteration} badCells {rec.nBadCells} passes {rec.passes} pointsReverted {rec.nPointsReverted}"
            + (" fullRevert" if rec.fullRevert else "") + "\n")


def format_quality_constraint_line(rec, more=False, last=False, scaled=False):
    """the line smoothMesh -qualityConstraint prints under the iteration line of an iteration whose nBadCells > 0 (csrc/host/
    smoothMesh_main.cpp), of a QualityConstraintRecord; more: the line of a run with one of the limits of DESIGN.md 10.16 given
    (-minTetQuality ... -minDeterminant), of a QualityConstraintRecordFull; last: the line of a run with one of the limits of 10.18
    on (-maxConcave -minFlatness -minVol -minArea), which carries the six counts of 10.16 too, of a QualityConstraintRecordAll;
    scaled: the line of a run with -scalePasses > 0 (10.19), of a QualityConstraintRecordScaled: the three values of the scaling
    passes directly in front of `passes`"""
    extra = (f" lowTetFaces {rec.nLowTetFaces} twistedFaces {rec.nLowTwistFaces} lowTriangleTwistFaces {rec.nLowTriangleTwistFaces} "
             f"lowWeightFaces {rec.nLowWeightFaces} lowVolRatioFaces {rec.nLowVolRatioFaces} underdeterminedCells {rec.nUnderdeterminedCells}") if (more or last) else ""
    if last:
        extra += f" concaveFaces {rec.nConcaveFaces} warpedFaces {rec.nWarpedFaces} smallAreaFaces {rec.nSmallAreaFaces} smallVolumeCells {rec.nSmallVolumeCells}"
    scaling = f" scalePasses {rec.nScalePasses} pointsScaled {rec.nPointsScaled} minScale {rec.minScale:g}" if scaled else ""
    return (f"    quality constraint iteration={rec.iteration} badCells {rec.nBadCells} tangled {rec.nTangledCells} nonOrthoFaces {rec.nNonOrthoFaces} "
            f"skewFaces {rec.nSkewFaces}{extra}{scaling} passes {rec.passes} pointsReverted {rec.nPointsReverted}" + (" fullRevert" if rec.fullRevert else "") + "\n")


def format_quality_constraint_limits_line(state):
    """the second set-up line of smoothMesh -qualityConstraint with one of the limits of DESIGN.md 10.16 given: the limits that are
    on, in the order of smgpu_quality_constraint_limits, and the determinant-exempt cells; of a QualityConstraintStateFull.  With one
    of the limits of 10.18 on (a QualityConstraintStateAll) the line lists it behind the six and gains the volume-exempt cells"""
    from .engine import QUALITY_CONSTRAINT_LIMITS_ALL_OFF, QUALITY_CONSTRAINT_LIMITS_OFF, quality_constraint_limits_all_on
    on = "".join(f" {k} {getattr(state, k):g}" for k, off in QUALITY_CONSTRAINT_LIMITS_OFF.items() if getattr(state, k) > off)
    last = quality_constraint_limits_all_on(**{k: getattr(state, k, None) for k in QUALITY_CONSTRAINT_LIMITS_ALL_OFF})
    on += "".join(f" {k} {v:g}" for k, v in last.items())
    tail = f", {state.nExemptVolumeCells} volume-exempt cells" if last else ""
    return f"Quality constraint limits:{on}, {state.nExemptDeterminantCells} determinant-exempt cells{tail}\n"


def format_quality_constraint_scaling_line(state):
    """the set-up line of smoothMesh -qualityConstraint with -scalePasses > 0, behind the other set-up lines of
    the constraint; of a QualityConstraintStateScaled"""
    return f"Quality constraint scaling: scalePasses {state.scalePasses} errorReduction {state.errorReduction:g} nSmoothScale {state.nSmoothScale}\n"


# the keys smhost_read_mesh_quality_dict reads, in the order of its arrays (include/smhost.h)
MESH_QUALITY_DICT_KEYS = ("maxNonOrtho", "maxBoundarySkewness", "maxInternalSkewness", "maxConcave", "minFlatness", "minVol", "minTetQuality", "minArea",
                          "minTwist", "minDeterminant", "minFaceWeight", "minVolRatio", "minTriangleTwist")


class MeshQualityLimits(dict):
    """read_mesh_quality_dict's answer: {limit: value} of the keys the file gives, keyword arguments of
    SmoothEngine.set_quality_constraint and of the smoothers' set_quality_constraint_limits_all; `ignored`: the file's other top-level
    keys; `path`: the file"""
    ignored = ()
    path = None


def read_mesh_quality_dict(path, etc_dirs=None):
    """The limits of an OpenFOAM system/meshQualityDict (DESIGN.md "Mesh quality", 10.18), read by the host library's parser
    (include/smhost.h, smhost_read_mesh_quality_dict: the one `smoothMesh -meshQualityDict` uses): a MeshQualityLimits, so that
    eng.set_quality_constraint(**d) and ms.set_quality_constraint_limits_all(**d) apply the file.  A key the file does not give is
    absent and keeps the call's default; OpenFOAM's disabling values (-1e30, -1, 180, 0) lie in the engine's off ranges.
    etc_dirs: where #includeEtc looks, in order; None: $WM_PROJECT_DIR/etc and $FOAM_ETC, where set.  The relaxed sub-dictionary
    and snappyHexMesh's own keys are not read: they are listed in `ignored`.  A malformed file raises RuntimeError naming file
    and line."""
    import ctypes as C
    import os
    from . import polymesh
    if etc_dirs is None:
        etc_dirs = [os.path.join(os.environ["WM_PROJECT_DIR"], "etc")] if os.environ.get("WM_PROJECT_DIR") else []
        etc_dirs += [os.environ["FOAM_ETC"]] if os.environ.get("FOAM_ETC") else []
    lib = polymesh.lib()
    lib.smhost_read_mesh_quality_dict.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p,
                                                  C.POINTER(C.c_int64)]
    n = len(MESH_QUALITY_DICT_KEYS)
    dirs = (C.c_char_p * max(1, len(etc_dirs)))(*[os.fspath(d).encode() for d in etc_dirs])
    values, found, size = (C.c_double * n)(), (C.c_int32 * n)(), C.c_int64(4096)
    while True:
        buf = C.create_string_buffer(size.value)
        have = size.value
        if lib.smhost_read_mesh_quality_dict(os.fspath(path).encode(), dirs, len(etc_dirs), values, found, buf, C.byref(size)):
            raise RuntimeError(lib.smhost_last_error().decode())
        if size.value <= have:
            break
    out = MeshQualityLimits((k, float(values[i])) for i, k in enumerate(MESH_QUALITY_DICT_KEYS) if found[i])
    out.ignored = tuple(x for x in buf.value.decode().split("\n") if x)
    out.path = os.fspath(path)
    return out


def format_guard_lines(state):
    """the two lines smoothMesh -qualityGuard prints under the lines of the chunk in which the guard tripped (csrc/host/
    smoothMesh_main.cpp), of a QualityGuardState that has tripped"""
    t, b = state.tripRecord, state.baseline
    return (f"    ***Quality guard: iteration {state.trippedIteration}: {t.nNonPositiveVolume} non-positive volume cells and "
            f"{t.nWrongOrientedFaces} wrongly oriented faces (initial mesh: {b.nNonPositiveVolume}, {b.nWrongOrientedFaces})\n"
            f"    ***Quality guard: restored the mesh of iteration {state.restoredIteration}, stopping.\n")


def format_report(q, which="mesh", geometry=None, motion=None):
    """the block smoothMesh -checkQuality prints (csrc/host/smoothMesh_main.cpp, reportQuality); geometry: the MeshQualityGeometry
    whose lines -allGeometry adds before the block's blank line; motion: the MeshQualityMotion whose lines -meshQuality adds after them"""
    g = lambda x: "%.9g" % x  # noqa: E731
    lines = [f"Mesh quality ({which}):",
             f"    cells {q.nCells} faces {q.nFaces} internalFaces {q.nInternalFaces}",
             f"    cellVolume min {g(q.minVolume)} max {g(q.maxVolume)} total {g(q.totalVolume)} nonPositive {q.nNonPositiveVolume} "
             f"minCell {q.minVolumeCell}",
             f"    faceArea min {g(q.minFaceArea)} max {g(q.maxFaceArea)} zero {q.nZeroAreaFaces}",
             f"    nonOrthogonality max {g(q.maxNonOrth)} average {g(q.avgNonOrth)} severe {q.nSevereNonOrth} error {q.nErrorNonOrth} "
             f"maxFace {q.maxNonOrthFace}",
             f"    skewness max {g(q.maxSkewness)} severe {q.nSkewFaces} maxFace {q.maxSkewFace}",
             f"    facePyramids wrongOriented {q.nWrongOrientedFaces}",
             f"    cellOpenness max {g(q.maxOpenness)} open {q.nOpenCells}",
             f"    cellAspectRatio max {g(q.maxAspectRatio)} high {q.nHighAspectCells}"]
    if q.nNonPositiveVolume > 0 or q.nWrongOrientedFaces > 0:
        lines.append(f"    ***Mesh has {q.nNonPositiveVolume} non-positive volume cells and {q.nWrongOrientedFaces} wrongly oriented faces")
    return ("\n".join(lines) + "\n" + (format_geometry_lines(geometry) if geometry is not None else "")
            + (format_motion_lines(motion) if motion is not None else "") + "\n")
