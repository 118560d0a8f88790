"""Host-side mirror of the C-ABI (include/smgpu.h): one SmoothEngine = one rank's fvMesh in the
reference's loop (src/smoothMesh.C:2257-2437).  Parameter names are the reference's command-line
option names (SM.C:1642-1784), defaults as SM.C:1857-1918."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi
from .mesh import PolyMesh


class SmgpuError(RuntimeError):
    """A non-zero status from the library (the reference would FatalError/abort here)."""


@dataclass
class SmoothParams:
    maxStepLength: float
    minEdgeLength: float
    relStepFrac: float = 0.5
    totalMinFreeze: bool = False
    edgeAngleConstraint: bool = True
    faceAngleConstraint: bool = True
    minAngle: float = 35.0
    maxAngle: float = 160.0


@dataclass
class LayerParams:
    """Boundary layer treatment options (SM.C:1749-1775), defaults SM.C:1892-1905."""
    layerPatches: tuple = ()                  # patch names; a name in double quotes is a regular expression
    layerMaxBlendingFraction: float = 0.3
    layerEdgeLength: Optional[float] = None   # None = minEdgeLength
    layerExpansionRatio: float = 1.3
    minLayers: int = 1
    maxLayers: int = 4


@dataclass
class BoundaryParams:
    """Boundary point smoothing inputs: the contents of constant/geometry/{initEdges,targetEdges,targetSurfaces}.obj
    (SM.C:1924-1926) and the options SM.C:1758-1770, 1907."""
    initEdges: tuple = None                   # (points (n,3), edges (m,2))
    targetSurfaces: tuple = None              # (points (n,3), triangles (m,3))
    targetEdges: tuple = None                 # None = the initial edges are the target (SM.C:2154-2160)
    smoothingPatches: tuple = ('".*"',)       # default: every patch (SM.C:1837-1840)
    internalSmoothingBlendingFraction: float = 0.0
    isCornerPointIO: object = None            # classification lists of a previous run (SM.C:2039-2077)
    isFeatureEdgePointIO: object = None


@dataclass
class MeshQuality:
    """smgpu_mesh_quality's report of the engine's current points (include/smgpu.h; definitions: DESIGN.md "Mesh quality")."""
    nCells: int
    nFaces: int
    nInternalFaces: int
    minVolume: float
    maxVolume: float
    totalVolume: float
    nNonPositiveVolume: int
    minVolumeCell: int
    minFaceArea: float
    maxFaceArea: float
    nZeroAreaFaces: int
    maxNonOrth: float
    avgNonOrth: float
    nSevereNonOrth: int
    nErrorNonOrth: int
    maxNonOrthFace: int
    maxSkewness: float
    nSkewFaces: int
    maxSkewFace: int
    nWrongOrientedFaces: int
    maxOpenness: float
    nOpenCells: int
    maxAspectRatio: float
    nHighAspectCells: int


@dataclass
class QualityTraceRecord:
    """One record of the run's quality history (include/smgpu.h, smgpu_quality_trace_record; DESIGN.md "Mesh quality", 10.10): the
    fields of MeshQuality that do not depend on the order of a floating-point sum, of the points after iteration `iteration`
    (1-based, counted since set_quality_trace).  Every field has the bits mesh_quality() gives for the same points."""
    iteration: int
    minVolume: float
    maxVolume: float
    nNonPositiveVolume: int
    minVolumeCell: int
    minFaceArea: float
    maxFaceArea: float
    nZeroAreaFaces: int
    maxNonOrth: float
    nSevereNonOrth: int
    nErrorNonOrth: int
    maxNonOrthFace: int
    maxSkewness: float
    nSkewFaces: int
    maxSkewFace: int
    nWrongOrientedFaces: int
    maxOpenness: float
    nOpenCells: int
    maxAspectRatio: float
    nHighAspectCells: int


# the criteria of the quality guard (include/smgpu.h, SMGPU_GUARD_*): name -> bit, in the order the reasons are listed
QUALITY_GUARD_CRITERIA = {"nonPositiveVolume": 1, "wrongOriented": 2, "errorNonOrth": 4}


@dataclass
class QualityGuardState:
    """The state of the guard on the quality history (include/smgpu.h, smgpu_quality_guard_state; DESIGN.md "Mesh quality", 10.11).
    The iterations are trace numbers; `reasons`: the names of the criteria that tripped, in QUALITY_GUARD_CRITERIA's order;
    `baseline`: the trace's record of the points at arming (iteration 0); `tripRecord`: the record that tripped, or None."""
    armed: bool
    tripped: bool
    reasons: tuple
    snapshotIteration: int
    trippedIteration: int
    restoredIteration: int
    baseline: QualityTraceRecord
    tripRecord: Optional[QualityTraceRecord]


@dataclass
class TangleRecord:
    """One record of the tangle constraint (include/smgpu.h, smgpu_tangle_record; DESIGN.md "Mesh quality", 10.12), of iteration
    `iteration` (1-based, counted since set_tangle_constraint): `nBadCells` cells that are not exempt were bad after the loop's
    move, `passes` evaluations reverted the points of such cells, `fullRevert` says whether every point went back in the end, and
    `nPointsReverted` points ended where the iteration found them although the loop had moved them."""
    iteration: int
    passes: int
    fullRevert: int
    nBadCells: int
    nPointsReverted: int


@dataclass
class QualityConstraintRecord:
    """One record of the quality constraint (include/smgpu.h, smgpu_quality_constraint_record; DESIGN.md "Mesh quality", 10.14), of
    iteration `iteration` (1-based, counted since set_quality_constraint).  iteration, passes, fullRevert and nPointsReverted are
    TangleRecord's; `nBadCells` cells were bad after the loop's move -- `nTangledCells` of them by the tangle constraint's
    definition, the others as the owner or the neighbour of one of the `nNonOrthoFaces` faces over the non-orthogonality limit
    or the `nSkewFaces` faces over a skewness limit (a face over both counts in both; exempt elements never count)."""
    iteration: int
    passes: int
    fullRevert: int
    nBadCells: int
    nPointsReverted: int
    nTangledCells: int
    nNonOrthoFaces: int
    nSkewFaces: int


@dataclass
class QualityConstraintState:
    """smgpu_quality_constraint_state: whether the constraint is on, its passes and limits, the cells and faces exempt since
    enabling, the running number"""
    on: bool
    passes: int
    maxNonOrtho: float
    maxInternalSkewness: float
    maxBoundarySkewness: float
    nExemptCells: int
    nExemptFaces: int
    iteration: int


# the limits of DESIGN.md "Mesh quality", 10.16, in the order of smgpu_quality_constraint_limits, with the value at or below
# which each is off
QUALITY_CONSTRAINT_LIMITS_OFF = dict(minTetQuality=-1e30, minTwist=-1.0, minTriangleTwist=-1.0, minFaceWeight=0.0, minVolRatio=0.0, minDeterminant=0.0)


def quality_constraint_limits_on(**limits):
    """the limits of QUALITY_CONSTRAINT_LIMITS_OFF among `limits` that are on (None: off; a NaN counts, to be refused), by name"""
    bad = set(limits) - set(QUALITY_CONSTRAINT_LIMITS_OFF)
    if bad:
        raise TypeError(f"set_quality_constraint: unknown limit {sorted(bad)[0]}")
    return {k: float(v) for k, v in limits.items() if v is not None and not float(v) <= QUALITY_CONSTRAINT_LIMITS_OFF[k]}


@dataclass
class QualityConstraintRecordFull(QualityConstraintRecord):
    """smgpu_quality_constraint_record_full (DESIGN.md "Mesh quality", 10.16): QualityConstraintRecord, then the faces that were
    bad after the loop's move by tet quality, twist, triangle twist, interpolation weight and volume ratio and the cells under
    the determinant limit (a face that fails several counts in each; exempt elements never count).  All 0 while none of these
    limits is on."""
    nLowTetFaces: int = 0
    nLowTwistFaces: int = 0
    nLowTriangleTwistFaces: int = 0
    nLowWeightFaces: int = 0
    nLowVolRatioFaces: int = 0
    nUnderdeterminedCells: int = 0


@dataclass
class QualityConstraintStateFull(QualityConstraintState):
    """smgpu_quality_constraint_state_full: QualityConstraintState, then the six limits of 10.16 (their off values while they are
    off) and the cells exempt from the determinant limit"""
    minTetQuality: float = -1e30
    minTwist: float = -1.0
    minTriangleTwist: float = -1.0
    minFaceWeight: float = 0.0
    minVolRatio: float = 0.0
    minDeterminant: float = 0.0
    nExemptDeterminantCells: int = 0


# the limits of DESIGN.md "Mesh quality", 10.18, in the order of smgpu_quality_constraint_limits_all's tail, with the value at
# which each is off (maxConcave: at or above it; the others: at or below it)
QUALITY_CONSTRAINT_LIMITS_ALL_OFF = dict(maxConcave=180.0, minFlatness=0.0, minVol=0.0, minArea=0.0)


def quality_constraint_limits_all_on(**limits):
    """the limits of QUALITY_CONSTRAINT_LIMITS_ALL_OFF among `limits` that are on (None: off; a NaN counts, to be refused), by name"""
    bad = set(limits) - set(QUALITY_CONSTRAINT_LIMITS_ALL_OFF)
    if bad:
        raise TypeError(f"set_quality_constraint: unknown limit {sorted(bad)[0]}")
    return {k: float(v) for k, v in limits.items()
            if v is not None and not (float(v) >= 180.0 if k == "maxConcave" else float(v) <= QUALITY_CONSTRAINT_LIMITS_ALL_OFF[k])}


@dataclass
class QualityConstraintRecordAll(QualityConstraintRecordFull):
    """smgpu_quality_constraint_record_all (DESIGN.md "Mesh quality", 10.18): QualityConstraintRecordFull, then the faces that were
    bad after the loop's move by concavity, flatness and area and the cells under the volume limit (a face that fails several
    counts in each; exempt elements never count).  All 0 while none of these limits is on."""
    nConcaveFaces: int = 0
    nWarpedFaces: int = 0
    nSmallAreaFaces: int = 0
    nSmallVolumeCells: int = 0


@dataclass
class QualityConstraintStateAll(QualityConstraintStateFull):
    """smgpu_quality_constraint_state_all: QualityConstraintStateFull, then the four limits of 10.18 (their off values while they
    are off) and the cells exempt from the volume limit"""
    maxConcave: float = 180.0
    minFlatness: float = 0.0
    minVol: float = 0.0
    minArea: float = 0.0
    nExemptVolumeCells: int = 0


# the entries of include/smgpu.h by tier: the three limits only (10.14), with the six (10.16), with the four (10.18); a coupled
# entry is the serial one's name + "_coupled"
_QC_ENTRIES = (("smgpu_set_quality_constraint", _ffi.QualityConstraintParams), ("smgpu_set_quality_constraint_limits", _ffi.QualityConstraintLimits),
               ("smgpu_set_quality_constraint_limits_all", _ffi.QualityConstraintLimitsAll))


def quality_constraint_request(maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes, limits, least=0):
    """(ctypes struct, tier) of the entry of _QC_ENTRIES a set of limits takes: the narrowest that holds every limit given (not
    None), and none below `least`; a limit that is None goes in at its off value.  limits: by name, those of
    QUALITY_CONSTRAINT_LIMITS_OFF and QUALITY_CONSTRAINT_LIMITS_ALL_OFF"""
    off = {**QUALITY_CONSTRAINT_LIMITS_OFF, **QUALITY_CONSTRAINT_LIMITS_ALL_OFF}
    given = {k for k, v in limits.items() if v is not None}
    tier = max(least, 2 if given & set(QUALITY_CONSTRAINT_LIMITS_ALL_OFF) else 1 if given else 0)
    ctype = _QC_ENTRIES[tier][1]
    more = {k: off[k] if limits.get(k) is None else float(limits[k]) for k, _ in ctype._fields_[4:]}
    return ctype(float(maxNonOrtho), float(maxInternalSkewness), float(maxBoundarySkewness), int(passes), **more), tier


@dataclass
class QualityConstraintRecordScaled(QualityConstraintRecordAll):
    """smgpu_quality_constraint_record_scaled (DESIGN.md "Mesh quality", 10.19): QualityConstraintRecordAll, then the marked passes
    that scaled (k < scalePasses), the points that keep a fraction of their move (accepted 0 < s < 1, moved by the loop) and the
    smallest accepted scale (1.0 in a clean iteration, 0 after a full revert).  nPointsReverted reads the accepted points; passes
    counts scaling and reverting passes.  All three 0 while scaling is off."""
    nScalePasses: int = 0
    nPointsScaled: int = 0
    minScale: float = 0.0


@dataclass
class QualityConstraintStateScaled(QualityConstraintStateAll):
    """smgpu_quality_constraint_state_scaled: QualityConstraintStateAll, then the parameters of 10.19 (scalePasses 0: off)"""
    scalePasses: int = 0
    nSmoothScale: int = 4
    errorReduction: float = 0.75


@dataclass
class TangleState:
    """smgpu_tangle_state: whether the constraint is on, its passes, the cells exempt since enabling, the running number"""
    on: bool
    passes: int
    nExemptCells: int
    iteration: int


QUALITY_FIELDS = ("cellVolume", "cellOpenness", "cellAspectRatio", "faceNonOrthogonality", "faceSkewness")
# the failing elements of the report as sets (DESIGN.md "Mesh quality", 10.5), in smgpu_quality_sets' order: name, topoSet class,
# the report counts whose sum is the set's size, and the words of the "<<Writing" line
QUALITY_SETS = (
    ("nonOrthoFaces", "faceSet", ("nSevereNonOrth", "nErrorNonOrth"), "non-orthogonal faces"),
    ("skewFaces", "faceSet", ("nSkewFaces",), "skew faces"),
    ("wrongOrientedFaces", "faceSet", ("nWrongOrientedFaces",), "wrongly oriented faces"),
    ("zeroAreaFaces", "faceSet", ("nZeroAreaFaces",), "zero area faces"),
    ("zeroVolumeCells", "cellSet", ("nNonPositiveVolume",), "zero or negative volume cells"),
    ("nonClosedCells", "cellSet", ("nOpenCells",), "non-closed cells"),
    ("highAspectRatioCells", "cellSet", ("nHighAspectCells",), "high aspect ratio cells"),
)


@dataclass
class MeshQualityGeometry:
    """smgpu_mesh_quality_geometry's report of the engine's current points: the checks `checkMesh -allGeometry` adds
    (include/smgpu.h; definitions: DESIGN.md "Mesh quality", 10.6)."""
    nConcaveFaces: int
    maxConcaveSin: float
    maxConcaveAngle: float
    maxConcaveFace: int
    minFlatness: float
    avgFlatness: float
    nFlatnessFaces: int
    nWarpedFaces: int
    minFlatnessFace: int
    minFaceWeight: float
    avgFaceWeight: float
    nLowWeightFaces: int
    minFaceWeightFace: int
    minVolRatio: float
    avgVolRatio: float
    nLowVolRatioFaces: int
    minVolRatioFace: int
    minDeterminant: float
    avgDeterminant: float
    nUnderdeterminedCells: int
    minDeterminantCell: int


QUALITY_GEOMETRY_FIELDS = ("faceConcavity", "faceFlatness", "faceWeight", "faceVolumeRatio", "cellDeterminant")


@dataclass
class MeshQualityMotion:
    """smgpu_mesh_quality_motion's report of the engine's current points: the motion criteria, i.e. the meshQualityDict checks the
    other two reports do not cover (include/smgpu.h; definitions: DESIGN.md "Mesh quality", 10.7)."""
    minTetQuality: float
    avgTetQuality: float
    nLowTetFaces: int
    minTetFace: int
    minBaseTetQuality: float
    nNoBasePointFaces: int
    minBaseTetFace: int
    minTwist: float
    avgTwist: float
    nTwistFaces: int
    nLowTwistFaces: int
    minTwistFace: int
    minTriangleTwist: float
    avgTriangleTwist: float
    nLowTriangleTwistFaces: int
    minTriangleTwistFace: int


QUALITY_MOTION_FIELDS = ("faceTetQuality", "faceBaseTetQuality", "faceTwist", "faceTriangleTwist")
# the findings of the two reports above as sets (DESIGN.md "Mesh quality", 10.9), in smgpu_quality_geometry_sets' and
# smgpu_quality_motion_sets' order; the 4-tuples of QUALITY_SETS, the counts being fields of MeshQualityGeometry / MeshQualityMotion
QUALITY_GEOMETRY_SETS = (
    ("concaveFaces", "faceSet", ("nConcaveFaces",), "concave faces"),
    ("warpedFaces", "faceSet", ("nWarpedFaces",), "warped faces"),
    ("lowWeightFaces", "faceSet", ("nLowWeightFaces",), "faces with low interpolation weight"),
    ("lowVolRatioFaces", "faceSet", ("nLowVolRatioFaces",), "faces with low volume ratio"),
    ("underdeterminedCells", "cellSet", ("nUnderdeterminedCells",), "under-determined cells"),
)
QUALITY_MOTION_SETS = (
    ("lowQualityTetFaces", "faceSet", ("nLowTetFaces",), "faces with low quality or negative volume decomposition tets"),
    ("noBasePointFaces", "faceSet", ("nNoBasePointFaces",), "faces without a valid tet base point"),
    ("twistedFaces", "faceSet", ("nLowTwistFaces",), "twisted faces"),
    ("lowTriangleTwistFaces", "faceSet", ("nLowTriangleTwistFaces",), "faces with low triangle twist"),
)


def patch_arrays(mesh: PolyMesh, layerPatches):
    """(start, size, kind, isLayer) of mesh.patches; kind 0 ordinary / 1 processor / 2 empty.  Selection as
    polyBoundaryMesh::patchSet (SM.C:1442-1471): a plain word matches a patch name, a quoted string is a regex."""
    import re
    pats = []
    for w in layerPatches:
        w = str(w)
        pats.append(re.compile(w[1:-1]) if len(w) >= 2 and w[0] == '"' and w[-1] == '"' else w)
    kinds = {"processor": 1, "empty": 2}
    start = np.array([p.startFace for p in mesh.patches], np.int32)
    size = np.array([p.nFaces for p in mesh.patches], np.int32)
    kind = np.array([kinds.get(p.type, 0) for p in mesh.patches], np.uint8)
    sel = np.array([any((q.fullmatch(p.name) is not None) if hasattr(q, "fullmatch") else (q == p.name) for q in pats)
                    for p in mesh.patches], np.uint8)
    return start, size, kind, sel


def default_params(meshMinEdgeLength: float, **over) -> SmoothParams:
    """SM.C:1861-1865: minEdgeLength = 0.5 * mesh min edge, maxStepLength = 0.3 * minEdgeLength."""
    minEdge = over.pop("minEdgeLength", 0.5 * meshMinEdgeLength)
    maxStep = over.pop("maxStepLength", 0.3 * minEdge)
    return SmoothParams(maxStepLength=maxStep, minEdgeLength=minEdge, **over)


def _p(a, t):
    return a.ctypes.data_as(t)


def make_desc(mesh: PolyMesh, isInternalPoint, isSmoothingSurfacePoint, device=0, stream=None):
    keep = dict(
        pts=np.ascontiguousarray(mesh.points, dtype=np.float64),
        fo=mesh.faceOffsets, fp=mesh.facePoints, ow=mesh.owner, ne=mesh.neighbour,
        ip=np.ascontiguousarray(isInternalPoint, dtype=np.uint8),
        sp=None if isSmoothingSurfacePoint is None else np.ascontiguousarray(isSmoothingSurfacePoint, dtype=np.uint8),
    )
    d = _ffi.MeshDesc()
    d.nPoints, d.nCells, d.nFaces, d.nInternalFaces = mesh.nPoints, mesh.nCells, mesh.nFaces, mesh.nInternalFaces
    d.points = _p(keep["pts"], _ffi.c_f64p)
    d.faceOffsets = _p(keep["fo"], _ffi.c_i32p)
    d.facePoints = _p(keep["fp"], _ffi.c_i32p)
    d.owner = _p(keep["ow"], _ffi.c_i32p)
    d.neighbour = _p(keep["ne"], _ffi.c_i32p)
    d.isInternalPoint = _p(keep["ip"], _ffi.c_u8p)
    d.isSmoothingSurfacePoint = _p(keep["sp"], _ffi.c_u8p) if keep["sp"] is not None else None
    d.device = device
    d.stream = stream if stream else None      # stream: None = library-owned stream; an int handle
    d.useCallerStream = 0 if stream is None else 1   # (0 = the HIP null stream) = run on the caller's
    return d, keep


TOPO_ARRAYS = ["sizes and maxima", "facePoints.off", "facePoints.val", "owner", "neighbour", "cellFacesGeom.off", "cellFacesGeom.val",
               "pointFaces.off", "pointFaces.val", "pfPrev", "pfNext", "pfPrevSlot", "pfNextSlot", "pointCells.off", "pointCells.val",
               "edges", "pointEdges.off", "pointEdges.val", "pointPoints", "edgeFaces.off", "edgeFaces.val", "edgeCells.off", "edgeCells.val",
               "ecFace0", "ecFace1", "ringFace", "ringCell", "edgeRingOk"]


class HostTopology:
    """Host-only addressing build (no GPU): the library's derived lists, for checks and hosts."""

    def __init__(self, mesh: PolyMesh):
        self._lib = _ffi.lib()
        d, self._keep = make_desc(mesh, np.ones(mesh.nPoints, np.uint8), None)
        self._h = C.c_void_p()
        if self._lib.smgpu_topology_create(C.byref(d), C.byref(self._h)):
            raise SmgpuError(self._lib.smgpu_last_error().decode())

    def addressing(self, kind):
        nnz = C.c_int64()
        k = kind.encode()
        if self._lib.smgpu_topology_get(self._h, k, None, None, C.byref(nnz)):
            raise SmgpuError(self._lib.smgpu_last_error().decode())
        vals = np.empty(nnz.value, np.int32)
        if kind == "edges":
            self._lib.smgpu_topology_get(self._h, k, None, _p(vals, _ffi.c_i32p), C.byref(nnz))
            return None, vals.reshape(-1, 2)
        rows = {"pointCells": "P", "pointPoints": "P", "pointEdges": "P", "pointFaces": "P", "pointFacePrev": "P",
                "pointFaceNext": "P", "edgeFaces": "E", "edgeCells": "E", "cellFacesGeom": "C"}[kind]
        n = {"P": self._keep["pts"].shape[0], "E": self.num_edges(), "C": int(self._keep["ow"].max()) + 1}[rows]
        off = np.empty(n + 1, np.int32)
        self._lib.smgpu_topology_get(self._h, k, _p(off, _ffi.c_i32p), _p(vals, _ffi.c_i32p), C.byref(nnz))
        return off, vals

    def num_edges(self):
        n = C.c_int32()
        self._lib.smgpu_topology_num_edges(self._h, C.byref(n))
        return n.value

    def checksums(self):
        """FNV-1a checksums of every array of the addressing, TOPO_ARRAYS order (include/smgpu.h smgpu_topology_checksums)"""
        out = (C.c_uint64 * 64)()
        if self._lib.smgpu_topology_checksums(self._h, out):
            raise SmgpuError(self._lib.smgpu_last_error().decode())
        return [int(x) for x in out][:len(TOPO_ARRAYS)]

    def close(self):
        if self._h:
            self._lib.smgpu_topology_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SmoothEngine:
    def __init__(self, mesh: PolyMesh, isInternalPoint=None, isSmoothingSurfacePoint=None, device=0, stream=None):
        self._lib = _ffi.lib()
        self.mesh = mesh
        if isInternalPoint is None:
            isInternalPoint = mesh.find_internal_points()
        if isSmoothingSurfacePoint is None:
            isSmoothingSurfacePoint = mesh.smoothing_surface_points()
        self.isInternalPoint = np.ascontiguousarray(isInternalPoint, dtype=np.uint8)
        d, keep = make_desc(mesh, self.isInternalPoint, isSmoothingSurfacePoint, device, stream)
        self._h = C.c_void_p()
        self._check(self._lib.smgpu_create(C.byref(d), C.byref(self._h)))
        self.nPoints = mesh.nPoints
        self._keepalive = []

    def _check(self, rc):
        if rc:
            raise SmgpuError(self._lib.smgpu_last_error().decode())

    def _drain(self, getter, ctype, record):
        """the pending records behind `getter` (a count call, then the read, which clears them) as `record` dataclasses"""
        n = C.c_int64(0)
        self._check(getter(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        buf = (ctype * n.value)()
        self._check(getter(self._h, buf, n.value, C.byref(n)))
        return [record(**{f: getattr(r, f) for f, _ in r._fields_}) for r in buf[:n.value]]

    def _read_state(self, getter, ctype, state):
        """the struct behind `getter` as a `state` dataclass, `on` a bool"""
        s = ctype()
        self._check(getter(self._h, C.byref(s)))
        return state(**{f: bool(s.on) if f == "on" else getattr(s, f) for f, _ in s._fields_})

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup ---------------------------------------------------------------------------------
    def sizes(self):
        s = _ffi.Sizes()
        self._check(self._lib.smgpu_get_sizes(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in s._fields_}

    def mesh_stats(self):
        """getMeshStats, SM.C:1478-1541 -> (meshMinEdgeLength, meshMaxEdgeLength)."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.smgpu_mesh_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_params(self, p: SmoothParams):
        q = _ffi.Params(p.maxStepLength, p.relStepFrac, p.minEdgeLength, int(p.totalMinFreeze),
                        int(p.edgeAngleConstraint), int(p.faceAngleConstraint), p.minAngle, p.maxAngle)
        self._check(self._lib.smgpu_set_params(self._h, C.byref(q)))
        self.params = p

    def set_foam_variant(self, variant):
        """"com" (OpenFOAM.com v2312-v2506, default) or "org" (OpenFOAM.org 12): whose face / cell geometry formulas the
        cell centres follow (the reference builds against either, Allwmake:47)"""
        self._check(self._lib.smgpu_set_foam_variant(self._h, {"com": 0, "org": 1}[variant]))

    def set_sync_variant(self, variant):
        """"master" (default: globalMeshData::syncData -- the master's fold handed to every sharer) or "own" (every sharer folds the
        others' values onto its own): the syncTools::syncPointList model of the multi-rank magnitude folds (include/smgpu.h)"""
        self._check(self._lib.smgpu_set_sync_variant(self._h, {"master": 0, "own": 1}[variant]))

    # -- the loop ------------------------------------------------------------------------------
    def _layer_desc(self, lp: LayerParams, minEdgeLength: float):
        start, size, kind, sel = patch_arrays(self.mesh, lp.layerPatches)
        d = _ffi.LayerDesc()
        d.nPatches = len(start)
        d.patchStart, d.patchSize = _p(start, _ffi.c_i32p), _p(size, _ffi.c_i32p)
        d.patchKind, d.isLayerPatch = _p(kind, _ffi.c_u8p), _p(sel, _ffi.c_u8p)
        d.layerMaxBlendingFraction = lp.layerMaxBlendingFraction
        d.layerEdgeLength = minEdgeLength if lp.layerEdgeLength is None else lp.layerEdgeLength
        d.layerExpansionRatio = lp.layerExpansionRatio
        d.minLayers, d.maxLayers = lp.minLayers, lp.maxLayers
        return d, (start, size, kind, sel)

    # step-wise set-up for runs with a halo (see include/smgpu.h, smgpu_layers_begin)
    LAYERS_HOPS_SWEEP, LAYERS_NORMALS_ACCUMULATE, LAYERS_NORMALS_FINISH, LAYERS_PROPAGATE_SWEEP, LAYERS_FINISH = range(5)
    LAYERS_F_HOPS, LAYERS_F_NORMALS_COUNT, LAYERS_F_NORMALS = range(3)
    _LAYER_FIELD_WIDTH = (1, 4, 3)

    def layers_begin(self, lp: LayerParams, minEdgeLength: float):
        d, keep = self._layer_desc(lp, minEdgeLength)
        on, it = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.smgpu_layers_begin(self._h, C.byref(d), C.byref(on), C.byref(it)))
        return bool(on.value), it.value

    def layers_step(self, step, arg=0):
        self._check(self._lib.smgpu_layers_step(self._h, int(step), int(arg)))

    def layers_shared_get(self, field):
        v = np.zeros((self._nShared, self._LAYER_FIELD_WIDTH[field]), np.float64)
        if self._nShared:
            self._check(self._lib.smgpu_layers_shared(self._h, int(field), 0, _p(v, _ffi.c_f64p)))
        return v

    def layers_shared_set(self, field, values):
        v = np.ascontiguousarray(values, np.float64).reshape(self._nShared, self._LAYER_FIELD_WIDTH[field])
        if self._nShared:
            self._check(self._lib.smgpu_layers_shared(self._h, int(field), 1, _p(v, _ffi.c_f64p)))

    def l_doubles(self):
        """doubles per slot of the exchange-L records in use (6 with the layer treatment only, 14 with boundary smoothing)"""
        n = C.c_int32(0)
        self._check(self._lib.smgpu_halo_l_doubles(self._h, C.byref(n)))
        return n.value

    def set_layers(self, lp: LayerParams, minEdgeLength: float):
        """Enable the boundary layer treatment on lp.layerPatches (serial runs); returns the reference's
        doLayerTreatment.  Call after construction, before iterating."""
        d, keep = self._layer_desc(lp, minEdgeLength)
        on = C.c_int32(0)
        self._check(self._lib.smgpu_set_layers(self._h, C.byref(d), C.byref(on)))
        return bool(on.value)

    def _boundary_desc(self, bp: "BoundaryParams", minEdgeLength: float, layerEdgeLength=None, meshMinEdgeLength=None):
        REL_TOL = 1e-4                                                     # COM.H:20
        lel = minEdgeLength if layerEdgeLength is None else layerEdgeLength
        mn = self.mesh_stats()[0] if meshMinEdgeLength is None else meshMinEdgeLength
        tol = REL_TOL * min(mn, lel)                                       # SM.C:1921
        start, size, kind, sel = patch_arrays(self.mesh, bp.smoothingPatches)
        def pe(m, w):
            if m is None:
                return np.zeros((0, 3), np.float64), np.zeros((0, w), np.int32)
            return np.ascontiguousarray(m[0], np.float64).reshape(-1, 3), np.ascontiguousarray(m[1], np.int32).reshape(-1, w)
        ip, ie = pe(bp.initEdges, 2); tp, te = pe(bp.targetEdges, 2); sp, st = pe(bp.targetSurfaces, 3)
        cio = None if bp.isCornerPointIO is None else np.ascontiguousarray(bp.isCornerPointIO, np.int32)
        fio = None if bp.isFeatureEdgePointIO is None else np.ascontiguousarray(bp.isFeatureEdgePointIO, np.int32)
        d = _ffi.BoundaryDesc()
        d.nPatches = len(start)
        d.patchStart, d.patchSize = _p(start, _ffi.c_i32p), _p(size, _ffi.c_i32p)
        d.patchKind, d.isSmoothingPatch = _p(kind, _ffi.c_u8p), _p(sel, _ffi.c_u8p)
        d.nInitEdgePoints, d.initEdgePoints, d.nInitEdges, d.initEdges = len(ip), _p(ip, _ffi.c_f64p), len(ie), _p(ie, _ffi.c_i32p)
        d.nTargetEdgePoints, d.targetEdgePoints, d.nTargetEdges, d.targetEdges = len(tp), _p(tp, _ffi.c_f64p), len(te), _p(te, _ffi.c_i32p)
        d.nSurfacePoints, d.surfacePoints, d.nSurfaceTriangles, d.surfaceTriangles = len(sp), _p(sp, _ffi.c_f64p), len(st), _p(st, _ffi.c_i32p)
        d.isCornerPointIO = None if cio is None else _p(cio, _ffi.c_i32p)
        d.isFeatureEdgePointIO = None if fio is None else _p(fio, _ffi.c_i32p)
        d.distanceTolerance = tol
        d.internalSmoothingBlendingFraction = bp.internalSmoothingBlendingFraction
        return d, (start, size, kind, sel, ip, ie, tp, te, sp, st, cio, fio)

    def set_boundary_smoothing(self, bp: "BoundaryParams", minEdgeLength: float, layerEdgeLength=None):
        """Enable the boundary point smoothing (serial runs; after set_layers when both are used).  minEdgeLength is
        the -minEdgeLength option value (the default of layerEdgeLength, SM.C:1895).  Returns a dict with the
        reference's doBoundarySmoothing ("enabled") and the classification summary (BPS.C:423-438)."""
        d, keep = self._boundary_desc(bp, minEdgeLength, layerEdgeLength)
        info = _ffi.BoundaryInfo()
        self._check(self._lib.smgpu_set_boundary_smoothing(self._h, C.byref(d), C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ffi.BoundaryInfo._fields_}

    # step-wise set-up for runs with a halo (see include/smgpu.h, smgpu_boundary_begin)
    BOUNDARY_HOPS_SWEEP, BOUNDARY_TABLES, BOUNDARY_NORMALS_ACCUMULATE, BOUNDARY_NORMALS_FINISH = range(4)
    BOUNDARY_F_HOPS, BOUNDARY_F_NORMALS_COUNT = range(2)
    _BOUNDARY_FIELD_WIDTH = (1, 4)

    def boundary_stats(self):
        """(minimum edge length, bounding box [min x, max x, min y, max y, min z, max z]) of this rank (SM.C:1478-1526)"""
        mn, bb = C.c_double(0), np.zeros(6, np.float64)
        self._check(self._lib.smgpu_boundary_stats(self._h, C.byref(mn), _p(bb, _ffi.c_f64p)))
        return mn.value, bb

    def boundary_begin(self, bp, minEdgeLength, minEdgeGlobal, perimeterGlobal, layerEdgeLength=None):
        d, keep = self._boundary_desc(bp, minEdgeLength, layerEdgeLength, meshMinEdgeLength=minEdgeGlobal)
        info = _ffi.BoundaryInfo()
        self._check(self._lib.smgpu_boundary_begin(self._h, C.byref(d), float(minEdgeGlobal), float(perimeterGlobal), C.byref(info)))
        return {k: getattr(info, k) for k, _ in _ffi.BoundaryInfo._fields_}

    def boundary_step(self, step):
        self._check(self._lib.smgpu_boundary_step(self._h, int(step)))

    def boundary_shared_get(self, field):
        v = np.zeros((self._nShared, self._BOUNDARY_FIELD_WIDTH[field]), np.float64)
        if self._nShared:
            self._check(self._lib.smgpu_boundary_shared(self._h, int(field), 0, _p(v, _ffi.c_f64p)))
        return v

    def boundary_shared_set(self, field, values):
        v = np.ascontiguousarray(values, np.float64).reshape(self._nShared, self._BOUNDARY_FIELD_WIDTH[field])
        if self._nShared:
            self._check(self._lib.smgpu_boundary_shared(self._h, int(field), 1, _p(v, _ffi.c_f64p)))

    def boundary_classification(self):
        """(isCornerPoint, isFeatureEdgePoint) as the labelIOLists the reference writes (SM.C:2039-2064)."""
        a, b = np.zeros(self.nPoints, np.int32), np.zeros(self.nPoints, np.int32)
        self._check(self._lib.smgpu_get_boundary_classification(self._h, _p(a, _ffi.c_i32p), _p(b, _ffi.c_i32p)))
        return a, b

    def debug_find_line(self, starts, ends):
        """nearest intersections of the segments with the target surface: (hit mask, hit points)"""
        seg = np.ascontiguousarray(np.concatenate([np.asarray(starts, np.float64).reshape(-1, 3),
                                                   np.asarray(ends, np.float64).reshape(-1, 3)], axis=1))
        n = len(seg)
        out, hit = np.zeros((n, 3), np.float64), np.zeros(n, np.int32)
        self._check(self._lib.smgpu_debug_find_line(self._h, n, _p(seg, _ffi.c_f64p), _p(out, _ffi.c_f64p), _p(hit, _ffi.c_i32p)))
        return hit.astype(bool), out

    def iterate(self, centroidalIters: int, relTol: float = 0.02):
        """Returns (nDone, residuals[nDone], nFrozenPoints[nDone]) -- the values of the reference's
        per-iteration log line (SM.C:2396)."""
        stats = (_ffi.IterStats * max(centroidalIters, 1))()
        nDone = C.c_int32()
        self._check(self._lib.smgpu_iterate(self._h, centroidalIters, relTol, stats, C.byref(nDone)))
        n = nDone.value
        res = np.array([stats[i].residual for i in range(n)], dtype=np.float64)
        frz = np.array([stats[i].nFrozenPoints for i in range(n)], dtype=np.int64)
        self.last_near_ties = np.array([stats[i].nNearTies for i in range(n)], dtype=np.int64)     # per iteration of this call
        return n, res, frz

    def near_ties(self):
        """Near-tie census since the engine was created (include/smgpu.h, smgpu_get_near_ties): {"total", "edge_angle" (SM.C:923),
        "good_range" (SM.C:1367), "walk" (SM.C:1391-1394 / 1421-1424)} -- angle comparisons whose two sides were 1 .. 4 ulp apart,
        i.e. decisions the reference's acos could have taken the other way.  All zero in a normal run."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.smgpu_get_near_ties(self._h, out))
        return {"total": int(out[0]), "edge_angle": int(out[1]), "good_range": int(out[2]), "walk": int(out[3])}

    def check_error(self):
        """wait for the engine's stream and raise SmgpuError for any error word a kernel has raised (include/smgpu.h)"""
        self._check(self._lib.smgpu_check_error(self._h))

    def get_points(self):
        out = np.empty((self.nPoints, 3), np.float64)
        self._check(self._lib.smgpu_get_points(self._h, _p(out, _ffi.c_f64p)))
        return out

    def set_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        assert pts.shape == (self.nPoints, 3)
        self._check(self._lib.smgpu_set_points(self._h, _p(pts, _ffi.c_f64p)))

    # -- mesh quality --------------------------------------------------------------------------
    def mesh_quality(self, nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0) -> MeshQuality:
        """Quality report of the current points, computed on the device (include/smgpu.h, smgpu_mesh_quality).  Does not change
        the points or the state of the loop; refused on an engine with a halo."""
        p = _ffi.QualityParams(nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold)
        q = _ffi.Quality()
        self._check(self._lib.smgpu_mesh_quality(self._h, C.byref(p), C.byref(q)))
        return MeshQuality(**{n: getattr(q, n) for n, _ in q._fields_})

    def set_quality_trace(self, interval, nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0):
        """Quality history of the run (include/smgpu.h, smgpu_set_quality_trace): interval > 0 makes iterate() leave one
        QualityTraceRecord after every interval-th iteration that runs, counted across calls from this call on, with no
        synchronisation added to the loop; 0 switches the trace off.  Discards unread records.  Refused on an engine with a halo."""
        p = _ffi.QualityParams(nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold)
        self._check(self._lib.smgpu_set_quality_trace(self._h, int(interval), C.byref(p)))

    def quality_trace(self) -> list:
        """The pending records of the quality history, in ascending iteration; clears them."""
        return self._drain(self._lib.smgpu_get_quality_trace, _ffi.QualityTraceRecord, QualityTraceRecord)

    def set_quality_guard(self, criteria=("nonPositiveVolume", "wrongOriented"), refine=True):
        """Guard on the quality history (include/smgpu.h, smgpu_set_quality_guard); needs set_quality_trace first.  The points now
        become the baseline and snapshot 0.  A traced iteration whose count of a criterion (names of QUALITY_GUARD_CRITERIA)
        exceeds the baseline's stops the loop on the device; the iterate() call that meets it returns the iterations that ran,
        the tripping one included, and leaves the engine at the last good state: the last traced iteration that passed, or with
        `refine` the exact last iteration that passes.  The guard then disarms itself.  criteria=None disarms.  Refused on an
        engine with a halo, and with boundary point smoothing unless set_boundary_revert() opted in."""
        if criteria is None:
            self._check(self._lib.smgpu_set_quality_guard(self._h, None, 0))
            return
        if isinstance(criteria, str):
            criteria = (criteria,)
        bits = 0
        for c in criteria:
            if c not in QUALITY_GUARD_CRITERIA:
                raise ValueError(f"unknown quality guard criterion {c!r}: one of {', '.join(QUALITY_GUARD_CRITERIA)}")
            bits |= QUALITY_GUARD_CRITERIA[c]
        p = _ffi.QualityGuardParams(bits, 1 if refine else 0)
        self._check(self._lib.smgpu_set_quality_guard(self._h, C.byref(p), 1))

    def quality_guard(self) -> QualityGuardState:
        """The guard's state; it keeps answering after the guard has tripped and disarmed itself."""
        s = _ffi.QualityGuardState()
        self._check(self._lib.smgpu_get_quality_guard(self._h, C.byref(s)))
        rec = lambda r: QualityTraceRecord(**{f: getattr(r, f) for f, _ in r._fields_})  # noqa: E731
        return QualityGuardState(armed=bool(s.armed), tripped=bool(s.tripped),
                                 reasons=tuple(n for n, b in QUALITY_GUARD_CRITERIA.items() if s.reasons & b),
                                 snapshotIteration=s.snapshotIteration, trippedIteration=s.trippedIteration,
                                 restoredIteration=s.restoredIteration, baseline=rec(s.baseline),
                                 tripRecord=rec(s.tripRecord) if s.tripped else None)

    def quality_guard_restore(self):
        """Roll the engine back to the guard's snapshot (snapshotIteration) on request, for callers who judge the trace by criteria
        of their own: no refining, the guard stays armed, the trace's running number becomes snapshotIteration."""
        self._check(self._lib.smgpu_quality_guard_restore(self._h))

    def set_boundary_revert(self, on=True):
        """The opt-in under which the serial tangle constraint, the serial quality constraint (every limit) and the quality guard
        accept an engine with boundary point smoothing (include/smgpu.h, smgpu_set_boundary_revert; DESIGN.md "Mesh quality",
        10.21): a boundary point marked by a bad cell goes back like any other, off the place its projection gave it; the point
        normals are the loop's and are never reverted; the guard's snapshot carries them.  Launches and allocates nothing.
        Refused on an engine with a halo, and off while a constraint or the guard is on over boundary point smoothing."""
        self._check(self._lib.smgpu_set_boundary_revert(self._h, 1 if on else 0))

    def boundary_revert(self) -> bool:
        on = C.c_int32(0)
        self._check(self._lib.smgpu_get_boundary_revert(self._h, C.byref(on)))
        return bool(on.value)

    def set_tangle_constraint(self, passes=2):
        """Tangle constraint (include/smgpu.h, smgpu_set_tangle_constraint): from now on iterate() puts the points of every cell
        that an iteration turned bad -- non-positive volume or a wrongly oriented face, by the report's measure -- back where the
        iteration found them, in up to `passes` marked passes and then a full revert of the iteration.  Cells bad at the current
        points are exempt.  Adds no synchronisation to the loop.  Refused on an engine with a halo, and with boundary point smoothing
        unless set_boundary_revert() opted in."""
        p = _ffi.TangleParams(int(passes))
        self._check(self._lib.smgpu_set_tangle_constraint(self._h, C.byref(p), 1))

    def clear_tangle_constraint(self):
        """Switch the tangle constraint (either form) off; discards unread records."""
        self._check(self._lib.smgpu_set_tangle_constraint(self._h, None, 0))

    def set_tangle_constraint_coupled(self, sendT, recvT, passes=2):
        """The tangle constraint on an engine with a halo (include/smgpu.h, smgpu_set_tangle_constraint_coupled; DESIGN.md "Mesh
        quality", 10.13).  sendT / recvT: raw device addresses (ints) of nSend / nRecv int32 the caller owns and moves like
        exchange F.  The passes are the caller's: tangle_pass_begin / tangle_pass_end behind every iter_end."""
        p = _ffi.TangleParams(int(passes))
        d = _ffi.TangleHaloDesc(sendT, recvT)
        self._check(self._lib.smgpu_set_tangle_constraint_coupled(self._h, C.byref(p), C.byref(d), 1))

    def tangle_pass_begin(self) -> int:
        """evaluates the points, packs the shared points' marks into sendT; this rank's bad cells that are not exempt"""
        n = C.c_int64(0)
        self._check(self._lib.smgpu_tangle_pass_begin(self._h, C.byref(n)))
        return n.value

    def tangle_pass_end(self, nBadGlobal) -> bool:
        """the pass's revert under the verdict on the all-rank count; True: the iteration's passes are over"""
        done = C.c_int32(0)
        self._check(self._lib.smgpu_tangle_pass_end(self._h, int(nBadGlobal), C.byref(done)))
        return bool(done.value)

    def tangle_records(self) -> list:
        """The pending records of the tangle constraint, one per iteration that ran, in ascending iteration; clears them."""
        return self._drain(self._lib.smgpu_get_tangle_records, _ffi.TangleRecord, TangleRecord)

    def tangle_state(self) -> TangleState:
        return self._read_state(self._lib.smgpu_get_tangle_state, _ffi.TangleState, TangleState)

    def set_quality_constraint(self, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2, minTetQuality=None,
                               minTwist=None, minTriangleTwist=None, minFaceWeight=None, minVolRatio=None, minDeterminant=None,
                               maxConcave=None, minFlatness=None, minVol=None, minArea=None, scalePasses=0, errorReduction=0.75, nSmoothScale=4):
        """Quality constraint (include/smgpu.h, smgpu_set_quality_constraint; DESIGN.md "Mesh quality", 10.14): the tangle
        constraint with limits on face non-orthogonality (degrees; >= 180: off) and on the skewness of internal and of boundary
        faces (<= 0: off).  From now on iterate() puts the points of every cell that an iteration turned bad -- by the tangle
        constraint's measure, or as the owner or neighbour of a face over a limit -- back where the iteration found them, in up to
        `passes` marked passes and then a full revert.  Cells and faces bad at the current points are exempt.  Adds no
        synchronisation to the loop.  Refused on an engine with a halo, with boundary point smoothing (unless set_boundary_revert()
        opted in), or with the tangle constraint on.
        The six further limits (smgpu_set_quality_constraint_limits; None: off) make a face bad whose face-centre
        tet quality, twist, triangle twist, interpolation weight or volume ratio lies under them, and a cell whose determinant
        does, by the measures of mesh_quality_motion / mesh_quality_geometry; with all six None the call is what it was.
        The last four (smgpu_set_quality_constraint_limits_all; None: off) make a face bad that has a concave
        corner sharper than maxConcave degrees (mesh_quality_geometry's faceConcavity with concaveThreshold = maxConcave), whose
        flatness lies under minFlatness or whose area under minArea, and a cell whose volume lies under minVol; with all four
        None the call goes through the entry it went through before.
        scalePasses > 0 then switches the scaling passes on: set_quality_constraint_scaling with the three
        keywords; if that is refused the constraint is left off.  With scalePasses = 0 the call is what it was."""
        self._enable_quality_constraint(maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes,
                                        dict(minTetQuality=minTetQuality, minTwist=minTwist, minTriangleTwist=minTriangleTwist, minFaceWeight=minFaceWeight,
                                             minVolRatio=minVolRatio, minDeterminant=minDeterminant, maxConcave=maxConcave, minFlatness=minFlatness, minVol=minVol,
                                             minArea=minArea))
        if scalePasses != 0:
            try:
                self.set_quality_constraint_scaling(scalePasses, errorReduction, nSmoothScale)
            except SmgpuError:
                self.clear_quality_constraint()
                raise

    def set_quality_constraint_scaling(self, scalePasses=0, errorReduction=0.75, nSmoothScale=4):
        """The scaling passes of the serial quality constraint (include/smgpu.h, smgpu_set_quality_constraint_scaling; DESIGN.md
        "Mesh quality", 10.19), valid while it is on: in the first `scalePasses` marked passes of an iteration the points of a bad
        cell keep `errorReduction` times their scale of the move instead of going back; `nSmoothScale` Jacobi sweeps smooth the
        scale field behind every marked pass; the constraint's `passes` reverting passes and the full revert follow.
        scalePasses = 0 switches the scaling off and frees its memory, and so does clearing or re-enabling the constraint."""
        p = _ffi.QualityConstraintScaling(int(scalePasses), int(nSmoothScale), float(errorReduction))
        self._check(self._lib.smgpu_set_quality_constraint_scaling(self._h, C.byref(p)))

    def _enable_quality_constraint(self, maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes, limits, least=0, coupled=None):
        """through the entry of include/smgpu.h the limits take (quality_constraint_request); coupled: the arguments of
        _coupled_desc, for the coupled entry of the same tier"""
        p, tier = quality_constraint_request(maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes, limits, least)
        name = _QC_ENTRIES[tier][0]
        if coupled is None:
            self._check(getattr(self._lib, name)(self._h, C.byref(p), 1))
        else:
            d = self._coupled_desc(tier > 0, *coupled)
            self._check(getattr(self._lib, name + "_coupled")(self._h, C.byref(p), C.byref(d), 1))

    def clear_quality_constraint(self):
        """Switch the quality constraint (either form) off; discards unread records."""
        self._check(self._lib.smgpu_set_quality_constraint(self._h, None, 0))

    def set_quality_constraint_coupled(self, coupling, sendT, recvT, sendCc, recvCc, maxNonOrtho=65.0, maxInternalSkewness=4.0,
                                       maxBoundarySkewness=20.0, passes=2):
        """The quality constraint on an engine with a halo (include/smgpu.h, smgpu_set_quality_constraint_coupled; DESIGN.md "Mesh
        quality", 10.15).  coupling: quality_coupling()'s; sendT / recvT: raw device addresses (ints) of nSend / nRecv int32,
        sendCc / recvCc: of 3 doubles per processor face, all the caller's.  Returns with sendCc packed at the current points: the
        caller moves it to the neighbours' recvCc and calls quality_constraint_coupled_exempt.  The passes are the caller's too:
        quality_constraint_pass_begin / _pass_faces / _pass_end behind every iter_end."""
        self._enable_quality_constraint(maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes, {}, coupled=(coupling, sendT, recvT, sendCc, recvCc))

    def set_quality_constraint_limits_coupled(self, coupling, sendT, recvT, sendCc, recvCc, sendVc=0, recvVc=0, maxNonOrtho=65.0,
                                              maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2, minTetQuality=None, minTwist=None,
                                              minTriangleTwist=None, minFaceWeight=None, minVolRatio=None, minDeterminant=None, maxConcave=None,
                                              minFlatness=None, minVol=None, minArea=None):
        """set_quality_constraint_coupled with the six further limits (include/smgpu.h, smgpu_set_quality_constraint_limits_coupled;
        DESIGN.md "Mesh quality", 10.17; None: off).  sendVc / recvVc: raw device addresses of one double per processor face, needed
        while minVolRatio is on: the call returns with sendVc packed next to sendCc, the caller moves both, and so behind every
        quality_constraint_pass_begin."""
        # (with the last four all None the entry of 10.17, as before)
        self._enable_quality_constraint(maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes,
                                        dict(minTetQuality=minTetQuality, minTwist=minTwist, minTriangleTwist=minTriangleTwist, minFaceWeight=minFaceWeight,
                                             minVolRatio=minVolRatio, minDeterminant=minDeterminant, maxConcave=maxConcave, minFlatness=minFlatness, minVol=minVol,
                                             minArea=minArea), least=1, coupled=(coupling, sendT, recvT, sendCc, recvCc, sendVc, recvVc))

    def quality_constraint_coupled_exempt(self):
        """the face verdicts of the enabling evaluation, with the neighbours' cell centres in recvCc, become the exempt faces"""
        self._check(self._lib.smgpu_quality_constraint_coupled_exempt(self._h))

    def quality_constraint_pass_begin(self):
        """evaluates the geometry of the points and packs the owner cell centres of the processor faces into sendCc"""
        self._check(self._lib.smgpu_quality_constraint_pass_begin(self._h))

    def quality_constraint_pass_faces(self) -> int:
        """the face verdicts with recvCc, the cells, the marks, the pack of sendT; this rank's bad cells"""
        n = C.c_int64(0)
        self._check(self._lib.smgpu_quality_constraint_pass_faces(self._h, C.byref(n)))
        return n.value

    def quality_constraint_pass_end(self, nBadGlobal) -> bool:
        """the pass's revert under the verdict on the all-rank count; True: the iteration's passes are over"""
        done = C.c_int32(0)
        self._check(self._lib.smgpu_quality_constraint_pass_end(self._h, int(nBadGlobal), C.byref(done)))
        return bool(done.value)

    def set_quality_constraint_scaling_coupled(self, rowOffsets, rowPoints, sharedDeg, sendS, recvS, scalePasses=0, errorReduction=0.75, nSmoothScale=4):
        """The scaling passes of the coupled quality constraint (include/smgpu.h, smgpu_set_quality_constraint_scaling_coupled;
        DESIGN.md "Mesh quality", 10.20), valid while it is on.  rowOffsets / rowPoints: the counted neighbours of every shared
        point (CSR in the halo's order, local ids, row order), sharedDeg: its degree in the whole mesh (halo.scale_tables builds
        them); sendS / recvS: raw device addresses (ints) of nSend / nRecv doubles the caller owns and moves like sendT / recvT.
        scalePasses = 0 switches the scaling off and frees its memory (the tables and buffers are then not read and may be None / 0).  The passes
        are the caller's: quality_constraint_pass_scale and _pass_sweep between the move of T and quality_constraint_pass_end."""
        p = _ffi.QualityConstraintScaling(int(scalePasses), int(nSmoothScale), float(errorReduction))
        if rowOffsets is None:                # (scalePasses = 0: nothing else is read)
            self._check(self._lib.smgpu_set_quality_constraint_scaling_coupled(self._h, C.byref(p), None))
            return
        off, pts, deg = (np.ascontiguousarray(a, dtype=np.int32) for a in (rowOffsets, rowPoints, sharedDeg))
        c = _ffi.QualityScaleCoupling(_p(off, _ffi.c_i32p), _p(pts, _ffi.c_i32p), _p(deg, _ffi.c_i32p), sendS or None, recvS or None)
        self._check(self._lib.smgpu_set_quality_constraint_scaling_coupled(self._h, C.byref(p), C.byref(c)))

    def quality_constraint_pass_scale(self, nBadGlobal):
        """behind the move of T in a pass with bad cells, scaling on: the marks become scales, sweep 0's local half; sendS is packed"""
        self._check(self._lib.smgpu_quality_constraint_pass_scale(self._h, int(nBadGlobal)))

    def quality_constraint_pass_sweep(self):
        """behind the move of S: finishes the sweep in hand on the shared points and queues the next one's local half"""
        self._check(self._lib.smgpu_quality_constraint_pass_sweep(self._h))

    def quality_constraint_records(self) -> list:
        """The pending records of the quality constraint (QualityConstraintRecordAll), one per iteration that ran, in ascending
        iteration; clears them."""
        return self._drain(self._lib.smgpu_get_quality_constraint_records_all, _ffi.QualityConstraintRecordAll, QualityConstraintRecordAll)

    def quality_constraint_records_scaled(self) -> list:
        """quality_constraint_records() with the three fields of DESIGN.md 10.19 (QualityConstraintRecordScaled); the two getters
        drain the same pending list."""
        return self._drain(self._lib.smgpu_get_quality_constraint_records_scaled, _ffi.QualityConstraintRecordScaled, QualityConstraintRecordScaled)

    def quality_constraint_state_scaled(self) -> QualityConstraintStateScaled:
        return self._read_state(self._lib.smgpu_get_quality_constraint_state_scaled, _ffi.QualityConstraintStateScaled, QualityConstraintStateScaled)

    def quality_constraint_state(self) -> QualityConstraintStateAll:
        return self._read_state(self._lib.smgpu_get_quality_constraint_state_all, _ffi.QualityConstraintStateAll, QualityConstraintStateAll)

    def quality_field(self, name) -> np.ndarray:
        """Per-element quality field in polyMesh order: one of QUALITY_FIELDS (non-orthogonality in degrees, 0 on boundary faces)."""
        n = C.c_int64()
        self._check(self._lib.smgpu_quality_field(self._h, name.encode(), None, C.byref(n)))
        out = np.empty(n.value, np.float64)
        self._check(self._lib.smgpu_quality_field(self._h, name.encode(), _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    def _sets(self, call, *args, table=QUALITY_SETS):
        # one call when the sets hold at most nFaces + nCells ids (an element in several sets may exceed that: then again with
        # the exact size, which the refused call has reported)
        counts = (C.c_int64 * len(table))()
        ids = np.empty(max(1, self.mesh.nFaces + self.mesh.nCells), np.int32)
        if call(self._h, *args, counts, _p(ids, _ffi.c_i32p), len(ids)):
            if sum(counts) <= len(ids):
                self._check(1)
            ids = np.empty(sum(counts), np.int32)
            self._check(call(self._h, *args, counts, _p(ids, _ffi.c_i32p), len(ids)))
        out, at = {}, 0
        for (name, *_), n in zip(table, counts):
            out[name] = ids[at:at + n].copy()
            at += n
        return out

    def quality_sets(self, nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0) -> dict:
        """The failing elements of mesh_quality's report as sets (include/smgpu.h, smgpu_quality_sets): {name: ascending int32
        ids} for every name of QUALITY_SETS, empty ones included; each size equals the report's count.  Refused on an engine
        with a halo; leaves the points and the loop as they were."""
        p = _ffi.QualityParams(nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold)
        return self._sets(self._lib.smgpu_quality_sets, C.byref(p))

    def mesh_quality_geometry(self, concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05, volRatioThreshold=0.01,
                              determinantThreshold=0.001) -> MeshQualityGeometry:
        """The checks `checkMesh -allGeometry` adds, of the current points (include/smgpu.h, smgpu_mesh_quality_geometry): face
        concavity, flatness, interpolation weight, volume ratio, cell determinant.  Side effects and refusals as mesh_quality."""
        p = _ffi.QualityGeometryParams(concaveThreshold, flatnessThreshold, weightThreshold, volRatioThreshold, determinantThreshold)
        q = _ffi.QualityGeometry()
        self._check(self._lib.smgpu_mesh_quality_geometry(self._h, C.byref(p), C.byref(q)))
        return MeshQualityGeometry(**{n: getattr(q, n) for n, _ in q._fields_})

    def quality_geometry_field(self, name) -> np.ndarray:
        """Per-element field of the geometry checks in polyMesh order: one of QUALITY_GEOMETRY_FIELDS (faceConcavity is the sine of
        the worst concave corner under the default threshold; weight and volume ratio are 1 on boundary faces)."""
        n = C.c_int64(0)
        self._check(self._lib.smgpu_quality_geometry_field(self._h, name.encode(), None, C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        self._check(self._lib.smgpu_quality_geometry_field(self._h, name.encode(), _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    def mesh_quality_motion(self, tetThreshold=1e-15, twistThreshold=0.02, triangleTwistThreshold=-1.0) -> MeshQualityMotion:
        """The motion criteria of the current points (include/smgpu.h, smgpu_mesh_quality_motion): face-centre and base-point tet
        quality, face twist, triangle twist, under the default meshQualityDict thresholds.  Side effects and refusals as mesh_quality."""
        p = _ffi.QualityMotionParams(tetThreshold, twistThreshold, triangleTwistThreshold)
        q = _ffi.QualityMotion()
        self._check(self._lib.smgpu_mesh_quality_motion(self._h, C.byref(p), C.byref(q)))
        return MeshQualityMotion(**{n: getattr(q, n) for n, _ in q._fields_})

    def quality_motion_field(self, name) -> np.ndarray:
        """Per-face field of the motion criteria in polyMesh order: one of QUALITY_MOTION_FIELDS (twist and triangle twist are 1 on
        triangles)."""
        n = C.c_int64(0)
        self._check(self._lib.smgpu_quality_motion_field(self._h, name.encode(), None, C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        self._check(self._lib.smgpu_quality_motion_field(self._h, name.encode(), _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    def quality_geometry_sets(self, concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05, volRatioThreshold=0.01,
                              determinantThreshold=0.001) -> dict:
        """The findings of mesh_quality_geometry's report as sets (include/smgpu.h, smgpu_quality_geometry_sets): {name: ascending
        int32 ids} for every name of QUALITY_GEOMETRY_SETS, empty ones included; each size equals the report's count under the same
        thresholds.  Refusals and side effects as mesh_quality_geometry."""
        p = _ffi.QualityGeometryParams(concaveThreshold, flatnessThreshold, weightThreshold, volRatioThreshold, determinantThreshold)
        return self._sets(self._lib.smgpu_quality_geometry_sets, C.byref(p), table=QUALITY_GEOMETRY_SETS)

    def quality_motion_sets(self, tetThreshold=1e-15, twistThreshold=0.02, triangleTwistThreshold=-1.0) -> dict:
        """The findings of mesh_quality_motion's report as sets (smgpu_quality_motion_sets): as quality_geometry_sets, the names of
        QUALITY_MOTION_SETS."""
        p = _ffi.QualityMotionParams(tetThreshold, twistThreshold, triangleTwistThreshold)
        return self._sets(self._lib.smgpu_quality_motion_sets, C.byref(p), table=QUALITY_MOTION_SETS)

    # -- mesh quality of a sub-domain (DESIGN.md "Mesh quality", 10.4; smoothmesh_amd/quality.py drives these) -------------
    def quality_coupling(self, rank=None):
        """(myRank, [(patchStart, patchSize, neighbRank)]) of this engine's processor patches in boundary-file order.  Refuses
        processorCyclic patches (their cell centres would need the patch transform)."""
        pats = []
        for p in self.mesh.patches:
            if p.type == "processorCyclic":
                raise SmgpuError(f"mesh quality: patch {p.name} is a processorCyclic patch: cyclic coupling between sub-domains is "
                                 "not supported")
            if p.type == "processor":
                if rank is None:
                    rank = int(p.myProcNo)
                pats.append((int(p.startFace), int(p.nFaces), int(p.neighbProcNo)))
        return (0 if rank is None else int(rank)), pats

    @staticmethod
    def _coupling(coupling):
        """quality_coupling()'s answer as smgpu_quality_coupling; the struct keeps the three arrays it points to alive"""
        rank, pats = coupling
        c = _ffi.QualityCoupling(int(rank), len(pats))
        c._keep = [np.array([p[i] for p in pats], np.int32) for i in range(3)]
        c.patchStart, c.patchSize, c.neighbRank = (_p(a, _ffi.c_i32p) for a in c._keep)
        return c

    def _coupled_desc(self, full, coupling, sendT, recvT, sendCc, recvCc, sendVc=0, recvVc=0):
        """the halo descriptor of a coupled quality constraint entry (full: with the volume buffers of 10.17); it keeps the
        coupling it points to alive"""
        c = self._coupling(coupling)
        bufs = [a or None for a in (sendT, recvT, sendCc, recvCc)]
        d = _ffi.QualityConstraintHaloDescFull(*bufs, C.pointer(c), sendVc or None, recvVc or None) if full else _ffi.QualityConstraintHaloDesc(*bufs, C.pointer(c))
        d._keep = c
        return d

    def quality_coupled_pack(self, coupling, sendCc) -> int:
        """smgpu_quality_coupled_pack: geometry of the current points, then the owner cell centre of every processor face (patch
        order) into the device buffer at address sendCc (3 doubles per face; 0 when there are none).  Returns the number of
        processor faces."""
        c = self._coupling(coupling)
        n = C.c_int64()
        self._check(self._lib.smgpu_quality_coupled_pack(self._h, C.byref(c), C.c_void_p(sendCc or None), C.byref(n)))
        return n.value

    def quality_coupled_report(self, recvCc, nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0) -> dict:
        """smgpu_quality_coupled_report: this rank's record (smgpu_quality_part field names, local ids), the neighbours' cell
        centres at device address recvCc"""
        p = _ffi.QualityParams(nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold)
        q = _ffi.QualityPart()
        self._check(self._lib.smgpu_quality_coupled_report(self._h, C.byref(p), C.c_void_p(recvCc or None), C.byref(q)))
        return {n: getattr(q, n) for n, _ in q._fields_}

    def quality_coupled_sets(self, recvCc, nonOrthThreshold=70.0, skewThreshold=4.0, closedThreshold=1e-6, aspectThreshold=1000.0) -> dict:
        """smgpu_quality_coupled_sets: as quality_sets for this rank, local ids; a processor face is a member only on the side
        that counts it"""
        p = _ffi.QualityParams(nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold)
        return self._sets(self._lib.smgpu_quality_coupled_sets, C.byref(p), C.c_void_p(recvCc or None))

    def quality_coupled_field(self, name, recvCc) -> np.ndarray:
        """smgpu_quality_coupled_field: as quality_field, processor faces with the internal-face definitions"""
        n = C.c_int64()
        self._check(self._lib.smgpu_quality_coupled_field(self._h, name.encode(), C.c_void_p(recvCc or None), None, C.byref(n)))
        out = np.empty(n.value, np.float64)
        self._check(self._lib.smgpu_quality_coupled_field(self._h, name.encode(), C.c_void_p(recvCc or None), _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    # -- the -allGeometry checks and the motion criteria of a sub-domain (DESIGN.md "Mesh quality", 10.8) --------------------
    def quality_coupled_pack_volumes(self, sendVc) -> int:
        """smgpu_quality_coupled_pack_volumes, after quality_coupled_pack on the same points: every cell's signed volume into the
        engine's scratch and the owner cell's volume of every processor face (the slot order of sendCc) into the device buffer at
        address sendVc (1 double per face; 0 when there are none).  Returns the number of processor faces."""
        n = C.c_int64()
        self._check(self._lib.smgpu_quality_coupled_pack_volumes(self._h, C.c_void_p(sendVc or None), C.byref(n)))
        return n.value

    def quality_coupled_geometry_report(self, recvCc, recvVc, concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05,
                                        volRatioThreshold=0.01, determinantThreshold=0.001) -> dict:
        """smgpu_quality_coupled_geometry_report: this rank's record (smgpu_quality_geometry_part field names, local ids), the
        neighbours' cell centres and volumes at the device addresses recvCc and recvVc"""
        p = _ffi.QualityGeometryParams(concaveThreshold, flatnessThreshold, weightThreshold, volRatioThreshold, determinantThreshold)
        q = _ffi.QualityGeometryPart()
        self._check(self._lib.smgpu_quality_coupled_geometry_report(self._h, C.byref(p), C.c_void_p(recvCc or None),
                                                                    C.c_void_p(recvVc or None), C.byref(q)))
        return {n: getattr(q, n) for n, _ in q._fields_}

    def quality_coupled_geometry_field(self, name, recvCc, recvVc) -> np.ndarray:
        """smgpu_quality_coupled_geometry_field: as quality_geometry_field, processor faces with the internal-face definitions"""
        n = C.c_int64()
        a = (self._h, name.encode(), C.c_void_p(recvCc or None), C.c_void_p(recvVc or None))
        self._check(self._lib.smgpu_quality_coupled_geometry_field(*a, None, C.byref(n)))
        out = np.empty(n.value, np.float64)
        self._check(self._lib.smgpu_quality_coupled_geometry_field(*a, _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    def quality_coupled_motion_report(self, recvCc, tetThreshold=1e-15, twistThreshold=0.02, triangleTwistThreshold=-1.0) -> dict:
        """smgpu_quality_coupled_motion_report: this rank's record (smgpu_quality_motion_part field names, local ids)"""
        p = _ffi.QualityMotionParams(tetThreshold, twistThreshold, triangleTwistThreshold)
        q = _ffi.QualityMotionPart()
        self._check(self._lib.smgpu_quality_coupled_motion_report(self._h, C.byref(p), C.c_void_p(recvCc or None), C.byref(q)))
        return {n: getattr(q, n) for n, _ in q._fields_}

    def quality_coupled_geometry_sets(self, recvCc, recvVc, concaveThreshold=10.0, flatnessThreshold=0.8, weightThreshold=0.05,
                                      volRatioThreshold=0.01, determinantThreshold=0.001) -> dict:
        """smgpu_quality_coupled_geometry_sets: as quality_geometry_sets for this rank, local ids; a processor face is a member only
        on the side that counts it"""
        p = _ffi.QualityGeometryParams(concaveThreshold, flatnessThreshold, weightThreshold, volRatioThreshold, determinantThreshold)
        return self._sets(self._lib.smgpu_quality_coupled_geometry_sets, C.byref(p), C.c_void_p(recvCc or None), C.c_void_p(recvVc or None),
                          table=QUALITY_GEOMETRY_SETS)

    def quality_coupled_motion_sets(self, recvCc, tetThreshold=1e-15, twistThreshold=0.02, triangleTwistThreshold=-1.0) -> dict:
        """smgpu_quality_coupled_motion_sets: as quality_motion_sets for this rank, local ids, members counted once"""
        p = _ffi.QualityMotionParams(tetThreshold, twistThreshold, triangleTwistThreshold)
        return self._sets(self._lib.smgpu_quality_coupled_motion_sets, C.byref(p), C.c_void_p(recvCc or None), table=QUALITY_MOTION_SETS)

    def quality_coupled_motion_field(self, name, recvCc) -> np.ndarray:
        """smgpu_quality_coupled_motion_field: as quality_motion_field, processor faces with the internal-face definitions"""
        n = C.c_int64()
        a = (self._h, name.encode(), C.c_void_p(recvCc or None))
        self._check(self._lib.smgpu_quality_coupled_motion_field(*a, None, C.byref(n)))
        out = np.empty(n.value, np.float64)
        self._check(self._lib.smgpu_quality_coupled_motion_field(*a, _p(out, _ffi.c_f64p), C.byref(n)))
        return out

    # -- timing --------------------------------------------------------------------------------
    def enable_timing(self, on=True):
        self._check(self._lib.smgpu_enable_timing(self._h, int(on)))

    def reset_counters(self):
        self._check(self._lib.smgpu_reset_counters(self._h))

    def counters(self):
        c = _ffi.Counters()
        self._check(self._lib.smgpu_get_counters(self._h, C.byref(c)))
        return [dict(name=c.name[i].decode(), ms=c.ms[i], launches=c.launches[i], algoBytesPerLaunch=c.algoBytesPerLaunch[i],
                     algoF64OpsPerLaunch=c.algoF64OpsPerLaunch[i])
                for i in range(c.nKernels)]

    # -- multi-rank ----------------------------------------------------------------------------
    def halo_configure(self, sharedLocal, sendShared, nRecv, combOffsets, combSlots, sendA, recvA, sendF, recvF, localStats,
                       exchangeStream=None, sendL=None, recvL=None):
        """Pointers are raw device addresses (ints); exchangeStream: raw hipStream_t (int, 0 = null stream) the
        caller enqueues its exchanges on, or None = the engine's own stream; see smgpu_halo_desc."""
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in (sharedLocal, sendShared, combOffsets, combSlots)]
        d = _ffi.HaloDesc()
        d.nShared = len(keep[0]); d.sharedLocal = _p(keep[0], _ffi.c_i32p)
        d.nSend = len(keep[1]); d.sendShared = _p(keep[1], _ffi.c_i32p)
        d.nRecv = int(nRecv); d.combOffsets = _p(keep[2], _ffi.c_i32p); d.combSlots = _p(keep[3], _ffi.c_i32p)
        d.sendA, d.recvA, d.sendF, d.recvF, d.localStats = sendA, recvA, sendF, recvF, localStats
        d.sendL, d.recvL = sendL, recvL
        self._nShared = len(keep[0])
        d.useExchangeStream = 0 if exchangeStream is None else 1
        d.exchangeStream = exchangeStream or None
        self._check(self._lib.smgpu_halo_configure(self._h, C.byref(d)))

    def set_push(self, peerCount, remoteBase, myIndexAtPeer, peerRecvA, peerRecvL, peerRecvF, peerFlags, localFlags):
        """peer-store transport (smgpu_halo_set_push): arrays per peer in ascending rank order; pointers = raw device addresses"""
        n = len(peerCount)
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in (peerCount, remoteBase, myIndexAtPeer)]
        arr = lambda v: (C.c_void_p * max(n, 1))(*[C.c_void_p(int(x) if x else None) for x in v])
        ptrs = [arr(v) for v in (peerRecvA, peerRecvL, peerRecvF, peerFlags)]
        d = _ffi.PushDesc()
        d.nPeers = n
        d.peerCount, d.remoteBase, d.myIndexAtPeer = (_p(k, _ffi.c_i32p) for k in keep)
        d.peerRecvA, d.peerRecvL, d.peerRecvF, d.peerFlags = (C.cast(a, C.POINTER(C.c_void_p)) for a in ptrs)
        d.localFlags = localFlags
        self._check(self._lib.smgpu_halo_set_push(self._h, C.byref(d)))

    def clear_push(self):
        self._check(self._lib.smgpu_halo_set_push(self._h, None))

    def set_exchange_stream(self, exchangeStream):
        """None = exchanges are enqueued on the engine's stream; int = raw hipStream_t they are enqueued on"""
        self._check(self._lib.smgpu_halo_set_exchange_stream(self._h, 0 if exchangeStream is None else 1, exchangeStream or None))

    def stream(self):
        """raw hipStream_t handle (int) of the engine's stream"""
        out = C.c_void_p()
        self._check(self._lib.smgpu_get_stream(self._h, C.byref(out)))
        return out.value or 0

    def set_stats_history(self, ptr, capacity):
        """device array of 2*capacity doubles that iter_end fills record by record (None switches it off)"""
        self._check(self._lib.smgpu_halo_set_stats_history(self._h, ptr, int(capacity)))

    def iter_begin(self):
        self._check(self._lib.smgpu_iter_begin(self._h))

    def iter_interior(self):
        self._check(self._lib.smgpu_iter_interior(self._h))

    def iter_mid(self):
        self._check(self._lib.smgpu_iter_mid(self._h))

    def iter_ahead(self):
        self._check(self._lib.smgpu_iter_ahead(self._h))

    def iter_end(self):
        self._check(self._lib.smgpu_iter_end(self._h))

    # -- debug / parity ------------------------------------------------------------------------
    def debug_walk_mode(self):
        """(replay form of the face-angle walk in use, number of automatic changes since set_params)"""
        mode, sw, cnt = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.smgpu_debug_walk_mode(self._h, C.byref(mode), C.byref(sw), C.byref(cnt)))
        self.last_active_count = cnt.value
        return mode.value, sw.value

    def debug_addressing_checksums(self):
        """checksums of the engine's addressing (built on the device where the mesh allows), TOPO_ARRAYS order"""
        out = (C.c_uint64 * 64)()
        self._check(self._lib.smgpu_debug_addressing_checksums(self._h, out))
        return [int(x) for x in out][:len(TOPO_ARRAYS)]

    def debug_tile_checksums(self):
        """checksums of the geometry tile tables as the kernels read them (include/smgpu.h smgpu_debug_tile_checksums)"""
        out = (C.c_uint64 * 64)()
        self._check(self._lib.smgpu_debug_tile_checksums(self._h, out))
        return [int(x) for x in out]

    def debug_halo_mode(self):
        """how the last multi-rank iteration went out: {"multi_role", "flagged", "fix_inside"} (include/smgpu.h)"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.smgpu_debug_halo_mode(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"multi_role": bool(a.value), "flagged": bool(b.value), "fix_inside": bool(c.value)}

    def debug_halo_tiles(self):
        """the tile counts the multi-role launches are split on: {"geom_shared", "geom_interior", "smooth_tiles", "shared_point_tiles"}
        (include/smgpu.h; all 0 on the direct-gather kernels)"""
        v = [C.c_int32() for _ in range(4)]
        self._check(self._lib.smgpu_debug_halo_tiles(self._h, *(C.byref(x) for x in v)))
        return dict(zip(("geom_shared", "geom_interior", "smooth_tiles", "shared_point_tiles"), (x.value for x in v)))

    def set_device_share(self, n_engines):
        """n_engines engines compute on this device at the same time: the persistent walk replay takes its share of the chip"""
        self._check(self._lib.smgpu_set_device_share(self._h, int(n_engines)))

    def debug_propose(self):
        self._check(self._lib.smgpu_debug_propose(self._h))

    def debug_field(self, name):
        n = C.c_int64()
        self._check(self._lib.smgpu_debug_get_field(self._h, name.encode(), None, C.byref(n)))
        out = np.empty(n.value, np.float64)
        self._check(self._lib.smgpu_debug_get_field(self._h, name.encode(), _p(out, _ffi.c_f64p), C.byref(n)))
        return out
