"""ctypes binding of include/smgpu.h (the drop-in boundary).  No torch types cross it."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMOOTHMESH_SMGPU_LIB", os.path.join(_HERE, "csrc", "libsmgpu.so"))   # override: experimental builds

c_i32p = C.POINTER(C.c_int32)
c_f64p = C.POINTER(C.c_double)
c_u8p = C.POINTER(C.c_uint8)


class MeshDesc(C.Structure):
    _fields_ = [
        ("nPoints", C.c_int32), ("nCells", C.c_int32), ("nFaces", C.c_int32), ("nInternalFaces", C.c_int32),
        ("points", c_f64p), ("faceOffsets", c_i32p), ("facePoints", c_i32p), ("owner", c_i32p),
        ("neighbour", c_i32p), ("isInternalPoint", c_u8p), ("isSmoothingSurfacePoint", c_u8p),
        ("device", C.c_int32), ("stream", C.c_void_p), ("useCallerStream", C.c_int32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("maxStepLength", C.c_double), ("relStepFrac", C.c_double), ("minEdgeLength", C.c_double),
        ("totalMinFreeze", C.c_int32), ("edgeAngleConstraint", C.c_int32), ("faceAngleConstraint", C.c_int32),
        ("minAngle", C.c_double), ("maxAngle", C.c_double),
    ]


class IterStats(C.Structure):
    _fields_ = [("residual", C.c_double), ("nFrozenPoints", C.c_int32), ("nNearTies", C.c_int32)]


class Sizes(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "nPoints", "nCells", "nFaces", "nInternalFaces", "nEdges", "nnzFacePoints", "nnzPointCells",
        "nnzPointPoints", "nnzPointFaces", "nnzEdgeFaces", "nnzEdgeCells", "nnzCellFaces", "deviceBytes")]


MAX_KERNELS = 24


class Counters(C.Structure):
    _fields_ = [
        ("nKernels", C.c_int32), ("name", C.c_char_p * MAX_KERNELS), ("ms", C.c_double * MAX_KERNELS),
        ("launches", C.c_int64 * MAX_KERNELS), ("algoBytesPerLaunch", C.c_int64 * MAX_KERNELS),
        ("algoF64OpsPerLaunch", C.c_int64 * MAX_KERNELS),
    ]


class HaloDesc(C.Structure):
    _fields_ = [
        ("nShared", C.c_int32), ("sharedLocal", c_i32p), ("nSend", C.c_int32), ("sendShared", c_i32p),
        ("nRecv", C.c_int32), ("combOffsets", c_i32p), ("combSlots", c_i32p),
        ("sendA", C.c_void_p), ("recvA", C.c_void_p), ("sendF", C.c_void_p), ("recvF", C.c_void_p),
        ("localStats", C.c_void_p), ("sendL", C.c_void_p), ("recvL", C.c_void_p),
        ("useExchangeStream", C.c_int32), ("exchangeStream", C.c_void_p),
    ]


class PushDesc(C.Structure):
    _fields_ = [
        ("nPeers", C.c_int32), ("peerCount", c_i32p), ("remoteBase", c_i32p), ("myIndexAtPeer", c_i32p),
        ("peerRecvA", C.POINTER(C.c_void_p)), ("peerRecvL", C.POINTER(C.c_void_p)), ("peerRecvF", C.POINTER(C.c_void_p)),
        ("peerFlags", C.POINTER(C.c_void_p)), ("localFlags", C.c_void_p),
    ]


class LayerDesc(C.Structure):
    _fields_ = [
        ("nPatches", C.c_int32), ("patchStart", c_i32p), ("patchSize", c_i32p), ("patchKind", c_u8p), ("isLayerPatch", c_u8p),
        ("layerMaxBlendingFraction", C.c_double), ("layerEdgeLength", C.c_double), ("layerExpansionRatio", C.c_double),
        ("minLayers", C.c_int32), ("maxLayers", C.c_int32),
    ]


class BoundaryDesc(C.Structure):
    _fields_ = [
        ("nPatches", C.c_int32), ("patchStart", c_i32p), ("patchSize", c_i32p), ("patchKind", c_u8p), ("isSmoothingPatch", c_u8p),
        ("nInitEdgePoints", C.c_int32), ("initEdgePoints", c_f64p), ("nInitEdges", C.c_int32), ("initEdges", c_i32p),
        ("nTargetEdgePoints", C.c_int32), ("targetEdgePoints", c_f64p), ("nTargetEdges", C.c_int32), ("targetEdges", c_i32p),
        ("nSurfacePoints", C.c_int32), ("surfacePoints", c_f64p), ("nSurfaceTriangles", C.c_int32), ("surfaceTriangles", c_i32p),
        ("isCornerPointIO", c_i32p), ("isFeatureEdgePointIO", c_i32p),
        ("distanceTolerance", C.c_double), ("internalSmoothingBlendingFraction", C.c_double),
    ]


class BoundaryInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("nCornerPoints", C.c_int32), ("nFeatureEdgePoints", C.c_int32),
                ("nSmoothingSurfacePoints", C.c_int32), ("nFrozenSurfacePoints", C.c_int32), ("nTargetEdgeStrings", C.c_int32)]


class QualityParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("nonOrthThreshold", "skewThreshold", "closedThreshold", "aspectThreshold")]


class Quality(C.Structure):
    _fields_ = [
        ("nCells", C.c_int64), ("nFaces", C.c_int64), ("nInternalFaces", C.c_int64),
        ("minVolume", C.c_double), ("maxVolume", C.c_double), ("totalVolume", C.c_double), ("nNonPositiveVolume", C.c_int64),
        ("minVolumeCell", C.c_int32),
        ("minFaceArea", C.c_double), ("maxFaceArea", C.c_double), ("nZeroAreaFaces", C.c_int64),
        ("maxNonOrth", C.c_double), ("avgNonOrth", C.c_double), ("nSevereNonOrth", C.c_int64), ("nErrorNonOrth", C.c_int64),
        ("maxNonOrthFace", C.c_int32),
        ("maxSkewness", C.c_double), ("nSkewFaces", C.c_int64), ("maxSkewFace", C.c_int32),
        ("nWrongOrientedFaces", C.c_int64),
        ("maxOpenness", C.c_double), ("nOpenCells", C.c_int64),
        ("maxAspectRatio", C.c_double), ("nHighAspectCells", C.c_int64),
    ]


class QualityTraceRecord(C.Structure):
    """smgpu_quality_trace_record: the running iteration number, then Quality without the sizes and the two fields that depend on
    the order of a floating-point sum"""
    _fields_ = [("iteration", C.c_int64)] + [(n, t) for n, t in Quality._fields_
                                             if n not in ("nCells", "nFaces", "nInternalFaces", "totalVolume", "avgNonOrth")]


class QualityGuardParams(C.Structure):
    _fields_ = [("criteria", C.c_uint32), ("refine", C.c_int32)]


class QualityGuardState(C.Structure):
    """smgpu_quality_guard_state"""
    _fields_ = [("armed", C.c_int32), ("tripped", C.c_int32), ("reasons", C.c_uint32),
                ("snapshotIteration", C.c_int64), ("trippedIteration", C.c_int64), ("restoredIteration", C.c_int64),
                ("baseline", QualityTraceRecord), ("tripRecord", QualityTraceRecord)]


class TangleParams(C.Structure):
    """smgpu_tangle_params"""
    _fields_ = [("passes", C.c_int32)]


class TangleRecord(C.Structure):
    """smgpu_tangle_record"""
    _fields_ = [("iteration", C.c_int64), ("passes", C.c_int32), ("fullRevert", C.c_int32), ("nBadCells", C.c_int64),
                ("nPointsReverted", C.c_int64)]


class TangleState(C.Structure):
    """smgpu_tangle_state"""
    _fields_ = [("on", C.c_int32), ("passes", C.c_int32), ("nExemptCells", C.c_int64), ("iteration", C.c_int64)]


class QualityConstraintParams(C.Structure):
    """smgpu_quality_constraint_params"""
    _fields_ = [("maxNonOrtho", C.c_double), ("maxInternalSkewness", C.c_double), ("maxBoundarySkewness", C.c_double), ("passes", C.c_int32)]


class QualityConstraintRecord(C.Structure):
    """smgpu_quality_constraint_record"""
    _fields_ = [("iteration", C.c_int64), ("passes", C.c_int32), ("fullRevert", C.c_int32), ("nBadCells", C.c_int64),
                ("nPointsReverted", C.c_int64), ("nTangledCells", C.c_int64), ("nNonOrthoFaces", C.c_int64), ("nSkewFaces", C.c_int64)]


class QualityConstraintState(C.Structure):
    """smgpu_quality_constraint_state"""
    _fields_ = [("on", C.c_int32), ("passes", C.c_int32), ("maxNonOrtho", C.c_double), ("maxInternalSkewness", C.c_double),
                ("maxBoundarySkewness", C.c_double), ("nExemptCells", C.c_int64), ("nExemptFaces", C.c_int64), ("iteration", C.c_int64)]


_QC_LIMITS = ("minTetQuality", "minTwist", "minTriangleTwist", "minFaceWeight", "minVolRatio", "minDeterminant")


class QualityConstraintLimits(C.Structure):
    """smgpu_quality_constraint_limits: QualityConstraintParams' fields, then the six limits of DESIGN.md 10.16"""
    _fields_ = QualityConstraintParams._fields_ + [(n, C.c_double) for n in _QC_LIMITS]


class QualityConstraintRecordFull(C.Structure):
    """smgpu_quality_constraint_record_full: QualityConstraintRecord's fields, then the six counts of DESIGN.md 10.16"""
    _fields_ = QualityConstraintRecord._fields_ + [(n, C.c_int64) for n in ("nLowTetFaces", "nLowTwistFaces", "nLowTriangleTwistFaces", "nLowWeightFaces",
                                                                             "nLowVolRatioFaces", "nUnderdeterminedCells")]


class QualityConstraintStateFull(C.Structure):
    """smgpu_quality_constraint_state_full"""
    _fields_ = QualityConstraintState._fields_ + [(n, C.c_double) for n in _QC_LIMITS] + [("nExemptDeterminantCells", C.c_int64)]


_QC_LIMITS_ALL = ("maxConcave", "minFlatness", "minVol", "minArea")


class QualityConstraintLimitsAll(C.Structure):
    """smgpu_quality_constraint_limits_all: QualityConstraintLimits' fields, then the four limits of DESIGN.md 10.18"""
    _fields_ = QualityConstraintLimits._fields_ + [(n, C.c_double) for n in _QC_LIMITS_ALL]


class QualityConstraintRecordAll(C.Structure):
    """smgpu_quality_constraint_record_all: QualityConstraintRecordFull's fields, then the four counts of DESIGN.md 10.18"""
    _fields_ = QualityConstraintRecordFull._fields_ + [(n, C.c_int64) for n in ("nConcaveFaces", "nWarpedFaces", "nSmallAreaFaces", "nSmallVolumeCells")]


class QualityConstraintStateAll(C.Structure):
    """smgpu_quality_constraint_state_all"""
    _fields_ = QualityConstraintStateFull._fields_ + [(n, C.c_double) for n in _QC_LIMITS_ALL] + [("nExemptVolumeCells", C.c_int64)]


class QualityConstraintScaling(C.Structure):
    """smgpu_quality_constraint_scaling"""
    _fields_ = [("scalePasses", C.c_int32), ("nSmoothScale", C.c_int32), ("errorReduction", C.c_double)]


class QualityConstraintRecordScaled(C.Structure):
    """smgpu_quality_constraint_record_scaled: QualityConstraintRecordAll's fields, then the three of DESIGN.md 10.19"""
    _fields_ = QualityConstraintRecordAll._fields_ + [("nScalePasses", C.c_int64), ("nPointsScaled", C.c_int64), ("minScale", C.c_double)]


class QualityConstraintStateScaled(C.Structure):
    """smgpu_quality_constraint_state_scaled: QualityConstraintStateAll's fields, then the three parameters of DESIGN.md 10.19"""
    _fields_ = QualityConstraintStateAll._fields_ + QualityConstraintScaling._fields_


class QualityScaleCoupling(C.Structure):
    """smgpu_quality_scale_coupling: the counted rows and degrees of the shared points, the buffers of exchange S"""
    _fields_ = [("rowOffsets", c_i32p), ("rowPoints", c_i32p), ("sharedDeg", c_i32p), ("sendS", C.c_void_p), ("recvS", C.c_void_p)]


class TangleHaloDesc(C.Structure):
    """smgpu_tangle_halo_desc"""
    _fields_ = [("sendT", C.c_void_p), ("recvT", C.c_void_p)]


class QualityGeometryParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("concaveThreshold", "flatnessThreshold", "weightThreshold", "volRatioThreshold",
                                          "determinantThreshold")]


class QualityGeometry(C.Structure):
    _fields_ = [
        ("nConcaveFaces", C.c_int64), ("maxConcaveSin", C.c_double), ("maxConcaveAngle", C.c_double), ("maxConcaveFace", C.c_int32),
        ("minFlatness", C.c_double), ("avgFlatness", C.c_double), ("nFlatnessFaces", C.c_int64), ("nWarpedFaces", C.c_int64),
        ("minFlatnessFace", C.c_int32),
        ("minFaceWeight", C.c_double), ("avgFaceWeight", C.c_double), ("nLowWeightFaces", C.c_int64), ("minFaceWeightFace", C.c_int32),
        ("minVolRatio", C.c_double), ("avgVolRatio", C.c_double), ("nLowVolRatioFaces", C.c_int64), ("minVolRatioFace", C.c_int32),
        ("minDeterminant", C.c_double), ("avgDeterminant", C.c_double), ("nUnderdeterminedCells", C.c_int64),
        ("minDeterminantCell", C.c_int32),
    ]


class QualityMotionParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("tetThreshold", "twistThreshold", "triangleTwistThreshold")]


class QualityMotion(C.Structure):
    _fields_ = [
        ("minTetQuality", C.c_double), ("avgTetQuality", C.c_double), ("nLowTetFaces", C.c_int64), ("minTetFace", C.c_int32),
        ("minBaseTetQuality", C.c_double), ("nNoBasePointFaces", C.c_int64), ("minBaseTetFace", C.c_int32),
        ("minTwist", C.c_double), ("avgTwist", C.c_double), ("nTwistFaces", C.c_int64), ("nLowTwistFaces", C.c_int64),
        ("minTwistFace", C.c_int32),
        ("minTriangleTwist", C.c_double), ("avgTriangleTwist", C.c_double), ("nLowTriangleTwistFaces", C.c_int64),
        ("minTriangleTwistFace", C.c_int32),
    ]


class QualityCoupling(C.Structure):
    _fields_ = [("myRank", C.c_int32), ("nPatches", C.c_int32), ("patchStart", c_i32p), ("patchSize", c_i32p), ("neighbRank", c_i32p)]


class QualityConstraintHaloDesc(C.Structure):
    """smgpu_quality_constraint_halo_desc"""
    _fields_ = [("sendT", C.c_void_p), ("recvT", C.c_void_p), ("sendCc", C.c_void_p), ("recvCc", C.c_void_p), ("coupling", C.POINTER(QualityCoupling))]


class QualityConstraintHaloDescFull(C.Structure):
    """smgpu_quality_constraint_halo_desc_full: QualityConstraintHaloDesc's fields, then the volume buffers of DESIGN.md 10.17"""
    _fields_ = QualityConstraintHaloDesc._fields_ + [("sendVc", C.c_void_p), ("recvVc", C.c_void_p)]


class QualityPart(C.Structure):
    """smgpu_quality_part: Quality with sumNonOrth in place of avgNonOrth"""
    _fields_ = [("sumNonOrth" if n == "avgNonOrth" else n, t) for n, t in Quality._fields_]


def _sums(fields):
    return [("sum" + n[3:] if n.startswith("avg") else n, t) for n, t in fields]


class QualityGeometryPart(C.Structure):
    """smgpu_quality_geometry_part: the counted denominators, then QualityGeometry with every average replaced by its sum"""
    _fields_ = [("nCells", C.c_int64), ("nFaces", C.c_int64), ("nInternalFaces", C.c_int64)] + _sums(QualityGeometry._fields_)


class QualityMotionPart(C.Structure):
    """smgpu_quality_motion_part: the counted faces, then QualityMotion with every average replaced by its sum"""
    _fields_ = [("nFaces", C.c_int64)] + _sums(QualityMotion._fields_)


# every symbol include/smgpu.h declares: (restype, argtypes)
SYMBOLS = {
    "smgpu_last_error": (C.c_char_p, []),
    "smgpu_version": (C.c_char_p, []),
    "smgpu_create": (C.c_int, [C.POINTER(MeshDesc), C.POINTER(C.c_void_p)]),
    "smgpu_destroy": (C.c_int, [C.c_void_p]),
    "smgpu_get_sizes": (C.c_int, [C.c_void_p, C.POINTER(Sizes)]),
    "smgpu_mesh_stats": (C.c_int, [C.c_void_p, c_f64p, c_f64p]),
    "smgpu_set_params": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "smgpu_set_foam_variant": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_set_sync_variant": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_halo_set_push": (C.c_int, [C.c_void_p, C.POINTER(PushDesc)]),
    "smgpu_push_alloc": (C.c_int, [C.c_int32, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]),
    "smgpu_push_open": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smgpu_push_close": (C.c_int, [C.c_void_p]),
    "smgpu_push_free": (C.c_int, [C.c_void_p]),
    "smgpu_set_device_share": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_debug_walk_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "smgpu_debug_halo_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "smgpu_debug_halo_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "smgpu_debug_selftest_fpexact": (C.c_int, [C.c_int32, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_iterate": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.POINTER(IterStats), c_i32p]),
    "smgpu_get_points": (C.c_int, [C.c_void_p, c_f64p]),
    "smgpu_check_error": (C.c_int, [C.c_void_p]),
    "smgpu_get_near_ties": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "smgpu_set_points": (C.c_int, [C.c_void_p, c_f64p]),
    "smgpu_enable_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_get_counters": (C.c_int, [C.c_void_p, C.POINTER(Counters)]),
    "smgpu_reset_counters": (C.c_int, [C.c_void_p]),
    "smgpu_halo_configure": (C.c_int, [C.c_void_p, C.POINTER(HaloDesc)]),
    "smgpu_iter_begin": (C.c_int, [C.c_void_p]),
    "smgpu_iter_interior": (C.c_int, [C.c_void_p]),
    "smgpu_iter_mid": (C.c_int, [C.c_void_p]),
    "smgpu_iter_ahead": (C.c_int, [C.c_void_p]),
    "smgpu_halo_set_stats_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "smgpu_set_layers": (C.c_int, [C.c_void_p, C.POINTER(LayerDesc), c_i32p]),
    "smgpu_layers_begin": (C.c_int, [C.c_void_p, C.POINTER(LayerDesc), c_i32p, c_i32p]),
    "smgpu_layers_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "smgpu_layers_shared": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_f64p]),
    "smgpu_set_boundary_smoothing": (C.c_int, [C.c_void_p, C.POINTER(BoundaryDesc), C.POINTER(BoundaryInfo)]),
    "smgpu_boundary_stats": (C.c_int, [C.c_void_p, c_f64p, c_f64p]),
    "smgpu_boundary_begin": (C.c_int, [C.c_void_p, C.POINTER(BoundaryDesc), C.c_double, C.c_double, C.POINTER(BoundaryInfo)]),
    "smgpu_boundary_step": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_boundary_shared": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_f64p]),
    "smgpu_get_boundary_classification": (C.c_int, [C.c_void_p, c_i32p, c_i32p]),
    "smgpu_debug_edge_strings": (C.c_int, [C.c_int32, C.c_int32, c_i32p, c_i32p, c_i32p]),
    "smgpu_debug_find_line": (C.c_int, [C.c_void_p, C.c_int32, c_f64p, c_f64p, c_i32p]),
    "smgpu_halo_l_doubles": (C.c_int, [C.c_void_p, c_i32p]),
    "smgpu_halo_set_exchange_stream": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "smgpu_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "smgpu_iter_end": (C.c_int, [C.c_void_p]),
    "smgpu_mesh_quality": (C.c_int, [C.c_void_p, C.POINTER(QualityParams), C.POINTER(Quality)]),
    "smgpu_quality_field": (C.c_int, [C.c_void_p, C.c_char_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_set_quality_trace": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(QualityParams)]),
    "smgpu_get_quality_trace": (C.c_int, [C.c_void_p, C.POINTER(QualityTraceRecord), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_set_quality_guard": (C.c_int, [C.c_void_p, C.POINTER(QualityGuardParams), C.c_int32]),
    "smgpu_get_quality_guard": (C.c_int, [C.c_void_p, C.POINTER(QualityGuardState)]),
    "smgpu_quality_guard_restore": (C.c_int, [C.c_void_p]),
    "smgpu_set_tangle_constraint": (C.c_int, [C.c_void_p, C.POINTER(TangleParams), C.c_int32]),
    "smgpu_get_tangle_records": (C.c_int, [C.c_void_p, C.POINTER(TangleRecord), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_get_tangle_state": (C.c_int, [C.c_void_p, C.POINTER(TangleState)]),
    "smgpu_set_tangle_constraint_coupled": (C.c_int, [C.c_void_p, C.POINTER(TangleParams), C.POINTER(TangleHaloDesc), C.c_int32]),
    "smgpu_tangle_pass_begin": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "smgpu_tangle_pass_end": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "smgpu_set_quality_constraint": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintParams), C.c_int32]),
    "smgpu_get_quality_constraint_records": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintRecord), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_get_quality_constraint_state": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintState)]),
    "smgpu_set_quality_constraint_limits": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintLimits), C.c_int32]),
    "smgpu_get_quality_constraint_records_full": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintRecordFull), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_get_quality_constraint_state_full": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintStateFull)]),
    "smgpu_set_quality_constraint_coupled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintParams), C.POINTER(QualityConstraintHaloDesc), C.c_int32]),
    "smgpu_set_quality_constraint_limits_coupled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintLimits), C.POINTER(QualityConstraintHaloDescFull), C.c_int32]),
    "smgpu_set_quality_constraint_limits_all": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintLimitsAll), C.c_int32]),
    "smgpu_set_quality_constraint_limits_all_coupled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintLimitsAll), C.POINTER(QualityConstraintHaloDescFull), C.c_int32]),
    "smgpu_get_quality_constraint_records_all": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintRecordAll), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_get_quality_constraint_state_all": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintStateAll)]),
    "smgpu_set_quality_constraint_scaling": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintScaling)]),
    "smgpu_get_quality_constraint_records_scaled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintRecordScaled), C.c_int64, C.POINTER(C.c_int64)]),
    "smgpu_get_quality_constraint_state_scaled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintStateScaled)]),
    "smgpu_set_quality_constraint_scaling_coupled": (C.c_int, [C.c_void_p, C.POINTER(QualityConstraintScaling), C.POINTER(QualityScaleCoupling)]),
    "smgpu_quality_constraint_pass_scale": (C.c_int, [C.c_void_p, C.c_int64]),
    "smgpu_quality_constraint_pass_sweep": (C.c_int, [C.c_void_p]),
    "smgpu_set_boundary_revert": (C.c_int, [C.c_void_p, C.c_int32]),
    "smgpu_get_boundary_revert": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "smgpu_quality_constraint_coupled_exempt": (C.c_int, [C.c_void_p]),
    "smgpu_quality_constraint_pass_begin": (C.c_int, [C.c_void_p]),
    "smgpu_quality_constraint_pass_faces": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "smgpu_quality_constraint_pass_end": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "smgpu_quality_coupled_pack": (C.c_int, [C.c_void_p, C.POINTER(QualityCoupling), C.c_void_p, C.POINTER(C.c_int64)]),
    "smgpu_quality_coupled_report": (C.c_int, [C.c_void_p, C.POINTER(QualityParams), C.c_void_p, C.POINTER(QualityPart)]),
    "smgpu_quality_coupled_field": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_quality_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityParams), C.POINTER(C.c_int64), c_i32p, C.c_int64]),
    "smgpu_quality_coupled_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityParams), C.c_void_p, C.POINTER(C.c_int64), c_i32p, C.c_int64]),
    "smgpu_mesh_quality_geometry": (C.c_int, [C.c_void_p, C.POINTER(QualityGeometryParams), C.POINTER(QualityGeometry)]),
    "smgpu_quality_geometry_field": (C.c_int, [C.c_void_p, C.c_char_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_mesh_quality_motion": (C.c_int, [C.c_void_p, C.POINTER(QualityMotionParams), C.POINTER(QualityMotion)]),
    "smgpu_quality_motion_field": (C.c_int, [C.c_void_p, C.c_char_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_quality_coupled_pack_volumes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "smgpu_quality_coupled_geometry_report": (C.c_int, [C.c_void_p, C.POINTER(QualityGeometryParams), C.c_void_p, C.c_void_p,
                                                        C.POINTER(QualityGeometryPart)]),
    "smgpu_quality_coupled_geometry_field": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_quality_coupled_motion_report": (C.c_int, [C.c_void_p, C.POINTER(QualityMotionParams), C.c_void_p, C.POINTER(QualityMotionPart)]),
    "smgpu_quality_coupled_motion_field": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_quality_geometry_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityGeometryParams), C.POINTER(C.c_int64), c_i32p, C.c_int64]),
    "smgpu_quality_motion_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityMotionParams), C.POINTER(C.c_int64), c_i32p, C.c_int64]),
    "smgpu_quality_coupled_geometry_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityGeometryParams), C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_int64), c_i32p, C.c_int64]),
    "smgpu_quality_coupled_motion_sets": (C.c_int, [C.c_void_p, C.POINTER(QualityMotionParams), C.c_void_p, C.POINTER(C.c_int64), c_i32p,
                                                    C.c_int64]),
    "smgpu_debug_get_field": (C.c_int, [C.c_void_p, C.c_char_p, c_f64p, C.POINTER(C.c_int64)]),
    "smgpu_debug_get_addressing": (C.c_int, [C.c_void_p, C.c_char_p, c_i32p, c_i32p, C.POINTER(C.c_int64)]),
    "smgpu_debug_propose": (C.c_int, [C.c_void_p]),
    "smgpu_topology_create": (C.c_int, [C.POINTER(MeshDesc), C.POINTER(C.c_void_p)]),
    "smgpu_topology_get": (C.c_int, [C.c_void_p, C.c_char_p, c_i32p, c_i32p, C.POINTER(C.c_int64)]),
    "smgpu_topology_num_edges": (C.c_int, [C.c_void_p, c_i32p]),
    "smgpu_topology_checksums": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "smgpu_debug_addressing_checksums": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "smgpu_debug_tile_checksums": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "smgpu_topology_destroy": (C.c_int, [C.c_void_p]),
}

_lib = None


def lib():
    """Load csrc/libsmgpu.so.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C smoothmesh_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same soname as /opt/rocm's).
        # Whichever is loaded first serves both; if ours came first torch would later fail with "No HIP GPUs
        # are available", so let torch (when present) load its runtime before libsmgpu.so is opened.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib
