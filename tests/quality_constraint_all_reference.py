"""The quality constraint with the last four meshQualityDict limits -- maxConcave, minFlatness, minVol, minArea (include/smgpu.h
smgpu_set_quality_constraint_limits_all; DESIGN.md "Mesh quality", 10.18) -- restated on the CPU, as an extension of
tests/quality_constraint_full_reference.py's QualityConstraintFullReference: the loop, the passes and the nine older criteria are
its own; concavity (evaluated with concaveThreshold = maxConcave) and flatness are the geometry report's, from
quality_geometry_reference (tests/test_quality_geometry_reference.py), the area is |S_f| and the volume quality_reference's
cellVolume (tests/test_quality_reference.py), all on the oracle's phaseA fields.  A helper, not a test:
tests/test_quality_constraint_all_reference.py pins it, tests/test_gpu_quality_constraint_all.py holds the engine to it.

Conditions on the inputs, asserted on every evaluation that judges: the parent's margins, and for every non-exempt element judged
under a new limit that is on |value - limit| > LAST_MARGIN; for concavity that margin holds for every valid corner of a judged
face, on s against sin(maxConcave) and, where s >= sin(maxConcave) so that the side is read at all, on (c/s).n against SMALL."""
import copy
import math

import numpy as np

from quality_constraint_full_reference import FIELDS_FULL, QualityConstraintFullReference
from tangle_reference import make_oracle
from test_quality_geometry_reference import SMALL, quality_geometry_reference
from test_quality_reference import _mag, quality_reference

LAST_MARGIN = 1e-9
# limit -> (the value at which it is off: maxConcave at or above it, the others at or below it; the record's count)
LAST = {
    "maxConcave": (180.0, "nConcaveFaces"),
    "minFlatness": (0.0, "nWarpedFaces"),
    "minArea": (0.0, "nSmallAreaFaces"),
    "minVol": (0.0, "nSmallVolumeCells"),
}
LAST_FACE_LIMITS = ("maxConcave", "minFlatness", "minArea")
FIELDS_ALL = FIELDS_FULL + tuple(v[1] for v in LAST.values())
LAST_OFF = {k: v[0] for k, v in LAST.items()}
GAPS = ("cornerSin", "cornerSide", "minFlatness", "minArea", "minVol")


def last_on(name, value):
    return value < 180.0 if name == "maxConcave" else value > 0.0


class QualityConstraintAllReference(QualityConstraintFullReference):
    """`oracle`: as QualityConstraintReference's.  A limit that is None or at its off value is off."""

    def __init__(self, oracle, mesh, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2, **more):
        given = {k: more.pop(k) for k in list(more) if k in LAST}
        self.lastLim = {k: LAST_OFF[k] if given.get(k) is None else float(given[k]) for k in LAST}
        assert not any(math.isnan(v) for v in self.lastLim.values()) and self.lastLim["maxConcave"] >= 0.0
        self.onLast = {k: last_on(k, v) for k, v in self.lastLim.items()}
        self.sinT = math.sin(math.radians(self.lastLim["maxConcave"]))   # as the geometry report forms sin(concaveThreshold)
        self.minGapLast = {k: np.inf for k in GAPS}
        self.exemptVol = None
        self.lastShape = None
        super().__init__(oracle, mesh, maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes, **more)
        # the enabling evaluation: a face bad by any criterion that is on is exempt; a cell under minVol is exempt from the volume
        # criterion only
        for k in LAST_FACE_LIMITS:
            self.exemptFaces = self.exemptFaces | self.lastShape[k]
        self.nExemptFaces = int(self.exemptFaces.sum())
        self.exemptVol = self.lastShape["minVol"].copy()
        self.nExemptVolumeCells = int(self.exemptVol.sum())

    def _gap(self, key, values, limit, judged):
        if judged.any():
            self.minGapLast[key] = min(self.minGapLast[key], float(np.abs(values - limit)[judged].min()))
        assert self.minGapLast[key] > LAST_MARGIN, (key, self.minGapLast[key])

    def bad_faces(self, pts, judge=True):
        """the parent's verdicts; self.lastShape: the verdict of each of the four criteria at pts (faces, and cells for the volume),
        exempt ones included, all False for one that is off"""
        out = super().bad_faces(pts, judge)
        m = copy.copy(self.mesh)
        m.points = np.array(pts)
        F, C = m.nFaces, m.nCells
        self.lastShape = {k: np.zeros(C if k == "minVol" else F, bool) for k in LAST}
        if not any(self.onLast.values()):
            return out
        fc, fa, cc = (self.o.field(k).reshape(-1, 3).copy() for k in ("faceCentres", "faceAreas", "cellCentres"))
        judging = judge and self.exemptVol is not None
        judgedF = ~self.exemptFaces if judging else np.zeros(F, bool)
        if self.onLast["maxConcave"] or self.onLast["minFlatness"]:
            fg = quality_geometry_reference(m, fc, fa, cc, *self.cf, concaveThreshold=self.lastLim["maxConcave"])[1]
        if self.onLast["maxConcave"]:
            self.lastShape["maxConcave"] = fg["faceConcavity"] > SMALL
            # the face of every valid corner, in the order of fg["_cornerSin"]: quality_geometry_reference's own mask
            fo = m.faceOffsets.astype(np.int64)
            nv = np.diff(fo)
            rowOf = np.repeat(np.arange(F), nv)
            first = fo[:-1][rowOf]
            local = np.arange(fo[-1]) - first
            P = m.points[m.facePoints]
            valid = (_mag(P[first + (local + 1) % nv[rowOf]] - P) > SMALL) & (_mag(P - P[first + (local - 1) % nv[rowOf]]) > SMALL)
            assert int(valid.sum()) == len(fg["_cornerSin"])
            onJudged = judgedF[rowOf[valid]]
            self._gap("cornerSin", fg["_cornerSin"], self.sinT, onJudged)
            # (the side is read only at a corner with s >= sin(maxConcave); a hanging node's corner has s = 0 and side = 0 exactly,
            # and with the margin on s held no rounding takes it there: the condition of tests/test_gpu_quality_geometry.py)
            self._gap("cornerSide", fg["_cornerSide"], SMALL, onJudged & (fg["_cornerSin"] >= self.sinT))
        if self.onLast["minFlatness"]:
            v, summed = fg["faceFlatness"], fg["_summed"]
            self.lastShape["minFlatness"] = summed & (v < self.lastLim["minFlatness"])
            self._gap("minFlatness", v, self.lastLim["minFlatness"], judgedF & summed)
        if self.onLast["minArea"]:
            v = _mag(fa)
            self.lastShape["minArea"] = v < self.lastLim["minArea"]
            self._gap("minArea", v, self.lastLim["minArea"], judgedF)
        if self.onLast["minVol"]:
            v = quality_reference(m, fc, fa, cc, *self.cf)[1]["cellVolume"]
            self.lastShape["minVol"] = v < self.lastLim["minVol"]
            self._gap("minVol", v, self.lastLim["minVol"], ~self.exemptVol if judging else np.zeros(C, bool))
        return out

    def bad_cells(self, pts, judge=True):
        tangled = super().bad_cells(pts, judge)
        if self.exemptVol is None:                                       # enabling
            return tangled
        ok = ~self.exemptFaces
        last = {k: self.lastShape[k] & ok for k in LAST_FACE_LIMITS}
        vol = self.lastShape["minVol"] & ~self.exemptVol
        bad = last["maxConcave"] | last["minFlatness"] | last["minArea"]
        byFace = np.zeros(self.mesh.nCells, bool)
        byFace[self.own[bad]] = True
        Fi = self.mesh.nInternalFaces
        byFace[self.nei[:Fi][bad[:Fi]]] = True
        # (the parent has just made countMore, and made it the iteration's first if this is the evaluation at k = 0)
        self.countMore.update({LAST[k][1]: int(last[k].sum()) for k in LAST_FACE_LIMITS})
        self.countMore["nSmallVolumeCells"] = int(vol.sum())
        self.byLastFace = byFace                                         # (bad through a face of 10.18's criteria alone)
        self.byFace = self.byFace | byFace | vol
        return tangled

    def bad_now(self, pts):
        """(non-exempt bad faces, non-exempt bad cells: 10.12's, the determinant's and the volume's) at pts, without judging margins"""
        faces, cells = super().bad_now(pts)
        for k in LAST_FACE_LIMITS:
            faces = faces | (self.lastShape[k] & ~self.exemptFaces)
        return faces, cells | (self.lastShape["minVol"] & ~self.exemptVol)


def reference_run(oracle_lib, mesh, nIters, limits=None, passes=2, variant="com", constraints=True, **over):
    """dict(pts, recs, ref): the accepted points after every iteration, the records, the QualityConstraintAllReference"""
    ref = QualityConstraintAllReference(make_oracle(oracle_lib, mesh, variant, constraints, **over), mesh, passes=passes, **(limits or {}))
    pts, recs = ref.run(nIters)
    return dict(pts=pts, recs=recs, ref=ref)
