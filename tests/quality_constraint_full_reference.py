"""The quality constraint with the tet, twist, weight, ratio and determinant limits (include/smgpu.h
smgpu_set_quality_constraint_limits; DESIGN.md "Mesh quality", 10.16) restated on the CPU, as an extension of
tests/quality_constraint_reference.py's QualityConstraintReference: the loop, the passes and the three old criteria are its own;
the six values are the reports', from quality_motion_reference (tests/test_quality_motion_reference.py) and
quality_geometry_reference (tests/test_quality_geometry_reference.py) on the oracle's phaseA fields.  A helper, not a test:
tests/test_quality_constraint_full_reference.py pins it, tests/test_gpu_quality_constraint_full.py holds the engine to it.

Conditions on the inputs, asserted on every evaluation that judges: the parent's margins, and for every non-exempt element judged
under a new limit that is on |value - limit| > MORE_MARGIN (the values are O(1), so the margin is absolute, like FACE_MARGIN)."""
import copy
import math

import numpy as np

from quality_constraint_reference import FIELDS, QualityConstraintReference
from tangle_reference import TangleReference, make_oracle
from test_quality_geometry_reference import quality_geometry_reference
from test_quality_motion_reference import quality_motion_reference

MORE_MARGIN = 1e-9
# limit -> (the value at or below which it is off, the record's count, the field of the reference it judges)
MORE = {
    "minTetQuality": (-1e30, "nLowTetFaces", "faceTetQuality"),
    "minTwist": (-1.0, "nLowTwistFaces", "faceTwist"),
    "minTriangleTwist": (-1.0, "nLowTriangleTwistFaces", "faceTriangleTwist"),
    "minFaceWeight": (0.0, "nLowWeightFaces", "faceWeight"),
    "minVolRatio": (0.0, "nLowVolRatioFaces", "faceVolumeRatio"),
    "minDeterminant": (0.0, "nUnderdeterminedCells", "cellDeterminant"),
}
FACE_LIMITS = tuple(k for k in MORE if k != "minDeterminant")
FIELDS_FULL = FIELDS + tuple(v[1] for v in MORE.values())
MORE_OFF = {k: v[0] for k, v in MORE.items()}


class QualityConstraintFullReference(QualityConstraintReference):
    """`oracle`: as QualityConstraintReference's.  A new limit that is None or at its off value is off."""

    def __init__(self, oracle, mesh, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2, **more):
        assert set(more) <= set(MORE), more
        self.more = {k: MORE_OFF[k] if more.get(k) is None else float(more[k]) for k in MORE}
        assert not any(math.isnan(v) for v in self.more.values())
        self.on = {k: self.more[k] > MORE_OFF[k] for k in MORE}
        self.minGap = {k: np.inf for k in MORE}
        self.exemptDet = None
        self.lastMore = None
        super().__init__(oracle, mesh, maxNonOrtho, maxInternalSkewness, maxBoundarySkewness, passes)
        # the enabling evaluation: a face bad by any criterion that is on is exempt; an under-determined cell is exempt from the
        # determinant criterion only
        for k in FACE_LIMITS:
            self.exemptFaces = self.exemptFaces | self.lastMore[k]
        self.nExemptFaces = int(self.exemptFaces.sum())
        self.exemptDet = self.lastMore["minDeterminant"].copy()
        self.nExemptDeterminantCells = int(self.exemptDet.sum())

    def bad_faces(self, pts, judge=True):
        """the parent's two verdicts; self.lastMore: the verdict of every new criterion at pts (faces, and cells for the
        determinant), exempt ones included, all False for one that is off"""
        out = super().bad_faces(pts, judge)
        m = copy.copy(self.mesh)
        m.points = np.array(pts)
        F, Fi, C = m.nFaces, m.nInternalFaces, m.nCells
        self.lastMore = {k: np.zeros(C if k == "minDeterminant" else F, bool) for k in MORE}
        if not any(self.on.values()):
            return out
        fc, fa, cc = (self.o.field(k).reshape(-1, 3).copy() for k in ("faceCentres", "faceAreas", "cellCentres"))
        fm = quality_motion_reference(m, fc, fa, cc, *self.cf)[1]
        fg = quality_geometry_reference(m, fc, fa, cc, *self.cf)[1]
        internal = np.arange(F) < Fi
        summed = np.diff(m.faceOffsets.astype(np.int64)) > 3
        applies = dict(minTetQuality=np.ones(F, bool), minTwist=summed, minTriangleTwist=summed, minFaceWeight=internal, minVolRatio=internal,
                       minDeterminant=np.ones(C, bool))
        for k, (_, _, field) in MORE.items():
            if not self.on[k]:
                continue
            v = (fg if field in fg else fm)[field]
            self.lastMore[k] = applies[k] & (v < self.more[k])
            exempt = self.exemptDet if k == "minDeterminant" else self.exemptFaces
            judged = applies[k] & ~exempt if (judge and exempt is not None) else np.zeros(len(v), bool)
            if judged.any():
                self.minGap[k] = min(self.minGap[k], float(np.abs(v - self.more[k])[judged].min()))
            assert self.minGap[k] > MORE_MARGIN, (k, self.minGap[k])
        return out

    def bad_cells(self, pts, judge=True):
        tangled = TangleReference.bad_cells(self, pts, judge)
        nonOrtho, skew = self.bad_faces(pts, judge)
        self.last = (nonOrtho, skew)
        if self.exemptFaces is None:                                     # enabling
            return tangled
        ok = ~self.exemptFaces
        nonOrtho, skew = nonOrtho & ok, skew & ok
        more = {k: self.lastMore[k] & ok for k in FACE_LIMITS}
        det = self.lastMore["minDeterminant"] & ~self.exemptDet
        bad = nonOrtho | skew
        for k in FACE_LIMITS:
            bad = bad | more[k]
        byFace = np.zeros(self.mesh.nCells, bool)
        byFace[self.own[bad]] = True
        Fi = self.mesh.nInternalFaces
        byFace[self.nei[:Fi][bad[:Fi]]] = True
        self.count = (int((tangled & ~self.exempt).sum()), int(nonOrtho.sum()), int(skew.sum()))
        self.countMore = {MORE[k][1]: int(more[k].sum()) for k in FACE_LIMITS}
        self.countMore["nUnderdeterminedCells"] = int(det.sum())
        if self._first is None:
            self._first = self.countMore
        # (step() takes byFace as "bad whatever the cell's own exemption": the determinant verdict has its own)
        self.byFace = byFace | det
        return tangled

    _first = None

    def step(self):
        self._first = None
        cur, rec, res, frz = super().step()
        rec.update(self._first)                                          # the counts of the evaluation at k = 0
        return cur, rec, res, frz

    def bad_now(self, pts):
        """(non-exempt bad faces, non-exempt bad cells: 10.12's and the determinant's) at pts, without judging margins"""
        tangled = TangleReference.bad_cells(self, pts, judge=False)
        nonOrtho, skew = self.bad_faces(pts, judge=False)
        bad = nonOrtho | skew
        for k in FACE_LIMITS:
            bad = bad | self.lastMore[k]
        return bad & ~self.exemptFaces, (tangled & ~self.exempt) | (self.lastMore["minDeterminant"] & ~self.exemptDet)


def reference_run(oracle_lib, mesh, nIters, limits=None, passes=2, variant="com", constraints=True, **over):
    """dict(pts, recs, ref): the accepted points after every iteration, the records, the QualityConstraintFullReference"""
    ref = QualityConstraintFullReference(make_oracle(oracle_lib, mesh, variant, constraints, **over), mesh, passes=passes, **(limits or {}))
    pts, recs = ref.run(nIters)
    return dict(pts=pts, recs=recs, ref=ref)
