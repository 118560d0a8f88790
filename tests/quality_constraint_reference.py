"""The quality constraint (include/smgpu.h smgpu_set_quality_constraint; DESIGN.md "Mesh quality", 10.14) restated on the CPU, as
an extension of tests/tangle_reference.py's TangleReference: the loop and the passes are its own, the bad cells gain the owners
and neighbours of the faces that fail a limit.  ortho_f and skew_f are the report's, from quality_reference of
tests/test_quality_reference.py on the oracle's phaseA fields.  A helper, not a test: tests/test_quality_constraint_reference.py
pins it, tests/test_gpu_quality_constraint.py holds the engine to it bit for bit.

Conditions on the inputs, asserted on every evaluation that judges: the tangle reference's margin on volumes and pyramids, and for
every non-exempt face judged |ortho_f - cosT| > FACE_MARGIN and |skew_f - limit| / limit > FACE_MARGIN, so that a last-bit
difference in a cosine or a division cannot flip a verdict unnoticed."""
import copy
import math

import numpy as np

from tangle_reference import TangleReference, make_oracle
from test_quality_reference import cell_faces, quality_reference

FACE_MARGIN = 1e-9
FIELDS = ("iteration", "passes", "fullRevert", "nBadCells", "nPointsReverted", "nTangledCells", "nNonOrthoFaces", "nSkewFaces")
SHARED = ("iteration", "passes", "fullRevert", "nBadCells", "nPointsReverted")
OFF = dict(maxNonOrtho=180.0, maxInternalSkewness=0.0, maxBoundarySkewness=0.0)


class QualityConstraintReference(TangleReference):
    """`oracle`: an Oracle of `mesh` with its variant, parameters (and layers) set, at the points the constraint is enabled on"""

    def __init__(self, oracle, mesh, maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2):
        self.maxNonOrtho, self.maxInternalSkewness, self.maxBoundarySkewness = float(maxNonOrtho), float(maxInternalSkewness), float(maxBoundarySkewness)
        assert not any(math.isnan(v) for v in (self.maxNonOrtho, self.maxInternalSkewness, self.maxBoundarySkewness))
        self.cosT = math.cos(self.maxNonOrtho * (math.pi / 180.0))        # as qualityThresholds() forms the report's cosine
        self.cf = cell_faces(mesh)
        self.own, self.nei = mesh.owner.astype(np.int64), mesh.neighbour.astype(np.int64)
        self.minCosGap = self.minSkewGap = np.inf
        self.exemptFaces = None
        self.last = None
        super().__init__(oracle, mesh, passes)                           # evaluates the current points once: the exempt cells ...
        nonOrtho, skew = self.last                                       # ... and, on the same geometry, the exempt faces
        self.exemptFaces = nonOrtho | skew
        self.nExemptFaces = int(self.exemptFaces.sum())
        self.nExemptNonOrtho, self.nExemptSkew = int(nonOrtho.sum()), int(skew.sum())

    def bad_faces(self, pts, judge=True):
        """(bad by non-orthogonality, bad by a skewness limit) at pts, on the fields phaseA has just left, exempt ones included"""
        o, m = self.o, copy.copy(self.mesh)
        m.points = np.array(pts)
        fc, fa, cc = (o.field(k).reshape(-1, 3).copy() for k in ("faceCentres", "faceAreas", "cellCentres"))
        f = quality_reference(m, fc, fa, cc, *self.cf)[1]
        ortho, skew = f["faceOrtho"], f["faceSkewness"]
        Fi, F = m.nInternalFaces, m.nFaces
        internal = np.arange(F) < Fi
        nonOrtho = np.zeros(F, bool)
        sk = np.zeros(F, bool)
        judged = ~self.exemptFaces if (judge and self.exemptFaces is not None) else np.zeros(F, bool)
        if self.maxNonOrtho < 180.0:
            nonOrtho = internal & (ortho < self.cosT)
            if (judged & internal).any():
                self.minCosGap = min(self.minCosGap, float(np.abs(ortho - self.cosT)[judged & internal].min()))
        for on, lim in ((internal, self.maxInternalSkewness), (~internal, self.maxBoundarySkewness)):
            if lim > 0.0:
                sk |= on & (skew > lim)
                if (judged & on).any():
                    self.minSkewGap = min(self.minSkewGap, float((np.abs(skew - lim) / lim)[judged & on].min()))
        assert self.minCosGap > FACE_MARGIN and self.minSkewGap > FACE_MARGIN, (self.minCosGap, self.minSkewGap)
        return nonOrtho, sk

    def bad_cells(self, pts, judge=True):
        """the cells bad at pts: 10.12's, exempt ones included, and the owners and neighbours of the bad faces that are not exempt.
        self.last: the two face verdicts; self.count: (nTangledCells, nNonOrthoFaces, nSkewFaces) of this evaluation"""
        tangled = super().bad_cells(pts, judge)
        nonOrtho, skew = self.bad_faces(pts, judge)
        self.last = (nonOrtho, skew)
        if self.exemptFaces is None:                                     # enabling: 10.12's verdict alone makes a cell exempt
            return tangled
        nonOrtho, skew = nonOrtho & ~self.exemptFaces, skew & ~self.exemptFaces
        bad = nonOrtho | skew
        byFace = np.zeros(self.mesh.nCells, bool)
        byFace[self.own[bad]] = True
        Fi = self.mesh.nInternalFaces
        byFace[self.nei[:Fi][bad[:Fi]]] = True
        self.count = (int((tangled & ~self.exempt).sum()), int(nonOrtho.sum()), int(skew.sum()))
        # step() masks the result with ~exempt: a cell exempt as a cell stays bad through a non-exempt bad face
        self.byFace = byFace
        return tangled

    def step(self):
        o, P = self.o, self.passes
        x = o.points().copy()
        n, res, frz = o.iterate(1, 0.0)
        assert n == 1
        loop = o.points().copy()
        cur = loop.copy()
        self.iteration += 1
        rec = dict(iteration=self.iteration, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0, nSkewFaces=0)
        reverted = np.zeros(self.mesh.nPoints, bool)
        for k in range(P + 1):
            B = (self.bad_cells(cur) & ~self.exempt) | self.byFace
            if k == 0:
                rec["nBadCells"] = int(B.sum())
                rec["nTangledCells"], rec["nNonOrthoFaces"], rec["nSkewFaces"] = self.count
            if not B.any():
                break
            if k == P:
                reverted[:] = True
                rec["fullRevert"] = 1
            else:
                reverted[self.cpPoint[B[self.cpCell]]] = True
                rec["passes"] += 1
            cur[reverted] = x[reverted]
        rec["nPointsReverted"] = int((reverted & (loop != x).any(axis=1)).sum())
        o.set_points(cur)
        cur.setflags(write=False)
        return cur, rec, float(res[0]), int(frz[0])

    def bad_now(self, pts):
        """(non-exempt bad faces, non-exempt 10.12-bad cells) at pts, without judging margins: the invariant's measure"""
        tangled = TangleReference.bad_cells(self, pts, judge=False)
        nonOrtho, skew = self.bad_faces(pts, judge=False)
        return (nonOrtho | skew) & ~self.exemptFaces, tangled & ~self.exempt


def reference_run(oracle_lib, mesh, nIters, limits=None, passes=2, variant="com", constraints=True, **over):
    """dict(pts, recs, ref): the accepted points after every iteration, the records, the QualityConstraintReference"""
    ref = QualityConstraintReference(make_oracle(oracle_lib, mesh, variant, constraints, **over), mesh, passes=passes, **(limits or {}))
    pts, recs = ref.run(nIters)
    return dict(pts=pts, recs=recs, ref=ref)
