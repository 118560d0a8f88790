"""The quality constraint with scaling passes (include/smgpu.h smgpu_set_quality_constraint_scaling; DESIGN.md "Mesh quality",
10.19) restated on the CPU, as an extension of tests/quality_constraint_all_reference.py's QualityConstraintAllReference: the
verdicts, the exemptions and the margins are its own -- every judged evaluation, the scaled ones included, asserts MARGIN,
FACE_MARGIN, MORE_MARGIN and LAST_MARGIN -- and step() is the contract of 10.19: a scale per point that the marked passes multiply
by errorReduction (k < S) or set to zero (S <= k < S + P), nSmoothScale Jacobi sweeps over the engine's pointPoints rows, and the
current points x + s (L - x).  A helper, not a test: tests/test_quality_constraint_scaled_reference.py pins it,
tests/test_gpu_quality_constraint_scaled.py holds the engine to it bit for bit.

The sweeps' sums are left folds from 0.0 in row order (np.add.accumulate along the padded rows, never np.sum, whose pairwise order
is another); the division is numpy's, correctly rounded; a + s * (b - a) is three separate IEEE operations."""
import numpy as np

from quality_constraint_all_reference import FIELDS_ALL, QualityConstraintAllReference
from tangle_reference import make_oracle

FIELDS_SCALED = FIELDS_ALL + ("nScalePasses", "nPointsScaled", "minScale")


class QualityConstraintScaledReference(QualityConstraintAllReference):
    """`oracle`, the limits and `passes`: as QualityConstraintAllReference's.  scalePasses = 0: its step()."""

    def __init__(self, oracle, mesh, *args, scalePasses=0, errorReduction=0.75, nSmoothScale=4, **kw):
        self.S, self.r, self.nSweeps = int(scalePasses), float(errorReduction), int(nSmoothScale)
        assert self.S >= 0 and 0.0 <= self.r < 1.0 and self.nSweeps >= 0
        super().__init__(oracle, mesh, *args, **kw)
        from smoothmesh_amd.engine import HostTopology
        off, val = HostTopology(mesh).addressing("pointPoints")
        off = off.astype(np.int64)
        self.deg = np.diff(off)
        assert len(self.deg) == mesh.nPoints
        # the rows padded to the widest: column j holds the j-th neighbour, or the extra slot nPoints (whose scale is 0.0: adding
        # +0.0 behind a row's end leaves the partial sum's bits, and the row's own sum is read at column deg - 1)
        width = max(1, int(self.deg.max()) if len(self.deg) else 1)
        self.rows = np.full((mesh.nPoints, width), mesh.nPoints, np.int64)
        col = np.arange(off[-1]) - np.repeat(off[:-1], self.deg)
        self.rows[np.repeat(np.arange(mesh.nPoints), self.deg), col] = val
        self.last_scale = None

    def sweep(self, s):
        """one Jacobi sweep of 10.19 over every point"""
        ext = np.append(s, 0.0)
        acc = np.add.accumulate(np.concatenate([np.zeros((len(s), 1)), ext[self.rows]], axis=1), axis=1)   # the fold starts from 0.0
        has = self.deg > 0
        total = acc[np.arange(len(s)), self.deg]
        mean = np.divide(total, self.deg, out=np.zeros_like(s), where=has)
        t = 0.5 * s + 0.5 * mean
        return np.where(has, np.minimum(s, t), s)

    def step(self):
        if self.S == 0:
            cur, rec, res, frz = super().step()
            return cur, {**rec, "nScalePasses": 0, "nPointsScaled": 0, "minScale": 0.0}, res, frz
        o, S, T = self.o, self.S, self.S + self.passes
        self._first = None
        x = o.points().copy()
        n, res, frz = o.iterate(1, 0.0)
        assert n == 1
        loop = o.points().copy()
        cur = loop.copy()
        self.iteration += 1
        rec = dict(iteration=self.iteration, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0, nSkewFaces=0)
        nScalePasses = 0
        s = np.ones(self.mesh.nPoints)
        for k in range(T + 1):
            B = (self.bad_cells(cur) & ~self.exempt) | self.byFace
            if k == 0:
                rec["nBadCells"] = int(B.sum())
                rec["nTangledCells"], rec["nNonOrthoFaces"], rec["nSkewFaces"] = self.count
            if not B.any():
                break
            if k == T:
                s = np.zeros_like(s)
                rec["fullRevert"] = 1
            else:
                M = np.zeros(self.mesh.nPoints, bool)
                M[self.cpPoint[B[self.cpCell]]] = True
                s = np.where(M, s * self.r if k < S else 0.0, s)
                rec["passes"] += 1
                nScalePasses += k < S
                for _ in range(self.nSweeps):
                    s = self.sweep(s)
            d = loop - x
            mid = x + s[:, None] * d
            cur = np.where((s == 1.0)[:, None], loop, np.where((s == 0.0)[:, None], x, mid))
        moved = (loop != x).any(axis=1)
        rec["nPointsReverted"] = int(((cur == x).all(axis=1) & moved).sum())
        rec.update(self._first)                                          # the counts of the evaluation at k = 0
        rec["nScalePasses"] = int(nScalePasses)
        rec["nPointsScaled"] = int(((s > 0.0) & (s < 1.0) & moved).sum())
        rec["minScale"] = float(s.min()) if len(s) else 1.0
        self.last_scale = s
        o.set_points(cur)
        cur.setflags(write=False)
        return cur, rec, float(res[0]), int(frz[0])


def reference_run(oracle_lib, mesh, nIters, limits=None, passes=2, variant="com", constraints=True, scaling=None, **over):
    """dict(pts, recs, ref, res, frz): the accepted points after every iteration, the records, the reference, residuals and frozen
    counts; scaling: dict(scalePasses, errorReduction, nSmoothScale) or None (off)"""
    ref = QualityConstraintScaledReference(make_oracle(oracle_lib, mesh, variant, constraints, **over), mesh, passes=passes, **(limits or {}), **(scaling or {}))
    out = [ref.step() for _ in range(nIters)]
    return dict(pts=[s[0] for s in out], recs=[s[1] for s in out], ref=ref, res=[s[2] for s in out], frz=[s[3] for s in out])
