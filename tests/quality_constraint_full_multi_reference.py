"""The quality constraint with the tet, twist, weight, ratio and determinant limits on a decomposed mesh (include/smgpu.h
smgpu_set_quality_constraint_limits_coupled; DESIGN.md "Mesh quality", 10.17) restated on the CPU, as an extension of
tests/quality_constraint_multi_reference.py's QualityConstraintMultiReference: the loop, the marks, the verdict on the summed
count and the three old criteria are its own.  Per rank the six values come from the numpy lines of the decomposed reports
(tests/test_quality_geometry_motion_decomposed_reference.py: geometry_part_reference, motion_part_reference) on the oracle's phaseA
fields: a processor face takes the internal branch of every face criterion with C_N from recvCc and V_N from recvVc, which are
built as send_reference / paired_offsets build the reports'; a cell's determinant runs over its internal and its processor faces;
a processor face flags its owner on the rank that judges it and counts only on the side with myRank < neighbRank.  A helper, not
a test: tests/test_quality_constraint_full_multi_reference.py pins it against the serial restatement,
tests/test_gpu_quality_constraint_full_multirank.py holds the two smoothers of halo.py to it.

Conditions on the inputs, asserted on every judged evaluation and on every rank: the parent's margins; |value - limit| >
MORE_MARGIN for every non-exempt element judged under a new limit that is on; and, on every evaluation, enabling included, that
the two sides of every processor face reach the same verdict by every criterion (ties are excluded from the inputs, not
tolerated).  Per run it also counts the non-exempt bad verdicts on processor faces by criterion (procVerdictsMore) and the cells
whose determinant verdict differs between the widened and the serial face rule (detRuleDiffers)."""
import copy
import math

import numpy as np

from quality_constraint_full_reference import FACE_LIMITS, FIELDS_FULL, MORE, MORE_MARGIN, MORE_OFF  # noqa: F401
from quality_constraint_multi_reference import QualityConstraintMultiReference
from test_quality_decomposed_reference import send_reference
from test_quality_geometry_motion_decomposed_reference import geometry_part_reference, motion_part_reference
from test_quality_geometry_reference import quality_geometry_reference
from test_quality_reference import cell_faces, quality_reference

SUMMED_FULL = ("nBadCells", "nPointsReverted", "nTangledCells", "nNonOrthoFaces", "nSkewFaces") + tuple(v[1] for v in MORE.values())


class QualityConstraintFullMultiReference(QualityConstraintMultiReference):
    """`mesh` cut into `grid` boxes; limits: the three of QualityConstraintMultiReference and the six of MORE (None or the off
    value: off)"""

    def __init__(self, oracle_lib, mesh, grid, limits=None, passes=2, variant="com", constraints=True, **over):
        limits = dict(limits or {})
        more = {k: limits.pop(k) for k in list(limits) if k in MORE}
        self.more = {k: MORE_OFF[k] if more.get(k) is None else float(more[k]) for k in MORE}
        assert not any(math.isnan(v) for v in self.more.values())
        self.on = {k: self.more[k] > MORE_OFF[k] for k in MORE}
        self.minGap = {k: np.inf for k in MORE}
        self.procVerdictsMore = {k: 0 for k in FACE_LIMITS}
        self.detRuleDiffers = 0
        self.exemptDet = None
        self.lastMore = self.lastCounted = None
        self.cf = None
        self._first = None
        super().__init__(oracle_lib, mesh, grid, limits, passes, variant, constraints, **over)
        # the enabling evaluation (the parent's, which went through evaluate() below): a face bad by any criterion that is on is
        # exempt on each rank that holds it and counts on one; an under-determined cell is exempt from the determinant criterion only
        for r in range(self.world):
            for k in FACE_LIMITS:
                self.exemptFaces[r] = self.exemptFaces[r] | self.lastMore[r][k]
        self.nExemptFaces = [int((e & cnt).sum()) for e, cnt in zip(self.exemptFaces, self.lastCounted)]
        self.exemptDet = [m["minDeterminant"].copy() for m in self.lastMore]
        self.nExemptDeterminantCells = [int(e.sum()) for e in self.exemptDet]

    def evaluate(self, cur, judge=True):
        """the parent's; self.lastMore[r]: the verdict of every new criterion on rank r (faces, and cells for the determinant),
        exempt ones included, all False for one that is off; self.lastCounted[r]: the counted-once mask by face"""
        tangled, faces = super().evaluate(cur, judge)    # (leaves phaseA's fields of cur[r] in every rank's oracle)
        if self.cf is None:
            self.cf = [cell_faces(s.mesh) for s in self.subs]
            self.slotFace = [np.concatenate([np.arange(s, s + n) for s, n, _ in c[1]] + [np.zeros(0, np.int64)]).astype(np.int64) for c in self.couplings]
        self.lastCounted = [f[3] for f in faces]
        self.lastMore = [{k: np.zeros(s.mesh.nCells if k == "minDeterminant" else s.mesh.nFaces, bool) for k in MORE} for s in self.subs]
        for i, off, j, ooff, n in self.copies:
            for v in (0, 1):                                             # non-orthogonality, skewness
                a, b = faces[i][v][self.slotFace[i][off:off + n]], faces[j][v][self.slotFace[j][ooff:ooff + n]]
                assert (a == b).all(), ("the two sides of a processor face disagree", ("maxNonOrtho", "skewness")[v], i, j)
        if not any(self.on.values()):
            return tangled, faces
        meshes, geo, vols = [], [], []
        for s, ref, c, cf in zip(self.subs, self.refs, cur, self.cf):
            m = copy.copy(s.mesh)
            m.points = np.array(c)
            g = tuple(ref.o.field(k).reshape(-1, 3).copy() for k in ("faceCentres", "faceAreas", "cellCentres"))
            meshes.append(m)
            geo.append(g)
            vols.append(quality_reference(m, *g, *cf)[1]["cellVolume"])
        send = [send_reference(m, g[2], c) for m, g, c in zip(meshes, geo, self.couplings)]
        sendV = [send_reference(m, np.repeat(v[:, None], 3, axis=1), c)[:, 0] for m, v, c in zip(meshes, vols, self.couplings)]
        recv, recvV = [np.zeros_like(x) for x in send], [np.zeros_like(x) for x in sendV]
        for i, off, j, ooff, n in self.copies:
            recv[i][off:off + n] = send[j][ooff:ooff + n]
            recvV[i][off:off + n] = sendV[j][ooff:ooff + n]
        for r, (m, g, cf) in enumerate(zip(meshes, geo, self.cf)):
            F, C = m.nFaces, m.nCells
            fg = geometry_part_reference(m, *g, *cf, recv[r], recvV[r], self.couplings[r])[1]
            fm = motion_part_reference(m, *g, *cf, recv[r], self.couplings[r])[1]
            inner = np.arange(F) < m.nInternalFaces
            inner = inner | faces[r][2]                                  # internal in the global mesh
            summed = np.diff(m.faceOffsets.astype(np.int64)) > 3
            applies = dict(minTetQuality=np.ones(F, bool), minTwist=summed, minTriangleTwist=summed, minFaceWeight=inner, minVolRatio=inner,
                           minDeterminant=np.ones(C, bool))
            for k, (_, _, field) in MORE.items():
                if not self.on[k]:
                    continue
                v = (fg if field in fg else fm)[field]
                self.lastMore[r][k] = applies[k] & (v < self.more[k])
                exempt = None if self.exemptDet is None else (self.exemptDet[r] if k == "minDeterminant" else self.exemptFaces[r])
                judged = applies[k] & ~exempt if (judge and exempt is not None) else np.zeros(len(v), bool)
                if judged.any():
                    self.minGap[k] = min(self.minGap[k], float(np.abs(v - self.more[k])[judged].min()))
                assert self.minGap[k] > MORE_MARGIN, (k, self.minGap[k])
            if self.on["minDeterminant"]:                                # the serial rule on the sub-domain: every cell on a cut loses a face
                serial = quality_geometry_reference(m, *g, *cf)[1]["cellDeterminant"] < self.more["minDeterminant"]
                self.detRuleDiffers += int((serial != self.lastMore[r]["minDeterminant"]).sum())
        for i, off, j, ooff, n in self.copies:
            for k in FACE_LIMITS:
                a, b = self.lastMore[i][k][self.slotFace[i][off:off + n]], self.lastMore[j][k][self.slotFace[j][ooff:ooff + n]]
                assert (a == b).all(), ("the two sides of a processor face disagree", k, i, j)
        return tangled, faces

    def bad(self, cur, judge=True):
        """per rank (B, counts = (nTangledCells, nNonOrthoFaces, nSkewFaces), the cells of B bad only through processor faces);
        self._first: per rank the six counts of the first evaluation since step() began"""
        tangled, faces = self.evaluate(cur, judge)
        out, counts = [], []
        for r, (t, (nonOrtho, sk, proc, counted)) in enumerate(zip(tangled, faces)):
            ex = self.exemptFaces[r]
            nonOrtho, sk = nonOrtho & ~ex, sk & ~ex
            more = {k: self.lastMore[r][k] & ~ex for k in FACE_LIMITS}
            det = self.lastMore[r]["minDeterminant"] & ~self.exemptDet[r]
            badF = nonOrtho | sk
            for k in FACE_LIMITS:
                badF = badF | more[k]
                self.procVerdictsMore[k] += int((more[k] & proc).sum())
            mesh = self.subs[r].mesh
            Fi = mesh.nInternalFaces
            byFace = np.zeros(mesh.nCells, bool)
            byFace[self.own[r][badF]] = True
            byFace[self.nei[r][:Fi][badF[:Fi]]] = True
            byOther = np.zeros(mesh.nCells, bool)                        # ... through faces that are not processor faces, or the determinant
            byOther[self.own[r][badF & ~proc]] = True
            byOther[self.nei[r][:Fi][badF[:Fi]]] = True
            t = t & ~self.refs[r].exempt
            self.procVerdicts += int((badF & proc).sum())
            B = t | byFace | det
            out.append((B, (int(t.sum()), int((nonOrtho & counted).sum()), int((sk & counted).sum())), B & ~(t | byOther | det)))
            cm = {MORE[k][1]: int((more[k] & counted).sum()) for k in FACE_LIMITS}
            cm["nUnderdeterminedCells"] = int(det.sum())
            counts.append(cm)
        if self._first is None:
            self._first = counts
        return out

    def bad_now(self, cur):
        """per rank (non-exempt bad faces, non-exempt bad cells: 10.12's and the determinant's) at cur, without judging margins"""
        keep = self.procVerdicts, self.detRuleDiffers
        tangled, faces = self.evaluate(cur, judge=False)
        self.procVerdicts, self.detRuleDiffers = keep
        out = []
        for r, (t, (no, sk, _, _)) in enumerate(zip(tangled, faces)):
            bad = no | sk
            for k in FACE_LIMITS:
                bad = bad | self.lastMore[r][k]
            out.append((bad & ~self.exemptFaces[r], (t & ~self.refs[r].exempt) | (self.lastMore[r]["minDeterminant"] & ~self.exemptDet[r])))
        return out

    def step(self):
        self._first = None
        cur, recs, res, frz = super().step()
        for rec, first in zip(recs, self._first):
            rec.update(first)                                            # the counts of the evaluation at k = 0
        return cur, recs, res, frz

    def run(self, nIters):
        out = super().run(nIters)
        out["recs"] = combine_full(out["per_rank"])
        return out


def combine_full(per_rank):
    """the full records of the undecomposed mesh: passes and fullRevert are global values, the counts are sums"""
    out = []
    for recs in zip(*per_rank):
        assert len({(r["iteration"], r["passes"], r["fullRevert"]) for r in recs}) == 1, recs
        out.append(dict(iteration=recs[0]["iteration"], passes=recs[0]["passes"], fullRevert=recs[0]["fullRevert"],
                        **{f: sum(r[f] for r in recs) for f in SUMMED_FULL}))
    return out
