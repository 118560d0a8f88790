"""The quality constraint on a decomposed mesh (include/smgpu.h smgpu_set_quality_constraint_coupled; DESIGN.md "Mesh quality", 10.15)
restated on the CPU, as an extension of tests/tangle_multi_reference.py's TangleMultiReference: the loop, the marks OR-ed over the
copies of a point and the verdict on the summed count are its own; the bad cells gain the owners and neighbours of the faces that
fail a limit.  Per rank ortho_f and skew_f come from the oracle's phaseA fields with the report's formulas
(tests/test_quality_decomposed_reference.py): a processor face takes the internal form with C_N from recvCc, which is built as
send_reference / paired_offsets build the coupled report's; it is tested against the two internal limits, flags its owner on the
rank that judges it, and counts only on the side with myRank < neighbRank.  A helper, not a test:
tests/test_quality_constraint_multi_reference.py pins it against the serial restatement,
tests/test_gpu_quality_constraint_multirank.py holds the two smoothers of halo.py to it.

Conditions on the inputs, asserted on every judged evaluation and on every rank: tangle_reference's MARGIN on volumes and pyramids,
quality_constraint_reference's FACE_MARGIN on every non-exempt face.  Per run it also counts the bad verdicts on processor faces
(procVerdicts: both sides' verdicts, every evaluation), the marked passes in which a rank is bad only through a processor face
(procOnly), and the cells of marked passes that are bad through nothing but a processor face (procOnlyCells): the cells a verdict
without recvCc would miss."""
import math

import numpy as np

from quality_constraint_reference import FACE_MARGIN, FIELDS, OFF, SHARED  # noqa: F401
from tangle_multi_reference import MARGIN, TangleMultiReference  # noqa: F401
from test_quality_decomposed_reference import coupling_of, send_reference
from test_quality_reference import ROOTVSMALL, VSMALL, _dot, _mag

SUMMED = ("nBadCells", "nPointsReverted", "nTangledCells", "nNonOrthoFaces", "nSkewFaces")


def face_values(mesh, pts, fc, fa, cc, recvCc, coupling):
    """(ortho_f, skew_f, internal in the global mesh, processor face, counted on this rank) of every face of a sub-domain at pts:
    coupled_part_reference's lines"""
    rank, pats = coupling
    F, Fi = mesh.nFaces, mesh.nInternalFaces
    own = mesh.owner.astype(np.int64)
    inner = np.zeros(F, bool)
    inner[:Fi] = True
    proc = np.zeros(F, bool)
    counted = np.ones(F, bool)
    CN = np.zeros((F, 3))
    CN[:Fi] = cc[mesh.neighbour]
    k = 0
    for s, n, o in pats:
        inner[s:s + n] = True
        proc[s:s + n] = True
        CN[s:s + n] = recvCc[k:k + n]
        counted[s:s + n] = rank < o
        k += n
    magSf = _mag(fa)
    CO = cc[own]
    Cpf = fc - CO
    d = CN - CO
    ortho = np.where(inner, _dot(d, fa) / (_mag(d) * magSf + VSMALL), 1.0)
    nb = fa / (magSf + ROOTVSMALL)[:, None]
    d = np.where(inner[:, None], d, _dot(nb, Cpf)[:, None] * nb)
    sv = Cpf - (_dot(fa, Cpf) / (_dot(fa, d) + ROOTVSMALL))[:, None] * d
    magSv = _mag(sv)
    sHat = sv / (magSv + ROOTVSMALL)[:, None]
    fo = mesh.faceOffsets.astype(np.int64)
    rowOf = np.repeat(np.arange(F), np.diff(fo))
    proj = np.abs(_dot(np.repeat(sHat, np.diff(fo), axis=0), np.asarray(pts)[mesh.facePoints] - fc[rowOf]))
    skew = magSv / np.maximum(0.2 * _mag(d) + ROOTVSMALL, np.maximum.reduceat(proj, fo[:-1]))
    return ortho, skew, inner, proc, counted


class QualityConstraintMultiReference(TangleMultiReference):
    """`mesh` cut into `grid` boxes; parameters as TangleMultiReference's; limits as QualityConstraintReference's"""

    def __init__(self, oracle_lib, mesh, grid, limits=None, passes=2, variant="com", constraints=True, **over):
        from smoothmesh_amd.quality import paired_offsets
        super().__init__(oracle_lib, mesh, grid, passes, variant, constraints, **over)     # the exempt cells, per rank
        lim = dict(maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0, **{})
        lim.update(limits or {})
        self.maxNonOrtho, self.maxInternalSkewness, self.maxBoundarySkewness = (float(lim[k]) for k in ("maxNonOrtho", "maxInternalSkewness", "maxBoundarySkewness"))
        assert not any(math.isnan(v) for v in (self.maxNonOrtho, self.maxInternalSkewness, self.maxBoundarySkewness))
        self.cosT = math.cos(self.maxNonOrtho * (math.pi / 180.0))        # as qualityThresholds() forms the report's cosine
        self.couplings = [coupling_of(s.mesh, s.rank) for s in self.subs]
        self.copies = paired_offsets(self.couplings)
        self.own = [s.mesh.owner.astype(np.int64) for s in self.subs]
        self.nei = [s.mesh.neighbour.astype(np.int64) for s in self.subs]
        self.minCosGap = self.minSkewGap = np.inf
        self.procVerdicts = 0
        self.procOnly = 0
        self.procOnlyCells = 0
        self.exemptFaces = None
        # the exempt faces: the geometry of the points the constraint is enabled on, one exchange of cell centres
        _, faces = self.evaluate([o.points().copy() for o in self.orcs], judge=False)
        self.exemptFaces = [no | sk for no, sk, _, _ in faces]
        self.nExemptFaces = [int((e & cnt).sum()) for e, (_, _, _, cnt) in zip(self.exemptFaces, faces)]

    def evaluate(self, cur, judge=True):
        """every rank's geometry of its points cur[r], the exchange of the owner cell centres of the processor faces, the
        verdicts: ([10.12's bad cells, exempt ones included], [(bad by non-orthogonality, bad by a skewness limit, processor
        face, counted) per face, exempt ones included])"""
        tangled, geo = [], []
        for ref, c in zip(self.refs, cur):
            tangled.append(ref.bad_cells(c, judge))                      # (leaves phaseA's fields of c in the rank's oracle)
            geo.append(tuple(ref.o.field(k).reshape(-1, 3).copy() for k in ("faceCentres", "faceAreas", "cellCentres")))
        send = [send_reference(s.mesh, g[2], c) for s, g, c in zip(self.subs, geo, self.couplings)]
        recv = [np.zeros_like(x) for x in send]
        for i, off, j, ooff, n in self.copies:
            recv[i][off:off + n] = send[j][ooff:ooff + n]
        faces = []
        for r, (s, c, g) in enumerate(zip(self.subs, cur, geo)):
            ortho, skew, inner, proc, counted = face_values(s.mesh, c, *g, recv[r], self.couplings[r])
            F = s.mesh.nFaces
            judged = ~self.exemptFaces[r] if (judge and self.exemptFaces is not None) else np.zeros(F, bool)
            nonOrtho, sk = np.zeros(F, bool), np.zeros(F, bool)
            if self.maxNonOrtho < 180.0:
                nonOrtho = inner & (ortho < self.cosT)
                if (judged & inner).any():
                    self.minCosGap = min(self.minCosGap, float(np.abs(ortho - self.cosT)[judged & inner].min()))
            for on, lim in ((inner, self.maxInternalSkewness), (~inner, self.maxBoundarySkewness)):
                if lim > 0.0:
                    sk |= on & (skew > lim)
                    if (judged & on).any():
                        self.minSkewGap = min(self.minSkewGap, float((np.abs(skew - lim) / lim)[judged & on].min()))
            assert self.minCosGap > FACE_MARGIN and self.minSkewGap > FACE_MARGIN, (self.minCosGap, self.minSkewGap)
            faces.append((nonOrtho, sk, proc, counted))
        return tangled, faces

    def bad(self, cur, judge=True):
        """per rank (B, counts = (nTangledCells, nNonOrthoFaces, nSkewFaces), the cells of B bad only through processor faces)"""
        tangled, faces = self.evaluate(cur, judge)
        out = []
        for r, (t, (nonOrtho, sk, proc, counted)) in enumerate(zip(tangled, faces)):
            ex = self.exemptFaces[r]
            nonOrtho, sk = nonOrtho & ~ex, sk & ~ex
            badF = nonOrtho | sk
            mesh = self.subs[r].mesh
            Fi = mesh.nInternalFaces
            byFace = np.zeros(mesh.nCells, bool)
            byFace[self.own[r][badF]] = True
            byFace[self.nei[r][:Fi][badF[:Fi]]] = True
            byOther = np.zeros(mesh.nCells, bool)                        # ... through faces that are not processor faces
            byOther[self.own[r][badF & ~proc]] = True
            byOther[self.nei[r][:Fi][badF[:Fi]]] = True
            t = t & ~self.refs[r].exempt
            self.procVerdicts += int((badF & proc).sum())
            B = t | byFace
            out.append((B, (int(t.sum()), int((nonOrtho & counted).sum()), int((sk & counted).sum())),
                        B & ~(t | byOther)))
        return out

    def bad_now(self, cur):
        """per rank (non-exempt bad faces, non-exempt 10.12-bad cells) at cur, without judging margins: the invariant's measure"""
        keep = self.procVerdicts
        tangled, faces = self.evaluate(cur, judge=False)
        self.procVerdicts = keep
        return [((no | sk) & ~ex, t & ~ref.exempt) for t, (no, sk, _, _), ex, ref in zip(tangled, faces, self.exemptFaces, self.refs)]

    def step(self):
        """one iteration of the loop on every rank and the passes behind it; returns (accepted points per rank, record per rank,
        residual, nFrozenPoints)"""
        P, W = self.passes, self.world
        x = [o.points().copy() for o in self.orcs]
        n, res, frz = self.mo.iterate(1, 0.0)
        assert n == 1
        loop = [o.points().copy() for o in self.orcs]
        cur = [p.copy() for p in loop]
        moved = [(a != b).any(axis=1) for a, b in zip(loop, x)]
        self.iteration += 1
        recs = [dict(iteration=self.iteration, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0,
                     nSkewFaces=0) for _ in range(W)]
        reverted = [np.zeros(len(p), bool) for p in cur]
        for k in range(P + 1):
            ev = self.bad(cur)
            B = [e[0] for e in ev]
            if k == 0:
                for rec, (b, cnt, _) in zip(recs, ev):
                    rec["nBadCells"] = int(b.sum())
                    rec["nTangledCells"], rec["nNonOrthoFaces"], rec["nSkewFaces"] = cnt
            if sum(int(b.sum()) for b in B) == 0:          # the verdict: on the whole mesh
                break
            if k == P:
                for rec, rv in zip(recs, reverted):
                    rv[:] = True
                    rec["fullRevert"] = 1
            else:
                self.procOnly += sum(1 for e in ev if e[0].any() and (e[0] == e[2]).all())
                self.procOnlyCells += sum(int(e[2].sum()) for e in ev)
                marks = np.zeros(self.mesh.nPoints, bool)   # OR over the copies of a point
                for ref, b, a in zip(self.refs, B, self.ppa):
                    m = np.zeros(len(a), bool)
                    m[ref.cpPoint[b[ref.cpCell]]] = True
                    marks[a[m]] = True
                for r in range(W):
                    got = marks[self.ppa[r]]
                    if not B[r].any() and got.any():
                        self.foreign.append((self.iteration, k, r, int(got.sum()), int((got & moved[r]).sum())))
                    reverted[r] |= got
                    recs[r]["passes"] += 1
            for c, rv, x0 in zip(cur, reverted, x):
                c[rv] = x0[rv]
        for r in range(W):
            recs[r]["nPointsReverted"] = int((reverted[r] & moved[r] & self.master[r]).sum())
            self.orcs[r].set_points(cur[r])
            cur[r].setflags(write=False)
        return cur, recs, float(res[0]), int(frz[0])

    def run(self, nIters):
        out = [self.step() for _ in range(nIters)]
        per_rank = [[s[1][r] for s in out] for r in range(self.world)]
        return dict(pts=[s[0] for s in out], per_rank=per_rank, recs=combine(per_rank), res=np.array([s[2] for s in out]),
                    frz=np.array([s[3] for s in out], np.int64), ref=self)


def combine(per_rank):
    """the records of the undecomposed mesh: passes and fullRevert are global values, the counts are sums"""
    out = []
    for recs in zip(*per_rank):
        assert len({(r["iteration"], r["passes"], r["fullRevert"]) for r in recs}) == 1, recs
        out.append(dict(iteration=recs[0]["iteration"], passes=recs[0]["passes"], fullRevert=recs[0]["fullRevert"],
                        **{f: sum(r[f] for r in recs) for f in SUMMED}))
    return out
