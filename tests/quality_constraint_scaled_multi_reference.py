"""The quality constraint's scaling passes on a decomposed mesh (include/smgpu.h smgpu_set_quality_constraint_scaling_coupled;
DESIGN.md "Mesh quality", 10.20) restated on the CPU, as an extension of tests/quality_constraint_full_multi_reference.py's
QualityConstraintFullMultiReference, the widest restatement of the decomposed constraint: the loop, the verdicts, the exemptions
and the margins are its own -- every judged evaluation, the scaled ones included, asserts the parents' margins on every rank --
and step() is the contract of 10.20:
  1. the marks are OR-ed over the copies of a point and the verdict is taken on the summed count, for k = 0 .. S + P;
  2. every rank turns the combined marks into scales on its own copy of the field;
  3. a sweep of a shared point runs over its neighbours in the whole mesh: per rank the partial sum over the COUNTED entries of
     its pointPoints row -- an entry (p, q) of rank R is counted iff R is the lowest rank whose sub-domain holds the edge pq --
     a left fold from 0.0 in row order; the total the left fold from 0.0 of the partial sums over the sharers in ascending rank;
     the degree the number of counted entries over all ranks; an unshared point is 10.19's;
  4. the accepted points are 10.19's on every rank;
  5. per rank a record: passes, fullRevert and nScalePasses global, nPointsReverted and nPointsScaled on the master of a shared
     point only, minScale the rank's own.
Which entries are counted, and the degrees, are worked out here from the definition -- sets of edges by the names (sharedGlobal,
sharedComp) of their ends -- not by smoothmesh_amd.halo.scale_tables, which tests/test_quality_constraint_scaled_multi_host.py holds
to a count on the undecomposed mesh.  Sums are left folds (np.add.accumulate along padded rows; a loop over the ranks), never np.sum.
After every pass it asserts that the copies of a shared point's scale are equal.  A helper, not a test:
tests/test_quality_constraint_scaled_multi_reference.py pins it against the serial restatement,
tests/test_gpu_quality_constraint_scaled_multirank.py holds the two smoothers of halo.py to it."""
import numpy as np

from quality_constraint_full_multi_reference import SUMMED_FULL, QualityConstraintFullMultiReference

SUMMED_SCALED = SUMMED_FULL + ("nPointsScaled",)
GLOBAL_SCALED = ("iteration", "passes", "fullRevert", "nScalePasses")


class QualityConstraintScaledMultiReference(QualityConstraintFullMultiReference):
    """`mesh` cut into `grid` boxes; limits and passes as QualityConstraintFullMultiReference's; scalePasses = 0: its step()"""

    def __init__(self, oracle_lib, mesh, grid, limits=None, passes=2, variant="com", constraints=True, scalePasses=0, errorReduction=0.75,
                 nSmoothScale=4, **over):
        self.S, self.r, self.nSweeps = int(scalePasses), float(errorReduction), int(nSmoothScale)
        assert self.S >= 0 and 0.0 <= self.r < 1.0 and self.nSweeps >= 0
        super().__init__(oracle_lib, mesh, grid, limits, passes, variant, constraints, **over)
        from smoothmesh_amd.engine import HostTopology
        from smoothmesh_amd.halo import HaloTables
        cands = [s.processor_patch_point_lists() for s in self.subs]
        self.tables = [HaloTables(s.rank, s.pointProcAddressing, cands) for s in self.subs]
        self.rows, self.deg = [], []                      # every rank's pointPoints rows, padded (10.19's, per sub-domain)
        self.sharedRows = []                              # per rank: the counted rows of its shared points, padded
        held = []                                         # per rank: the edges between two shared points its sub-domain holds
        names = {}                                        # (sharedGlobal, sharedComp) -> index
        flat = []
        for s, t in zip(self.subs, self.tables):
            nP = s.mesh.nPoints
            off, val = (np.asarray(a, np.int64) for a in HostTopology(s.mesh).addressing("pointPoints"))
            deg = np.diff(off)
            rows = np.full((nP, max(1, int(deg.max()) if nP else 1)), nP, np.int64)
            rows[np.repeat(np.arange(nP), deg), np.arange(off[-1]) - np.repeat(off[:-1], deg)] = val
            self.rows.append(rows)
            self.deg.append(deg)
            name = {int(p): (int(g), int(c)) for p, g, c in zip(t.sharedLocal, t.sharedGlobal, t.sharedComp)}
            for n in name.values():
                names.setdefault(n, len(names))
            edges, mine = set(), []
            for p in t.sharedLocal:
                row = []
                for q in val[off[p]:off[p + 1]]:
                    key = None if int(q) not in name else (min(name[int(p)], name[int(q)]), max(name[int(p)], name[int(q)]))
                    if key is not None:
                        edges.add(key)
                    row.append((int(q), key))
                mine.append(row)
            held.append(edges)
            flat.append((name, mine))
        self.nNames = len(names)
        self.gidx = [np.array([names[n[int(p)]] for p in t.sharedLocal], np.int64).reshape(-1) for (n, _), t in zip(flat, self.tables)]
        self.totalDeg = np.zeros(self.nNames, np.int64)
        self.uncounted = 0                                # row entries that are not counted: a condition on the inputs
        for r, ((_, mine), t) in enumerate(zip(flat, self.tables)):
            nP = self.subs[r].mesh.nPoints
            counted = [[q for q, key in row if key is None or not any(key in held[lo] for lo in range(r))] for row in mine]
            self.uncounted += sum(len(row) - len(c) for row, c in zip(mine, counted))
            pad = np.full((len(counted), max([1] + [len(c) for c in counted])), nP, np.int64)
            for i, c in enumerate(counted):
                pad[i, :len(c)] = c
            n = np.array([len(c) for c in counted], np.int64).reshape(-1)
            self.sharedRows.append((pad, n))
            np.add.at(self.totalDeg, self.gidx[r], n)
        self.last_scale = None

    def sweep(self, s):
        """one Jacobi sweep of 10.20 on every rank's copy of the field"""
        out, parts = [], []
        for r, sr in enumerate(s):
            ext = np.append(sr, 0.0)
            acc = np.add.accumulate(np.concatenate([np.zeros((len(sr), 1)), ext[self.rows[r]]], axis=1), axis=1)
            has = self.deg[r] > 0
            mean = np.divide(acc[np.arange(len(sr)), self.deg[r]], self.deg[r], out=np.zeros_like(sr), where=has)
            out.append(np.where(has, np.minimum(sr, 0.5 * sr + 0.5 * mean), sr))
            pad, n = self.sharedRows[r]
            pacc = np.add.accumulate(np.concatenate([np.zeros((len(n), 1)), ext[pad]], axis=1), axis=1)
            parts.append(pacc[np.arange(len(n)), n])      # the partial sum: 0.0 when no entry is counted
        total = np.zeros(self.nNames)                     # the fold over the sharers, from 0.0, in ascending rank
        for r in range(self.world):
            total[self.gidx[r]] = total[self.gidx[r]] + parts[r]
        for r, sr in enumerate(s):
            sl, g = np.asarray(self.tables[r].sharedLocal, np.int64), self.gidx[r]
            has = self.totalDeg[g] > 0
            old = sr[sl]
            mean = np.divide(total[g], self.totalDeg[g], out=np.zeros_like(old), where=has)
            out[r][sl] = np.where(has, np.minimum(old, 0.5 * old + 0.5 * mean), old)
        return out

    def _copies_equal(self, s):
        seen = np.full(self.mesh.nPoints, np.nan)
        for a, sr in zip(self.ppa, s):
            have = ~np.isnan(seen[a])
            assert np.array_equal(seen[a][have], sr[have]), "the copies of a shared point's scale differ"
            seen[a] = sr

    def step(self):
        if self.S == 0:
            cur, recs, res, frz = super().step()
            for rec in recs:
                rec.update(nScalePasses=0, nPointsScaled=0, minScale=0.0)
            return cur, recs, res, frz
        S, T, W = self.S, self.S + self.passes, self.world
        self._first = None
        x = [o.points().copy() for o in self.orcs]
        n, res, frz = self.mo.iterate(1, 0.0)
        assert n == 1
        loop = [o.points().copy() for o in self.orcs]
        cur = [p.copy() for p in loop]
        moved = [(a != b).any(axis=1) for a, b in zip(loop, x)]
        self.iteration += 1
        recs = [dict(iteration=self.iteration, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0, nNonOrthoFaces=0,
                     nSkewFaces=0) for _ in range(W)]
        nScalePasses = 0
        s = [np.ones(len(p)) for p in cur]
        for k in range(T + 1):
            ev = self.bad(cur)
            B = [e[0] for e in ev]
            if k == 0:
                for rec, (b, cnt, _) in zip(recs, ev):
                    rec["nBadCells"] = int(b.sum())
                    rec["nTangledCells"], rec["nNonOrthoFaces"], rec["nSkewFaces"] = cnt
            if sum(int(b.sum()) for b in B) == 0:          # the verdict: on the whole mesh
                break
            if k == T:
                s = [np.zeros_like(sr) for sr in s]
                for rec in recs:
                    rec["fullRevert"] = 1
            else:
                marks = np.zeros(self.mesh.nPoints, bool)   # OR over the copies of a point
                for ref, b, a in zip(self.refs, B, self.ppa):
                    m = np.zeros(len(a), bool)
                    m[ref.cpPoint[b[ref.cpCell]]] = True
                    marks[a[m]] = True
                s = [np.where(marks[a], sr * self.r if k < S else 0.0, sr) for a, sr in zip(self.ppa, s)]
                for rec in recs:
                    rec["passes"] += 1
                nScalePasses += k < S
                for _ in range(self.nSweeps):
                    s = self.sweep(s)
            self._copies_equal(s)
            cur = [np.where((sr == 1.0)[:, None], l, np.where((sr == 0.0)[:, None], x0, x0 + sr[:, None] * (l - x0))) for sr, l, x0 in zip(s, loop, x)]
        for r in range(W):
            recs[r]["nPointsReverted"] = int(((cur[r] == x[r]).all(axis=1) & moved[r] & self.master[r]).sum())
            recs[r].update(self._first[r])                 # the counts of the evaluation at k = 0
            recs[r]["nScalePasses"] = int(nScalePasses)
            recs[r]["nPointsScaled"] = int(((s[r] > 0.0) & (s[r] < 1.0) & moved[r] & self.master[r]).sum())
            recs[r]["minScale"] = float(s[r].min()) if len(s[r]) else 1.0
            self.orcs[r].set_points(cur[r])
            cur[r].setflags(write=False)
        self.last_scale = s
        return cur, recs, float(res[0]), int(frz[0])

    def run(self, nIters):
        out = super().run(nIters)
        out["recs"] = combine_scaled(out["per_rank"])
        return out


def combine_scaled(per_rank):
    """the scaled records of the undecomposed mesh: passes, fullRevert and nScalePasses are global values, minScale the minimum,
    the counts sums"""
    out = []
    for recs in zip(*per_rank):
        assert len({tuple(r[f] for f in GLOBAL_SCALED) for r in recs}) == 1, recs
        out.append(dict(**{f: recs[0][f] for f in GLOBAL_SCALED}, **{f: sum(r[f] for r in recs) for f in SUMMED_SCALED},
                        minScale=min(r["minScale"] for r in recs)))
    return out
