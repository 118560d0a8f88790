"""Probe helper of the f32 angle filters (smoothmesh_amd/csrc/kernels_filter.hpp): what the host hands the filters for a pair
of angle parameters, the inverse (the parameters that put a filter's threshold where a test wants it), the meshes of the
boundary tests and the oracle's side of them.  A plain module: tests/test_filter_probe_host.py checks it without a GPU,
tests/test_gpu_filter_boundary.py drives the engine with it.

host_thresholds mirrors makePrm and the cosSmall line of runConstraints in smoothmesh_amd/csrc/smgpu.hip and the constants of
kernels_filter.hpp; both places carry a comment that points here.  A change there is a change here."""
import concurrent.futures
import dataclasses
import math
import os

import numpy as np

K_FA_MARGIN = float(np.float32(2.0e-3))     # kFaMargin
K_EA_MARGIN = np.float32(1.0e-3)            # kEaMargin
FA_M = K_FA_MARGIN + 2.0e-5                 # makePrm: M

# the margin a GOOD verdict may have consumed, per form (the header's error budget, on cosines)
BUDGET = {"k_ea_filter_tile": 1.7e-4, "k_edge_angle_filter": 1.0e-6, "k_fa_filter_tile": 2.0e-4 + 2.0e-5, "k_fa_edges_filter": 2.0e-4 + 2.0e-5}

LADDER = [s * d for d in (2e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6) for s in (1.0, -1.0)]     # starts at +2e-3: eligibility
N_PROBES = 24
N_CANDIDATES = 48


def host_thresholds(minAngle, maxAngle):
    """degrees -> what the filters compare with: smallAngle, largeAngle (f64 radians, the exact kernels' thresholds too),
    thrEA (f32 arithmetic, as in both edge-angle filters), faCosLo / faCosHi (f32, Prm)"""
    small = math.pi * minAngle / 180.0
    large = math.pi * maxAngle / 180.0
    thrEA = np.float32(math.cos(small)) - K_EA_MARGIN
    lo = np.float32(-2.0) if small >= math.pi else np.float32(math.cos(max(small, 0.0)) - FA_M)
    hi = np.float32(2.0) if large <= 0.0 else np.float32(math.cos(min(large, math.pi)) + FA_M)
    assert thrEA.dtype == np.float32
    return dict(smallAngle=small, largeAngle=large, thrEA=float(thrEA), faCosLo=float(lo), faCosHi=float(hi))


def _deg(angle):
    return angle * 180.0 / math.pi


def degrees_for_thrEA(thr):
    """minAngle whose thrEA is `thr` up to the two f32 roundings (thr + kEaMargin <= 1)"""
    return _deg(math.acos(thr + float(K_EA_MARGIN)))


def degrees_for_faCosLo(c):
    """minAngle whose faCosLo is `c` up to the f32 rounding (c + M <= 1)"""
    return _deg(math.acos(c + FA_M))


def degrees_for_faCosHi(c):
    """maxAngle whose faCosHi is `c` up to the f32 rounding (c - M >= -1)"""
    return _deg(math.acos(c - FA_M))


def degrees_at_angle(x):
    """the three degree values around the angle x (radians): the one whose pi * d / 180 is nearest to x and its two neighbours"""
    d = _deg(x)
    near = min((np.nextafter(d, -np.inf), d, np.nextafter(d, np.inf)), key=lambda v: abs(math.pi * float(v) / 180.0 - x))
    near = float(near)
    return [float(np.nextafter(near, -np.inf)), near, float(np.nextafter(near, np.inf))]


# ---- the meshes ------------------------------------------------------------------------------------------------------------
STRETCH = (10, 30, 100, 150, 300, 1000)
SHIFT = (1e6, 1e9)
SCALE = (1e-8, 1e-15, 1e-19, 1e-20, 3e-21, 1e-21, 3e-22, 1e-23, 1e15, 1e20)
CASES = (["block"] + ["stretch%d" % a for a in STRETCH] + ["shift%g" % s for s in SHIFT] + ["scale%g" % s for s in SCALE]
         + ["cavity", "fan"])
_CELL = 1.0 / 8.0            # the block's cell size along x


def case_mesh(name):
    from smoothmesh_amd.meshgen import hex_block
    if name == "block":
        return hex_block(8, 7, 6, jitter=0.25)
    if name.startswith("stretch"):
        return hex_block(8, 7, 6, lengths=(1.0, 1.0, 1.0 / float(name[7:])), jitter=0.25)
    if name.startswith("shift"):
        m = hex_block(8, 7, 6, jitter=0.25)
        return dataclasses.replace(m, points=m.points + float(name[5:]) * _CELL)
    if name.startswith("scale"):
        m = hex_block(8, 7, 6, jitter=0.25)
        return dataclasses.replace(m, points=m.points * (float(name[5:]) / _CELL))
    if name == "cavity":
        from smoothmesh_amd.polymesh import cavity_mesh
        return cavity_mesh(8, jitter=0.2)
    if name == "fan":
        from test_gpu_edge_cases import _fan_mesh
        return _fan_mesh(20)
    raise ValueError(name)


def asserts_budget(name):
    """the cases where the budget (assertion 2) and the floor of 24 eligible elements hold unconditionally; on the stretched
    blocks they hold where the filter decides anything at all, on the scaled blocks the share decided is only recorded"""
    return not (name.startswith("stretch") or name.startswith("scale"))


# ---- the oracle's side -------------------------------------------------------------------------------------------------------
def _spread(order, n):
    """n of the sorted indices, evenly over the distribution (all of them if there are fewer)"""
    if len(order) <= n:
        return list(order)
    return [order[i] for i in np.unique(np.linspace(0, len(order) - 1, n).round().astype(int))]


class Reference:
    """the oracle (with the engine's acos: oracle_ffi.set_acos_variant("device") is the caller's business) after phaseA / phaseB on
    one mesh: the exact values the filters estimate, and the decisions for any pair of thresholds"""

    def __init__(self, mesh, oracle_lib):
        from smoothmesh_amd import default_params
        self.mesh = mesh
        self.o = oracle_lib.Oracle(mesh)
        self.base = default_params(self.o.mesh_stats()[0])
        self.o.set_params(self.base)
        self.o.phaseA(); self.o.phaseB()
        self.eaMinN = self.o.field("eaMinN")
        self.edgeMin, self.edgeMax = self.o.field("edgeMinAngle"), self.o.field("edgeMaxAngle")
        self.frozenLen = self.o.field("frozenAfterEdgeLen").astype(bool)
        self.edges = self.o.addressing("edges")[1]
        self.cosEa = np.cos(self.eaMinN)
        self.cosMin, self.cosMax = np.cos(self.edgeMin), np.cos(self.edgeMax)
        # edges for which the exact evaluator has no angle: its sentinels (no cell gave one), or not a number
        self.noAngle = ~np.isfinite(self.edgeMin) | ~np.isfinite(self.edgeMax) | (self.edgeMin >= 2.0 * math.pi) | (self.edgeMax <= 0.0)
        self._dec = {}
        self._clones = []

    def params(self, minAngle, maxAngle):
        return dataclasses.replace(self.base, minAngle=minAngle, maxAngle=maxAngle)

    def _decide(self, o, minAngle, maxAngle):
        o.set_params(self.params(minAngle, maxAngle))
        o.phaseA(); o.phaseB()         # (phaseA clears the frozen flags)
        th = host_thresholds(minAngle, maxAngle)
        act = ~((o.field("pointMinAngle") > th["smallAngle"]) & (o.field("pointMaxAngle") < th["largeAngle"]))
        return o.field("frozenAfterFaceAngle").astype(bool), act

    def decisions(self, minAngle, maxAngle):
        """(frozenAfterFaceAngle, active set of the face-angle walk) for these thresholds"""
        key = (minAngle, maxAngle)
        if key not in self._dec:
            self._dec[key] = self._decide(self.o, minAngle, maxAngle)
        return self._dec[key]

    def prefetch(self, pairs):
        """the decisions for many threshold pairs at once: one oracle per worker thread on the same mesh (a Domain shares nothing
        with another; the library calls release the interpreter lock) -- the oracle's pass is most of a probe's cost on the larger meshes"""
        todo = [k for k in dict.fromkeys(pairs) if k not in self._dec]
        if len(todo) < 32 or self.mesh.nPoints < 1000:
            return
        nw = max(1, min(16, os.cpu_count() or 1))
        while len(self._clones) < nw:
            self._clones.append(type(self.o)(self.mesh))

        def work(w):
            return [(k, self._decide(self._clones[w], *k)) for k in todo[w::nw]]
        with concurrent.futures.ThreadPoolExecutor(nw) as ex:
            for part in ex.map(work, range(nw)):
                self._dec.update(part)

    # candidates: (element id, point whose mark shows the element's verdict)
    def ea_candidates(self, n=N_CANDIDATES):
        ok = np.flatnonzero(~self.frozenLen & (self.cosEa < 0.99))
        return [(int(p), int(p)) for p in _spread(ok[np.argsort(self.eaMinN[ok], kind="stable")], n)]

    def _point_extreme_edges(self, side):
        """per point the edge that holds its smallest (largest) face angle: only that edge's verdict can be read off the point's mark,
        since every other edge of the point is further from the threshold on this side"""
        val = np.where(self.noAngle, np.inf, self.edgeMin) if side == "min" else np.where(self.noAngle, -np.inf, -self.edgeMax)
        best = {}
        for e, (a, b) in enumerate(self.edges):
            for p in (int(a), int(b)):
                if p not in best or val[e] < val[best[p]]:
                    best[p] = e
        seen, out = set(), []
        for p, e in sorted(best.items()):
            if e not in seen and np.isfinite(val[e]):
                seen.add(e)
                out.append((int(e), p))
        return out

    def fa_candidates(self, side, n=N_CANDIDATES):
        """edges for the ladder: |cos| < 0.99, so that every rung is a threshold the host can be asked for"""
        c = self.cosMin if side == "min" else self.cosMax
        ang = self.edgeMin if side == "min" else self.edgeMax
        pairs = [(e, p) for e, p in self._point_extreme_edges(side) if abs(c[e]) < 0.99 and ang[e] < math.pi]
        pairs.sort(key=lambda ep: (ang[ep[0]], ep[0]))
        return _spread(pairs, n)

    def near_pi_edges(self, n=8):
        """edges whose largest angle lies in (pi - 0.1, pi), and above pi"""
        ok = ~self.noAngle
        below = np.flatnonzero(ok & (self.edgeMax > math.pi - 0.1) & (self.edgeMax < math.pi))
        above = np.flatnonzero(ok & (self.edgeMax > math.pi))
        return below, above, _spread(below[np.argsort(self.edgeMax[below], kind="stable")], n), _spread(above[np.argsort(self.edgeMax[above], kind="stable")], n)
