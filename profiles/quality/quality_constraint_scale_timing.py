"""What the quality constraint's scaling passes (smgpu_set_quality_constraint_scaling) cost: per iteration with
nothing bad, and per kernel in a pass that scales.

    overhead:  no profiler: ms per iteration of iterate(STEPS) on cavity_mesh(N) with the quality constraint on at its default
               limits, scaling off (the parent's behaviour) against scalePasses = 2, nSmoothScale = 4, with no cell ever bad, in
               alternating pairs on one engine with the order swapped in every second pair.
    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: the same
               engine with the reference's constraints off, a trace and an armed guard for two iterations (k_quality_guard_snapshot
               on the same points, for the bandwidth of the L copy), then one iteration with one interior point folded through
               its cells before it, as tangle_timing.py forces its full revert: every scaling, reverting and the full pass runs,
               and k_qs_keep, k_qs_mark, k_qs_sweep and k_qs_apply show in the statistics with their call counts.
    noop:      under the profiler again: 20 iterations of the overhead run with the scaling on and nothing bad, for the time of
               every gated launch that returns on the clean word."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.engine import HostTopology  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
MODE = sys.argv[2] if len(sys.argv) > 2 else "overhead"
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)

if MODE == "kernels":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    e.set_quality_trace(1)
    e.set_quality_guard()
    assert e.iterate(2, 0.0)[0] == 2
    e.set_quality_trace(0)
    pts = e.get_points()
    inner = np.flatnonzero(m.find_internal_points())
    p = int(inner[len(inner) // 2])
    e.set_quality_constraint(scalePasses=2, errorReduction=0.75, nSmoothScale=4)      # on the smoothed points: their bad elements are exempt
    moved = pts.copy()
    moved[p] += 1.5 / N                                       # past its neighbours: its cells fold, none was exempt
    e.set_points(moved)
    n = e.iterate(1, 0.0)[0]
    recs = e.quality_constraint_records_scaled()
    P = m.nPoints
    nnz = len(HostTopology(m).addressing("pointPoints")[1])
    print(f"forced: {[(r.nBadCells, r.passes, r.nScalePasses, r.fullRevert, r.nPointsReverted, r.nPointsScaled, r.minScale) for r in recs]}", flush=True)
    print(f"P = {P}, nnz(pointPoints) = {nnz}; the L copy moves 48 P = {48 * P / 1e9:.4f} GB (+ 8 P of scale written: {8 * P / 1e9:.4f} GB); one sweep reads "
          f"8 P + 4 P + 4 nnz + 8 nnz gathered = {(12 * P + 12 * nnz) / 1e9:.4f} GB and writes 8 P = {8 * P / 1e9:.4f} GB; the full-revert apply reads "
          f"8 P + 48 P and writes 24 P = {80 * P / 1e9:.4f} GB", flush=True)
elif MODE == "noop":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.set_quality_constraint(scalePasses=2, nSmoothScale=4)
    n = e.iterate(20, 0.0)[0]
    assert n == 20 and not any(r.nBadCells for r in e.quality_constraint_records_scaled())
else:
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    diffs = []
    for pair in range(4):
        ms = {}
        for on in ((False, True) if pair % 2 == 0 else (True, False)):   # (the mesh smooths on: the later run of a pair has less to do)
            e.set_quality_constraint(**(dict(scalePasses=2, nSmoothScale=4) if on else {}))
            e.check_error()
            t = time.time()
            n = e.iterate(STEPS, 0.0)[0]
            ms[on] = 1e3 * (time.time() - t) / n
            assert n == STEPS
            recs = e.quality_constraint_records_scaled()
            assert len(recs) == STEPS and not any(r.nBadCells for r in recs)
            e.clear_quality_constraint()
        diffs.append(1e3 * (ms[True] - ms[False]))
        print(f"pair {pair}: {ms[False]:.4f} ms per iteration with the constraint and scaling off, {ms[True]:.4f} with scalePasses 2, nSmoothScale 4 "
              f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {diffs[-1]:+.1f} us)", flush=True)
    print(f"difference: mean {np.mean(diffs):+.1f} us, spread {min(diffs):+.1f} .. {max(diffs):+.1f} us per iteration", flush=True)
