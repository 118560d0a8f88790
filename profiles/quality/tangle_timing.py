"""Kernel time of the tangle constraint's launches (smgpu_set_tangle_constraint) beside the fused trace's and the
loop's geometry tile, and what the constraint costs per iteration.

    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: one engine on
               cavity_mesh(N) with the reference's constraints off, the tangle constraint on and a trace at every iteration, a
               few iterations: k_tangle_tile, k_quality_geom_tile and k_geom_tile run on the same points in the same process.
               Then, to time the apply pass against its 72 P + P bytes, one full revert: passes = 0 and one point folded through
               its cells before the iteration.
    overhead:  no profiler: ms per iteration of iterate(STEPS) with the reference's constraints on (configs[3]), the tangle
               constraint off (the parent's behaviour) against on, with no cell ever bad, in alternating pairs on one engine
               with the order swapped.
    hex:       the same pairs on the 100^3 hex block with the reference's constraints off (an 85 us iteration: the queued no-op
               launches weigh most there).
    hexkernels: under the profiler again: 20 iterations of that hex run with the constraint on, for the sum of its kernel times."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.meshgen import hex_block  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
MODE = sys.argv[2] if len(sys.argv) > 2 else "kernels"
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
t = time.time()
m = hex_block(N) if MODE.startswith("hex") else cavity_mesh(N)
print(f"{'hex_block' if MODE.startswith('hex') else 'cavity_mesh'}({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)

if MODE == "kernels":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    e.set_tangle_constraint()
    e.set_quality_trace(1)
    n = e.iterate(4, 0.0)[0]
    recs = e.tangle_records()
    print(f"{n} iterations, exempt {e.tangle_state().nExemptCells}, records {[(r.nBadCells, r.passes, r.fullRevert, r.nPointsReverted) for r in recs]}", flush=True)
    assert n == 4 and len(e.quality_trace()) == 4
    # a full revert, forced: enable with passes = 0 on the smoothed points (no exempt cells), then fold one interior point through
    # its cells; the next iteration finds them bad and puts every point back
    pts = e.get_points()
    inner = np.flatnonzero(m.find_internal_points())
    p = int(inner[len(inner) // 2])
    e.clear_tangle_constraint()
    e.set_quality_trace(0)
    e.set_tangle_constraint(0)
    moved = pts.copy()
    moved[p] += 1.5 / N                                       # past its neighbours: its cells fold, none was exempt
    e.set_points(moved)
    n = e.iterate(1, 0.0)[0]
    recs = e.tangle_records()
    print(f"forced: {[(r.nBadCells, r.passes, r.fullRevert, r.nPointsReverted) for r in recs]}; a full revert reads x, x' and the marks and writes "
          f"x': {73 * m.nPoints / 1e9:.3f} GB", flush=True)
elif MODE == "hexkernels":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    e.set_tangle_constraint()
    n = e.iterate(20, 0.0)[0]
    assert n == 20 and not any(r.nBadCells for r in e.tangle_records())
else:
    e = SmoothEngine(m)
    over = dict(edgeAngleConstraint=False, faceAngleConstraint=False) if MODE == "hex" else {}
    e.set_params(default_params(e.mesh_stats()[0], **over))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    for pair in range(4):
        ms = {}
        for on in ((False, True) if pair % 2 == 0 else (True, False)):   # (the mesh smooths on: the later run of a pair has less to do)
            if on:
                e.set_tangle_constraint()
                e.check_error()
            t = time.time()
            n = e.iterate(STEPS, 0.0)[0]
            ms[on] = 1e3 * (time.time() - t) / n
            assert n == STEPS
            if on:
                recs = e.tangle_records()
                assert len(recs) == STEPS and not any(r.nBadCells for r in recs)
                e.clear_tangle_constraint()
        print(f"pair {pair}: {ms[False]:.4f} ms per iteration without the constraint, {ms[True]:.4f} with it "
              f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {1e3 * (ms[True] - ms[False]):+.1f} us)", flush=True)
