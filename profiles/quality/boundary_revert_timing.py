"""What the tangle constraint costs per iteration on an engine with boundary point smoothing (smgpu_set_boundary_revert, DESIGN.md
10.21), for the record: workload hex100B of bench.py -- hex_block(N, jitter 0.2) with all six sides smoothed onto the block's own
surface and its twelve feature edges, the reference's constraints off -- ms per iteration of iterate(STEPS) with the constraint off
against on, no cell ever bad, in alternating pairs on one engine with the order swapped in every second pair.  No profiler.

    python profiles/quality/boundary_revert_timing.py [N = 100] [STEPS = 200]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import BoundaryParams, SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.meshgen import hex_block  # noqa: E402
from smoothmesh_amd.surfgen import box_feature_edges, box_surface  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
t = time.time()
m = hex_block(N, jitter=0.2, seed=12345)
print(f"hex_block({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)
e = SmoothEngine(m)
prm = default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False)
e.set_params(prm)
info = e.set_boundary_smoothing(BoundaryParams(initEdges=box_feature_edges(N), targetSurfaces=box_surface(max(N // 2, 1))), prm.minEdgeLength)
assert info["enabled"]
e.set_boundary_revert()
e.iterate(20, 0.0)                                           # warm-up: allocations
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
