"""Kernel time of the quality guard's two launches (smgpu_set_quality_guard) beside the fused trace's, and what
an armed run costs, on the 10 M-cell polyhedral mesh of configs[3] (cavity_mesh(215)).

    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters: one engine with the
               constraints off, a trace at every iteration and the guard armed, three iterations: three verdicts and three
               snapshots behind the fused trace's launches of the same process, and the snapshot of the arming.
    overhead:  no profiler: ms per iteration of iterate(STEPS) with the constraints on (configs[3]) at interval 10, trace only
               (the parent's behaviour) against trace plus guard, in alternating pairs on one engine with the order swapped."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
MODE = sys.argv[2] if len(sys.argv) > 2 else "kernels"
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)

if MODE == "kernels":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    e.set_quality_trace(1)
    e.set_quality_guard()
    n = e.iterate(3, 0.0)[0]
    g = e.quality_guard()
    print(f"{n} iterations, guard: armed {g.armed} tripped {g.tripped} snapshot {g.snapshotIteration}", flush=True)
    print(f"snapshot: {48 * m.nPoints / 1e9:.3f} GB read + written per copy", flush=True)
    assert n == 3 and len(e.quality_trace()) == 3
else:
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    for pair in range(4):
        ms = {}
        for armed in ((False, True) if pair % 2 == 0 else (True, False)):   # (the mesh smooths on: the later run of a pair has less to do)
            e.set_quality_trace(10)
            if armed:
                e.set_quality_guard()
                e.check_error()
            t = time.time()
            n = e.iterate(STEPS, 0.0)[0]
            ms[armed] = 1e3 * (time.time() - t) / n
            assert n == STEPS and len(e.quality_trace()) == STEPS // 10
            if armed:
                g = e.quality_guard()
                assert g.armed and not g.tripped and g.snapshotIteration == STEPS, g
                e.set_quality_guard(None)
        print(f"pair {pair}: {ms[False]:.4f} ms per iteration with the trace alone, {ms[True]:.4f} with the guard armed "
              f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {1e3 * (ms[True] - ms[False]):+.1f} us)", flush=True)
