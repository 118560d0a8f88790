"""Kernel time of the sets of the -allGeometry checks and of the motion criteria (smgpu_quality_geometry_sets /
smgpu_quality_motion_sets) next to their reports, on the 10 M-cell polyhedral mesh of configs[3]
(cavity_mesh(215)).  Run under `rocprofv3 --kernel-trace --stats` in a run of its own, no counters
(profiles/quality/README.md).  Per report kind: three report calls and three sets calls; `default` runs them at the default
thresholds, `every` with thresholds that put every eligible face and cell in a set.  One mode per run, so that the per-kernel
means of the stats file belong to one set of thresholds:
    python profiles/quality/more_sets_timing.py [N] [default|every]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
mode = sys.argv[2] if len(sys.argv) > 2 else "default"
EVERY = dict(geometry=dict(flatnessThreshold=2.0, weightThreshold=1.0, volRatioThreshold=2.0, determinantThreshold=1e30),
             motion=dict(tetThreshold=2.0, twistThreshold=2.0, triangleTwistThreshold=2.0))
thr = EVERY if mode == "every" else dict(geometry={}, motion={})
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s); thresholds: {mode}", flush=True)
e = SmoothEngine(m)
for kind, report, sets in (("geometry", e.mesh_quality_geometry, e.quality_geometry_sets), ("motion", e.mesh_quality_motion, e.quality_motion_sets)):
    for i in range(3):
        t = time.time()
        report(**thr[kind])
        print(f"{kind} report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
    for i in range(3):
        t = time.time()
        s = sets(**thr[kind])
        print(f"{kind} sets {i}: {1e3 * (time.time() - t):.2f} ms wall (with the copies and the allocations): "
              f"{ {k: len(v) for k, v in s.items()} }", flush=True)
