"""Kernel time of the quality sets (smgpu_quality_sets) next to the report, on the 10 M-cell polyhedral mesh of
configs[3] (cavity_mesh(215)).  Run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md): three reports, three
sets calls with the default thresholds, then three with every face in skewFaces (skewThreshold -1).  The first report allocates
the report's memory and derives owner / neighbour (k_quality_owners, once per engine)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)
e = SmoothEngine(m)
for i in range(3):
    t = time.time()
    q = e.mesh_quality()
    print(f"report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
for label, thr in (("default", {}), ("all faces skew", dict(skewThreshold=-1.0))):
    for i in range(3):
        t = time.time()
        s = e.quality_sets(**thr)
        print(f"sets ({label}) {i}: {1e3 * (time.time() - t):.2f} ms wall (with the copies and the allocations): "
              f"{ {k: len(v) for k, v in s.items()} }", flush=True)
