"""Kernel time of the motion criteria (smgpu_mesh_quality_motion) next to the geometry checks' face pass, on the
10 M-cell polyhedral mesh of configs[3] (cavity_mesh(215)).  Run under `rocprofv3 --kernel-trace --stats`
(profiles/quality/README.md): three geometry reports, then three motion reports, in one process.  The first report of each kind
allocates its memory (and the very first derives owner / neighbour: k_quality_owners, once per engine)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces ({m.nInternalFaces} internal), {m.nPoints} points, "
      f"{len(m.facePoints)} face vertices ({time.time() - t:.1f} s)", flush=True)
e = SmoothEngine(m)
for i in range(3):
    t = time.time()
    g = e.mesh_quality_geometry()
    print(f"geometry report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
for i in range(3):
    t = time.time()
    q = e.mesh_quality_motion()
    print(f"motion report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
print(q, flush=True)
