"""Kernel time of one decomposed mesh quality report (smoothmesh_amd/quality.py) on configs[4]'s split of the 10 M-cell polyhedral
mesh: cavity_mesh(215) cut 2 x 2 x 2 (cavity_subdomain), eight plain engines on one device.  Run under
`rocprofv3 --kernel-trace --stats` (profiles/quality/README.md): three reports; the first one allocates the report's memory,
uploads the coupling and derives owner / neighbour (k_quality_owners, once per engine)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402
from smoothmesh_amd import SmoothEngine  # noqa: E402
from smoothmesh_amd.polymesh import cavity_subdomain  # noqa: E402
from smoothmesh_amd.quality import local_quality  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
t = time.time()
subs = [cavity_subdomain(N, (2, 2, 2), r) for r in range(8)]
print(f"cavity_subdomain({N}, 2x2x2): {sum(s.mesh.nCells for s in subs)} cells, "
      f"{sum(p.nFaces for s in subs for p in s.mesh.patches if p.type == 'processor')} processor faces ({time.time() - t:.1f} s)", flush=True)
engines = [SmoothEngine(s.mesh) for s in subs]
for e in engines:
    e.set_device_share(len(engines))
for i in range(3):
    t = time.time()
    q = local_quality(engines, subs, torch.device("cuda", 0), {})
    print(f"report {i}: {1e3 * (time.time() - t):.2f} ms wall (8 packs, the copies, 8 reports, the combine): {q}", flush=True)
