"""Kernel time of the decomposed -allGeometry and motion reports (smoothmesh_amd/quality.py) beside the serial
ones, in one run: cavity_mesh(215) cut 2 x 2 x 2 (cavity_subdomain, configs[4]'s layout), eight plain engines on one device, then
the undecomposed cavity_mesh(215) on one engine.  Run under `rocprofv3 --kernel-trace --stats` with no counters
(profiles/quality/README.md): three reports of each kind; the first one of each allocates its memory (and the very first of an
engine uploads the coupling and derives owner / neighbour: k_quality_owners, once per engine)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402
from smoothmesh_amd import SmoothEngine  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh, cavity_subdomain  # noqa: E402
from smoothmesh_amd.quality import local_quality_geometry, local_quality_motion  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
t = time.time()
subs = [cavity_subdomain(N, (2, 2, 2), r) for r in range(8)]
print(f"cavity_subdomain({N}, 2x2x2): {sum(s.mesh.nCells for s in subs)} cells, "
      f"{sum(p.nFaces for s in subs for p in s.mesh.patches if p.type == 'processor')} processor faces ({time.time() - t:.1f} s)", flush=True)
engines = [SmoothEngine(s.mesh) for s in subs]
for e in engines:
    e.set_device_share(len(engines))
dev = torch.device("cuda", 0)
for i in range(3):
    t = time.time()
    g = local_quality_geometry(engines, subs, dev, {})
    print(f"decomposed geometry report {i}: {1e3 * (time.time() - t):.2f} ms wall (8 packs, 8 volume packs, the copies, 8 reports, "
          f"the combine)", flush=True)
for i in range(3):
    t = time.time()
    q = local_quality_motion(engines, subs, dev, {})
    print(f"decomposed motion report {i}: {1e3 * (time.time() - t):.2f} ms wall (8 packs, the copies, 8 reports, the combine)", flush=True)
print(g, q, sep="\n", flush=True)
for e in engines:
    e.close()
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces ({m.nInternalFaces} internal) ({time.time() - t:.1f} s)", flush=True)
e = SmoothEngine(m)
for i in range(3):
    t = time.time()
    sg = e.mesh_quality_geometry()
    print(f"serial geometry report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
for i in range(3):
    t = time.time()
    sq = e.mesh_quality_motion()
    print(f"serial motion report {i}: {1e3 * (time.time() - t):.2f} ms wall", flush=True)
print(sg, sq, sep="\n", flush=True)
