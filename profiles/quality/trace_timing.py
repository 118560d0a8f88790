"""Kernel time of one traced iteration's extra launches (smgpu_set_quality_trace) on the 10 M-cell polyhedral mesh
of configs[3] (cavity_mesh(215)), beside the report's (smgpu_mesh_quality) in the same run.

    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters: three reports, then three
               traced iterations with the fused tile kernel, then three with the fallback launches (SMGPU_QUALITY_TRACE_FUSED=0,
               a second engine).  The loop runs with the constraints off: its own kernels are not what is measured.
    overhead:  no profiler: ms per iteration of iterate(STEPS) with the constraints on (configs[3]) and a trace every 10th
               iteration against none, in alternating pairs on one engine."""
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
    for i in range(3):
        t = time.time()
        q = e.mesh_quality()
        print(f"report {i}: {1e3 * (time.time() - t):.2f} ms wall (with the copy and synchronise)", flush=True)
    e.set_quality_trace(1)
    e.iterate(3, 0.0)
    fused = e.quality_trace()
    print("fused:", fused[-1], flush=True)
    os.environ["SMGPU_QUALITY_TRACE_FUSED"] = "0"
    f = SmoothEngine(m)
    f.set_params(default_params(f.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    f.set_quality_trace(1)
    f.iterate(3, 0.0)
    fallback = f.quality_trace()
    print("fused == fallback:", fused == fallback, flush=True)
    assert fused == fallback and len(fused) == 3
else:
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    for pair in range(3):
        ms = {}
        for interval in ((0, 10) if pair % 2 == 0 else (10, 0)):     # (the mesh smooths on: the later run of a pair has less to do)
            e.set_quality_trace(interval)
            t = time.time()
            n = e.iterate(STEPS, 0.0)[0]
            ms[interval] = 1e3 * (time.time() - t) / n
            assert len(e.quality_trace()) == (STEPS // 10 if interval else 0)
        print(f"pair {pair}: {ms[0]:.4f} ms per iteration without, {ms[10]:.4f} with a trace every 10th "
              f"({100 * (ms[10] / ms[0] - 1):+.2f} %)", flush=True)
