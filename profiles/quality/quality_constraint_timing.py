"""Kernel time of the quality constraint's launches (smgpu_set_quality_constraint) beside its yardsticks, and what the
constraint costs per iteration.

    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: one engine on
               cavity_mesh(N) with the reference's constraints off and a trace at every iteration.  Four iterations with the
               tangle constraint on, then four with the quality constraint on at its default limits: k_tangle_tile,
               k_quality_geom_tile and k_quality_faces (the yardsticks, the parent's code paths) and k_qc_tile, k_qc_faces<false>,
               k_qc_cells, k_qc_verdict run on the same mesh in the same process.
    overhead:  no profiler: ms per iteration of iterate(STEPS) with the reference's constraints on (configs[3]), in alternating
               off / on pairs on one engine with the order swapped in every second pair, the number of iterations with a bad element printed (0 on this mesh): the quality
               constraint at its defaults, then the tangle constraint, then the quality constraint with passes = 0 (one
               evaluation and no queued no-op pass: the difference to the first is the no-op cost of two passes)."""
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
    e.set_tangle_constraint()
    n = e.iterate(4, 0.0)[0]
    recs = e.tangle_records()
    print(f"tangle constraint: {n} iterations, exempt {e.tangle_state().nExemptCells}, records {[(r.nBadCells, r.passes) for r in recs]}", flush=True)
    assert n == 4
    e.clear_tangle_constraint()
    e.set_quality_constraint()
    st = e.quality_constraint_state()
    n = e.iterate(4, 0.0)[0]
    recs = e.quality_constraint_records()
    print(f"quality constraint: {n} iterations, exempt {st.nExemptCells} cells {st.nExemptFaces} faces, records "
          f"{[(r.nBadCells, r.nTangledCells, r.nNonOrthoFaces, r.nSkewFaces, r.passes) for r in recs]}", flush=True)
    assert n == 4 and len(e.quality_trace()) == 8
else:
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    forms = [("quality constraint", lambda: e.set_quality_constraint(), e.quality_constraint_records, e.clear_quality_constraint),
             ("tangle constraint", lambda: e.set_tangle_constraint(), e.tangle_records, e.clear_tangle_constraint),
             ("quality constraint, passes = 0", lambda: e.set_quality_constraint(passes=0), e.quality_constraint_records, e.clear_quality_constraint)]
    for name, enable, records, clear in forms:
        for pair in range(2):
            ms = {}
            for on in ((False, True) if pair % 2 == 0 else (True, False)):   # (the mesh smooths on: the later run of a pair has less to do)
                if on:
                    enable()
                    e.check_error()
                t = time.time()
                n = e.iterate(STEPS, 0.0)[0]
                ms[on] = 1e3 * (time.time() - t) / n
                assert n == STEPS
                if on:
                    recs = records()
                    assert len(recs) == STEPS
                    fired = sum(1 for r in recs if r.nBadCells)      # (0: the figure is the cost with nothing bad)
                    clear()
            print(f"{name}, pair {pair}: {ms[False]:.4f} ms per iteration without, {ms[True]:.4f} with it "
                  f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {1e3 * (ms[True] - ms[False]):+.1f} us); {fired} iterations had bad cells", flush=True)
