"""Kernel time of the launches that the quality constraint's last four limits change (smgpu_set_quality_constraint_limits_all,
DESIGN.md 10.18) beside their yardsticks, and what they cost per iteration.

    kernels:   run under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: one engine on
               cavity_mesh(N) with the reference's constraints off.  The -allGeometry report once (k_quality_geom_faces, whose
               vertex walk the face kernel repeats, and k_quality_geom_cells), four iterations with the six limits of 10.16 on
               (k_qc_faces_more<true, true, false, 0>, k_qc_cells_more<true, false, false>: the yardsticks), four with the three
               new face criteria alone (k_qc_faces_more<false, false, false, 2>), four with all thirteen on
               (k_qc_faces_more<true, true, false, 2>, k_qc_cells_more<true, false, true>).
    overhead:  no profiler: ms per iteration of iterate(STEPS) with the reference's constraints on (configs[3]), in alternating
               pairs on one engine, the order swapped in every second pair.  The "off" run of a pair is the constraint with the
               nine limits through smgpu_set_quality_constraint_limits, whose kernels are the parent commit's register for register
               (scripts/kernel_resources.sh); the "on" run is (a) the new entry with the four off, whose launches are that
               entry's, then (b) all thirteen on, at limits nothing on this mesh reaches."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.engine import QUALITY_CONSTRAINT_LIMITS_ALL_OFF  # noqa: E402
from smoothmesh_amd.polymesh import cavity_mesh  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 215
MODE = sys.argv[2] if len(sys.argv) > 2 else "kernels"
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 200
# on, and out of reach: tet quality >= -1 by its normalisation, the twists are cosines, the others are >= 0; sin(90 degrees) is 1,
# which only a convex right angle's sine reaches
SIX_ON = dict(minTetQuality=-1e9, minTwist=-0.999999, minTriangleTwist=-0.999999, minFaceWeight=1e-12, minVolRatio=1e-12, minDeterminant=1e-12)
FACES_ON = dict(maxConcave=90.0, minFlatness=1e-12, minArea=1e-300)
FOUR_ON = dict(FACES_ON, minVol=1e-300)
t = time.time()
m = cavity_mesh(N)
print(f"cavity_mesh({N}): {m.nCells} cells, {m.nFaces} faces, {m.nPoints} points ({time.time() - t:.1f} s)", flush=True)

if MODE == "kernels":
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False))
    e.mesh_quality_geometry()
    for name, lim in (("the six of 10.16", SIX_ON), ("the three new face criteria", FACES_ON), ("all thirteen", dict(SIX_ON, **FOUR_ON))):
        e.set_quality_constraint(**lim)
        st = e.quality_constraint_state()
        assert e.iterate(4, 0.0)[0] == 4
        print(f"{name}: exempt {st.nExemptCells} cells {st.nExemptFaces} faces {st.nExemptDeterminantCells} determinant cells "
              f"{st.nExemptVolumeCells} volume cells, records {[(r.nBadCells, r.passes) for r in e.quality_constraint_records()]}", flush=True)
else:
    e = SmoothEngine(m)
    e.set_params(default_params(e.mesh_stats()[0]))
    e.iterate(20, 0.0)                                       # warm-up: allocations, the walk's replay form
    for name, off, on_ in (("(a) new entry, the four off", SIX_ON, dict(SIX_ON, **QUALITY_CONSTRAINT_LIMITS_ALL_OFF)),
                           ("(b) all thirteen on", SIX_ON, dict(SIX_ON, **FOUR_ON))):
        for pair in range(2):
            ms = {}
            for on in ((False, True) if pair % 2 == 0 else (True, False)):   # (the mesh smooths on: the later run of a pair has less to do)
                e.set_quality_constraint(**(on_ if on else off))
                e.check_error()
                t = time.time()
                n = e.iterate(STEPS, 0.0)[0]
                ms[on] = 1e3 * (time.time() - t) / n
                recs = e.quality_constraint_records()
                assert n == STEPS and len(recs) == STEPS
                if on:
                    fired = sum(1 for r in recs if r.nBadCells)      # (0: the figure is the cost with nothing bad)
                e.clear_quality_constraint()
            print(f"{name}, pair {pair}: {ms[False]:.4f} ms per iteration under the nine limits, {ms[True]:.4f} under this form "
                  f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {1e3 * (ms[True] - ms[False]):+.1f} us); {fired} iterations had bad cells", flush=True)
