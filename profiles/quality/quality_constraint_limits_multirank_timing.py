"""What the quality constraint's six further limits cost per iteration on a decomposed mesh
(smgpu_set_quality_constraint_limits_coupled), against the parent commit's coupled quality constraint (10.15), and
the kernel times of its face pass beside the serial twin's.

One leg per process, so that the reference leg can be another build: SMOOTHMESH_TREE names the checkout whose smoothmesh_amd
package (and libsmgpu.so) the process loads -- the parent commit's for `parent`, this one's for `none` and `all`.  The caller
alternates the legs in pairs and swaps the order in every second pair.

    dist N STEPS LEG:   one rank (world 1, gloo) of a hex N^3 block through DistributedSmoother, the reference's constraints off:
                        ms per iteration of iterate(STEPS, 0.0), no element ever bad, and the time spent inside the three pass
                        calls.  LEG: parent (set_quality_constraint, which the parent's build has) | none
                        (set_quality_constraint_limits, no new limit on) | all (all six on, at limits nothing reaches).
    local STEPS LEG:    the same through LocalMultiSmoother on the two halves, 100 x 100 x 50 cells each, of a hex block.
    kernels:            under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: those
                        halves with all nine criteria on for a few iterations, and then the serial constraint under the same
                        limits on one half as a mesh of its own, for k_qc_faces_more<..., false> beside k_qc_faces_more<..., true> and
                        k_qc_cells_more<..., false> beside k_qc_cells_more<..., true>."""
import os
import socket
import sys
import time

sys.path.insert(0, os.environ.get("SMOOTHMESH_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother  # noqa: E402
from smoothmesh_amd.meshgen import hex_subdomain  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "dist"
NEVER = dict(maxNonOrtho=179.9, maxInternalSkewness=1e9, maxBoundarySkewness=1e9)     # every old criterion on, no face ever over a limit
NEVER_MORE = dict(minTetQuality=-1e9, minTwist=-0.999, minTriangleTwist=-0.999, minFaceWeight=1e-9, minVolRatio=1e-9, minDeterminant=1e-12)
CALLS = ("quality_constraint_pass_begin", "quality_constraint_pass_faces", "quality_constraint_pass_end")


def leg_run(sm, engines, steps, leg):
    sm.iterate(20, 0.0)                                          # warm-up: allocations
    if leg == "parent":
        sm.set_quality_constraint(**NEVER)
    elif leg == "none":
        sm.set_quality_constraint_limits(**NEVER)
    else:
        sm.set_quality_constraint_limits(**NEVER, **NEVER_MORE)
    spent = {}
    for name in CALLS:
        spent[name] = 0.0
        for eng in engines:
            def timed(*a, _f=getattr(eng, name), _n=name):
                t = time.perf_counter()
                r = _f(*a)
                spent[_n] += time.perf_counter() - t
                return r
            setattr(eng, name, timed)
    sm.iterate(10, 0.0)
    for k in spent:
        spent[k] = 0.0
    t = time.time()
    n = sm.iterate(steps, 0.0)[0]
    ms = 1e3 * (time.time() - t) / n
    assert n == steps
    recs = sm.quality_constraint_records()
    assert len(recs) == steps + 10 and not any(r.nBadCells for r in recs)
    inside = ", ".join(f"{1e6 * v / steps:.1f} us inside {k}" for k, v in spent.items())
    print(f"{MODE} {leg}: {ms:.4f} ms per iteration ({inside})", flush=True)


def halves(jitter=0.0):
    t = time.time()
    subs = [hex_subdomain((100, 100, 50), (2, 1, 1), r, jitter=jitter, seed=5) for r in range(2)]
    print(f"two sub-domains of {subs[0].mesh.nCells} cells, {subs[0].mesh.nPoints} points ({time.time() - t:.1f} s)", flush=True)
    return subs


if MODE == "dist":
    import torch.distributed as dist
    N, STEPS, LEG = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    sub = hex_subdomain((N, N, N), (1, 1, 1), 0, jitter=0.0, seed=5)
    ds = DistributedSmoother(sub, device=0, overlap=False)
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    leg_run(ds, [ds.engine], STEPS, LEG)
    ds.close()
    dist.destroy_process_group()
elif MODE == "local":
    STEPS, LEG = int(sys.argv[2]), sys.argv[3]
    ms = LocalMultiSmoother(halves(), device=0, overlap=False)
    ms.set_params(default_params(ms.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    leg_run(ms, [st.eng for st in ms.states], STEPS, LEG)
else:
    subs = halves()
    ms = LocalMultiSmoother(subs, device=0, overlap=False)
    prm = default_params(ms.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False)
    ms.set_params(prm)
    ms.set_quality_constraint_limits(passes=1, **NEVER, **NEVER_MORE)
    assert ms.iterate(3, 0.0)[0] == 3
    print(f"coupled halves: records {[(r.nBadCells, r.passes) for r in ms.quality_constraint_records()]}", flush=True)
    # the serial constraint on one half, its processor patch an ordinary boundary: the serial twins on the same number of faces
    e = SmoothEngine(subs[0].mesh, device=0)
    e.set_params(prm)
    e.set_quality_constraint(passes=1, **NEVER, **NEVER_MORE)
    assert e.iterate(3, 0.0)[0] == 3
    print(f"serial half: records {[(r.nBadCells, r.passes) for r in e.quality_constraint_records()]}", flush=True)
