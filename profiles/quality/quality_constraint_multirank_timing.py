"""What the quality constraint costs per iteration on a decomposed mesh (smgpu_set_quality_constraint_coupled), against
the run without it and against the coupled tangle constraint (10.13), and the kernel times of its face pass.

One leg per process, so that the "off" leg can be another build: SMOOTHMESH_TREE names the checkout whose smoothmesh_amd package
(and libsmgpu.so) the process loads -- the parent commit's for `off` and `tangle`, this one's for `quality`.  The caller alternates
the legs in pairs and swaps the order in every second pair.

    dist N STEPS LEG:   one rank (world 1, gloo) of a hex N^3 block through DistributedSmoother, the reference's constraints off:
                        ms per iteration of iterate(STEPS, 0.0), no element ever bad.  LEG: off | tangle | quality.  With a
                        constraint on also the time spent inside its pass calls (the waits for the engine are inside them).
    local STEPS LEG:    the same through LocalMultiSmoother on the two halves, 100 x 100 x 50 cells each, of a hex block.
    kernels:            under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: those
                        halves with passes = 1 and one point next to the processor plane folded through its cells -- a marked pass
                        and the full revert behind it -- and then the serial constraint on one half as a mesh of its own, for
                        k_qc_faces<false> beside k_qc_faces<true>."""
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("SMOOTHMESH_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import SmoothEngine, default_params  # noqa: E402
from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother  # noqa: E402
from smoothmesh_amd.meshgen import hex_subdomain  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "dist"
NEVER = dict(maxNonOrtho=179.9, maxInternalSkewness=1e9, maxBoundarySkewness=1e9)     # every criterion on, no face ever over a limit
CALLS = {"tangle": ("tangle_pass_begin", "tangle_pass_end"),
         "quality": ("quality_constraint_pass_begin", "quality_constraint_pass_faces", "quality_constraint_pass_end")}


def leg_run(sm, engines, steps, leg):
    sm.iterate(20, 0.0)                                          # warm-up: allocations
    spent = {}
    if leg == "tangle":
        sm.set_tangle_constraint()
    elif leg == "quality":
        sm.set_quality_constraint(**NEVER)
    for name in CALLS.get(leg, ()):
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
    if leg != "off":
        recs = sm.tangle_records() if leg == "tangle" else sm.quality_constraint_records()
        assert len(recs) == steps + 10 and not any(r.nBadCells for r in recs)
    inside = ", ".join(f"{1e6 * v / steps:.1f} us inside {k}" for k, v in spent.items())
    print(f"{MODE} {leg}: {ms:.4f} ms per iteration" + (f" ({inside})" if inside else ""), flush=True)


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
    # (a step of a tenth of an edge: the loop cannot carry the folded point back in the one iteration)
    prm = default_params(ms.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False, maxStepLength=0.1 * ms.global_min_edge())
    ms.set_params(prm)
    assert ms.iterate(2, 0.0)[0] == 2
    pts = ms.states[0].eng.get_points()
    xs, ys, zs = (np.unique(pts[:, a]) for a in range(3))      # (no jitter: the lattice planes)
    step = np.array([xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]])
    p = int(np.argmin(np.abs(pts - [xs[-2], ys[len(ys) // 2], zs[len(zs) // 2]]).sum(axis=1)))   # one layer inside the processor plane
    moved = pts.copy()
    moved[p] += 1.5 * step                                       # diagonally past its neighbours: cells fold, faces skew, and
                                                                 # their faces hold shared points
    lim = dict(maxNonOrtho=65.0, maxInternalSkewness=4.0, maxBoundarySkewness=20.0)
    ms.set_quality_constraint(passes=1, **lim)
    ms.states[0].eng.set_points(moved)
    assert ms.iterate(1, 0.0)[0] == 1
    per = ms.quality_constraint_records(per_rank=True)
    # the run is for the kernels' times: one that never launched them is a failure
    assert per[0][0].nBadCells > 0 and per[0][0].passes == 1 and per[0][0].fullRevert == 1 and per[0][0].nPointsReverted > 0, per
    assert per[1][0].passes == 1 and per[1][0].fullRevert == 1
    print(f"shared points {ms.states[0].t.nSend}; records {[(r[0].nBadCells, r[0].nTangledCells, r[0].nNonOrthoFaces, r[0].nSkewFaces, r[0].passes, r[0].fullRevert, r[0].nPointsReverted) for r in per]}", flush=True)
    # the serial constraint on one half, its processor patch an ordinary boundary: k_qc_faces on the same number of faces
    e = SmoothEngine(subs[0].mesh, device=0)
    e.set_params(prm)
    e.set_quality_constraint(passes=1, **lim)
    assert e.iterate(3, 0.0)[0] == 3
    print(f"serial half: records {[(r.nBadCells, r.passes) for r in e.quality_constraint_records()]}", flush=True)
