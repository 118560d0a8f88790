"""What the scaling passes of the quality constraint cost on a decomposed mesh (smgpu_set_quality_constraint_scaling_coupled,
DESIGN.md 10.20): nothing while they are off, nothing in an iteration without a bad cell, and per marked pass the new kernels and
the waits of its sweeps.  A sibling of quality_constraint_multirank_timing.py, run as its legs are.

One leg per process, so that a leg can be another build: SMOOTHMESH_TREE names the checkout whose smoothmesh_amd package (and
libsmgpu.so) the process loads -- the parent commit's for the `quality` leg it is compared against, this one's for `quality` and
`scaled`.  The caller alternates the legs and swaps their order in every second round.

    dist N STEPS LEG:   one rank (world 1, gloo) of a hex N^3 block through DistributedSmoother, the reference's constraints off,
                        the constraint on with limits nothing ever reaches: ms per iteration of iterate(STEPS, 0.0).
                        LEG: quality (scaling never switched on) | scaled (S = 2, n = 4).
    local STEPS LEG:    the same through LocalMultiSmoother on the two halves, 100 x 100 x 50 cells each, of a hex block.
    kernels:            under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: those
                        halves with one point next to the processor plane folded through its cells, S = 1, P = 1, n = 4 -- a
                        scaling pass, a reverting pass and the full revert behind them -- and the wall time inside the calls of
                        the passes, the new ones beside pass_begin / pass_faces."""
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("SMOOTHMESH_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import default_params  # noqa: E402
from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother  # noqa: E402
from smoothmesh_amd.meshgen import hex_subdomain  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "dist"
NEVER = dict(maxNonOrtho=179.9, maxInternalSkewness=1e9, maxBoundarySkewness=1e9)     # every criterion on, no face ever over a limit
CALLS = ("quality_constraint_pass_begin", "quality_constraint_pass_faces", "quality_constraint_pass_scale", "quality_constraint_pass_sweep",
         "quality_constraint_pass_end")


def timed_calls(engines):
    """wraps the calls of the passes on every engine; returns {name: [seconds, calls]}"""
    spent = {}
    for name in CALLS:
        if not hasattr(engines[0], name):                         # (the parent build has no scaling calls)
            continue
        spent[name] = [0.0, 0]
        for eng in engines:
            def timed(*a, _f=getattr(eng, name), _n=name):
                t = time.perf_counter()
                r = _f(*a)
                spent[_n][0] += time.perf_counter() - t
                spent[_n][1] += 1
                return r
            setattr(eng, name, timed)
    return spent


def leg_run(sm, engines, steps, leg):
    sm.iterate(20, 0.0)                                          # warm-up: allocations
    sm.set_quality_constraint(**NEVER)
    if leg == "scaled":
        sm.set_quality_constraint_scaling(2, 0.75, 4)
    spent = timed_calls(engines)
    sm.iterate(10, 0.0)
    for v in spent.values():
        v[0], v[1] = 0.0, 0
    t = time.time()
    n = sm.iterate(steps, 0.0)[0]
    ms = 1e3 * (time.time() - t) / n
    assert n == steps
    recs = sm.quality_constraint_records()
    assert len(recs) == steps + 10 and not any(r.nBadCells for r in recs)
    assert all(v[1] == 0 for k, v in spent.items() if k.endswith(("_scale", "_sweep")))       # a clean iteration makes neither call
    inside = ", ".join(f"{1e6 * v[0] / steps:.1f} us inside {k}" for k, v in spent.items() if v[1])
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
    ms.set_quality_constraint_scaling(1, 0.75, 4)
    ms.states[0].eng.set_points(moved)
    spent = timed_calls([st.eng for st in ms.states])
    t = time.perf_counter()
    assert ms.iterate(1, 0.0)[0] == 1
    wall = time.perf_counter() - t
    per = ms.quality_constraint_records_scaled(per_rank=True)
    # the run is for the kernels' times: one that never launched them is a failure
    r0 = per[0][0]
    assert r0.nBadCells > 0 and r0.passes == 2 and r0.nScalePasses == 1 and r0.fullRevert == 1 and r0.nPointsReverted > 0 and r0.minScale == 0.0, per
    assert per[1][0].passes == 2 and per[1][0].fullRevert == 1
    print(f"shared points {ms.states[0].t.nSend}; counted row entries {[int(st.scaleTables[0][-1]) for st in ms.states]}; records "
          f"{[(r[0].nBadCells, r[0].passes, r[0].nScalePasses, r[0].fullRevert, r[0].nPointsReverted, r[0].nPointsScaled, r[0].minScale) for r in per]}", flush=True)
    print(f"the iteration with its three passes: {1e3 * wall:.3f} ms; inside the calls, both engines: " +
          ", ".join(f"{k[len('quality_constraint_'):]} {1e6 * v[0]:.0f} us in {v[1]} calls" for k, v in spent.items()), flush=True)
