"""What the tangle constraint costs per iteration on a decomposed mesh (smgpu_set_tangle_constraint_coupled), and
the kernel times of its exchange and revert.

    dist N STEPS:   no profiler: one rank (world 1, gloo) of a hex N^3 block through DistributedSmoother, the reference's
                    constraints off: ms per iteration of iterate(STEPS) with the constraint off against on, with no cell ever bad,
                    in alternating pairs on one smoother with the order swapped.  Off is the parent's behaviour launch for launch
                    (tests/test_gpu_tangle_multirank.py::test_numbering_across_calls_and_clearing).  Then the host's share on its
                    own: the time spent inside tangle_pass_begin (the read that waits for the iteration) and tangle_pass_end, and
                    a loop of the all_reduce of {count, failed} that a world of more than one rank adds (gloo on the CPU here).
    local STEPS:    the same pairs through LocalMultiSmoother on the two halves, 100 x 100 x 50 cells each, of a hex block.
    kernels:        under `rocprofv3 --kernel-trace --stats` (profiles/quality/README.md), no counters, one process: those halves
                    with passes = 1 and one point next to the processor plane folded through its cells: a marked pass (k_tangle_pack,
                    k_tangle_combine, k_tangle_apply_counted on the marks) and the full revert behind it."""
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from smoothmesh_amd import default_params  # noqa: E402
from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother  # noqa: E402
from smoothmesh_amd.meshgen import hex_subdomain  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "dist"


def pairs(sm, steps, records):
    sm.iterate(20, 0.0)                                          # warm-up: allocations
    for pair in range(4):
        ms = {}
        for on in ((False, True) if pair % 2 == 0 else (True, False)):
            if on:
                sm.set_tangle_constraint()
            t = time.time()
            n = sm.iterate(steps, 0.0)[0]
            ms[on] = 1e3 * (time.time() - t) / n
            assert n == steps
            if on:
                recs = records(sm)
                assert len(recs) == steps and not any(r.nBadCells for r in recs)
                sm.clear_tangle_constraint()
        print(f"pair {pair}: {ms[False]:.4f} ms per iteration without the constraint, {ms[True]:.4f} with it "
              f"({100 * (ms[True] / ms[False] - 1):+.2f} %, {1e3 * (ms[True] - ms[False]):+.1f} us)", flush=True)


def halves(jitter=0.0):
    t = time.time()
    subs = [hex_subdomain((100, 100, 50), (2, 1, 1), r, jitter=jitter, seed=5) for r in range(2)]
    print(f"two sub-domains of {subs[0].mesh.nCells} cells, {subs[0].mesh.nPoints} points ({time.time() - t:.1f} s)", flush=True)
    return subs


if MODE == "dist":
    import torch
    import torch.distributed as dist
    N, STEPS = int(sys.argv[2]), int(sys.argv[3])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    sub = hex_subdomain((N, N, N), (1, 1, 1), 0, jitter=0.0, seed=5)
    print(f"one rank of hex {N}^3: {sub.mesh.nCells} cells, {sub.mesh.nPoints} points", flush=True)
    ds = DistributedSmoother(sub, device=0, overlap=False)
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    pairs(ds, STEPS, lambda x: x.tangle_records())
    # the host's share: time inside the two calls of a clean iteration
    ds.set_tangle_constraint()
    eng, spent = ds.engine, {"begin": 0.0, "end": 0.0}
    b0, e0 = eng.tangle_pass_begin, eng.tangle_pass_end

    def begin():
        t = time.perf_counter(); r = b0(); spent["begin"] += time.perf_counter() - t
        return r

    def end(n):
        t = time.perf_counter(); r = e0(n); spent["end"] += time.perf_counter() - t
        return r
    eng.tangle_pass_begin, eng.tangle_pass_end = begin, end
    t = time.time()
    assert ds.iterate(STEPS, 0.0)[0] == STEPS
    total = time.time() - t
    print(f"constraint on: {1e3 * total / STEPS:.4f} ms per iteration, of it {1e6 * spent['begin'] / STEPS:.1f} us inside tangle_pass_begin (launches and the "
          f"read that waits for the iteration) and {1e6 * spent['end'] / STEPS:.1f} us inside tangle_pass_end", flush=True)
    v = torch.tensor([0, 0], dtype=torch.int64)
    t = time.perf_counter()
    for _ in range(1000):
        v = torch.tensor([0, 0], dtype=torch.int64)
        dist.all_reduce(v)
        v.tolist()
    print(f"the verdict's all_reduce of two int64 (gloo, CPU tensor, world 1): {1e3 * (time.perf_counter() - t):.1f} us per call", flush=True)
    ds.close()
    dist.destroy_process_group()
elif MODE == "local":
    STEPS = int(sys.argv[2])
    subs = halves()
    ms = LocalMultiSmoother(subs, device=0, overlap=False)
    ms.set_params(default_params(ms.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    pairs(ms, STEPS, lambda x: x.tangle_records())
else:
    subs = halves()
    ms = LocalMultiSmoother(subs, device=0, overlap=False)
    # (a step of a tenth of an edge: the loop cannot carry the folded point back in the one iteration)
    ms.set_params(default_params(ms.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False, maxStepLength=0.1 * ms.global_min_edge()))
    assert ms.iterate(2, 0.0)[0] == 2
    pts = ms.states[0].eng.get_points()
    xs, ys, zs = (np.unique(pts[:, a]) for a in range(3))      # (no jitter: the lattice planes)
    step = np.array([xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]])
    p = int(np.argmin(np.abs(pts - [xs[-2], ys[len(ys) // 2], zs[len(zs) // 2]]).sum(axis=1)))   # one layer inside the processor plane
    moved = pts.copy()
    moved[p] += 1.5 * step                                       # diagonally past its neighbours: four cells fold (none was exempt),
                                                                 # and their faces hold shared points
    ms.set_tangle_constraint(1)
    ms.states[0].eng.set_points(moved)
    assert ms.iterate(1, 0.0)[0] == 1
    per = ms.tangle_records(per_rank=True)
    # the run is for the kernels' times: one that never launched them is a failure
    assert per[0][0].nBadCells > 0 and per[0][0].passes == 1 and per[0][0].fullRevert == 1 and per[0][0].nPointsReverted > 0, per
    assert per[1][0].passes == 1 and per[1][0].fullRevert == 1
    print(f"shared points {ms.states[0].t.nSend}; records {[(r[0].nBadCells, r[0].passes, r[0].fullRevert, r[0].nPointsReverted) for r in per]}", flush=True)
