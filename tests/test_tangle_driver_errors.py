"""DistributedSmoother's pass loop of the tangle constraint (smoothmesh_amd/halo.py, DESIGN.md "Mesh quality" 10.13) when a call of
a pass fails on ONE rank: every rank raises from the same iterate() call, and none is left inside a collective.  Two gloo
processes on the CPU; the oracle's rank engine stands in for the HIP engine, with the three tangle calls scripted: it keeps the
engine's own rule that smgpu_iter_begin refuses while passes are due, so a failed rank that touched its engine again would raise
alone and leave its peer hanging (the process group's 30 s time-out then ends the test as a failure, not the suite)."""
import datetime
import os
import sys

import pytest

from test_halo_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL_AT = 2          # the iteration (1-based) whose pass fails on rank 1


def _stub(rank, what):
    from oracle.oracle_ffi import OracleRankEngine

    class Stub(OracleRankEngine):
        """what: "begin" -- pass_begin raises; "end_mid" -- rank 0 reports a bad cell at k = 0, so the pass is not the last, and
        pass_end raises; "end_last" -- nothing is bad, the first pass is the last, and pass_end raises"""
        due, k, iteration = False, 0, 0

        def set_tangle_constraint_coupled(self, sendT, recvT, passes=2):
            self.passes = passes

        def iter_begin(self):
            if self.due:
                raise RuntimeError("smgpu_iter_begin: the coupled tangle constraint has not finished the passes of the last iteration")
            super().iter_begin()

        def iter_end(self):
            super().iter_end()
            self.due, self.k = True, 0
            self.iteration += 1

        def tangle_pass_begin(self):
            assert self.due
            if what == "begin" and rank == 1 and self.iteration == FAIL_AT:
                raise RuntimeError("scripted failure in tangle_pass_begin")
            return 1 if (what == "end_mid" and rank == 0 and self.k == 0) else 0

        def tangle_pass_end(self, total):
            if what.startswith("end") and rank == 1 and self.iteration == FAIL_AT and self.k == 0:
                raise RuntimeError("scripted failure in tangle_pass_end")
            if total == 0 or self.k == self.passes:
                self.due = False
                return True
            self.k += 1
            return False
    return Stub


def _worker(rank, world, port, what, relTol, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))
    sub = hex_subdomain((5, 4, 4), (2, 1, 1), rank, jitter=0.3, seed=9)
    ds = DistributedSmoother(sub, engine_factory=_stub(rank, what), torch_device=torch.device("cpu"))
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    ds.set_tangle_constraint(2)
    out = "no error"
    try:
        ds.iterate(5, relTol)
    except Exception as ex:  # noqa: BLE001 -- the outcome under test
        out = f"{type(ex).__name__}: {ex}"
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(out)
    dist.barrier()                      # both ranks are out of iterate() and in step: nobody hangs behind
    dist.destroy_process_group()


@pytest.mark.parametrize("relTol", [0.0, 1e-9])
@pytest.mark.parametrize("what", ["begin", "end_mid", "end_last"])
def test_a_failure_inside_a_pass_on_one_rank_raises_on_every_rank(tmp_path, oracle_lib, what, relTol):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), what, relTol, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = ((tmp_path / f"rank{r}.txt").read_text() for r in range(2))
    assert r1 == f"RuntimeError: scripted failure in tangle_pass_{'begin' if what == 'begin' else 'end'}", (r0, r1)
    assert r0.startswith("RuntimeError: another rank"), (r0, r1)
