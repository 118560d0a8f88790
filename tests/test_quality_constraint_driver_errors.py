"""DistributedSmoother's pass loop of the quality constraint (smoothmesh_amd/halo.py, DESIGN.md "Mesh quality" 10.15) when a call of a
pass fails on ONE rank: every rank raises from the same iterate() call, and none is left inside a collective -- the exchange of
cell centres in the middle of a pass included.  As tests/test_tangle_driver_errors.py: two gloo processes on the CPU, the oracle's
rank engine standing in for the HIP engine with the constraint's calls scripted; it keeps the engine's own rules (the order of the
three calls of a pass, smgpu_iter_begin refusing while passes are due), so a failed rank that touched its engine again would raise
alone and leave its peer hanging (the process group's 30 s time-out then ends the test as a failure, not the suite)."""
import datetime
import os
import sys

import pytest

from test_halo_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL_AT = 2          # the iteration (1-based) whose pass fails on rank 1
# what -> (the call that raises, the pass it raises in, whether rank 0 reports a bad cell at k = 0 so that the pass is not the last)
SCRIPTS = {"begin_first": ("begin", 0, False), "begin_later": ("begin", 1, True), "faces_first": ("faces", 0, False),
           "faces_later": ("faces", 1, True), "end_mid": ("end", 0, True), "end_last": ("end", 0, False)}


def _stub(rank, what):
    from oracle.oracle_ffi import OracleRankEngine
    call, at, bad0 = SCRIPTS[what]

    class Stub(OracleRankEngine):
        due, k, stage, iteration = False, 0, 0, 0

        def quality_coupling(self, r=None):
            return (0 if r is None else int(r)), []

        def set_quality_constraint_coupled(self, coupling, sendT, recvT, sendCc, recvCc, maxNonOrtho=65.0, maxInternalSkewness=4.0,
                                           maxBoundarySkewness=20.0, passes=2):
            self.passes, self.pending = passes, True

        def quality_constraint_coupled_exempt(self):
            assert self.pending
            self.pending = False

        def iter_begin(self):
            if self.due:
                raise RuntimeError("smgpu_iter_begin: the coupled quality constraint has not finished the passes of the last iteration")
            super().iter_begin()

        def iter_end(self):
            super().iter_end()
            self.due, self.k, self.stage = True, 0, 0
            self.iteration += 1

        def _fails(self, name):
            return call == name and rank == 1 and self.iteration == FAIL_AT and self.k == at

        def quality_constraint_pass_begin(self):
            assert self.due and self.stage == 0
            if self._fails("begin"):
                raise RuntimeError("scripted failure in quality_constraint_pass_begin")
            self.stage = 1

        def quality_constraint_pass_faces(self):
            assert self.stage == 1
            if self._fails("faces"):
                raise RuntimeError("scripted failure in quality_constraint_pass_faces")
            self.stage = 2
            return 1 if (bad0 and rank == 0 and self.k == 0) else 0

        def quality_constraint_pass_end(self, total):
            assert self.stage == 2
            if self._fails("end"):
                raise RuntimeError("scripted failure in quality_constraint_pass_end")
            self.stage = 0
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
    ds.set_quality_constraint(passes=2)
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
@pytest.mark.parametrize("what", list(SCRIPTS))
def test_a_failure_inside_a_pass_on_one_rank_raises_on_every_rank(tmp_path, oracle_lib, what, relTol):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), what, relTol, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = ((tmp_path / f"rank{r}.txt").read_text() for r in range(2))
    assert r1 == f"RuntimeError: scripted failure in quality_constraint_pass_{SCRIPTS[what][0]}", (r0, r1)
    assert r0.startswith("RuntimeError: another rank"), (r0, r1)
