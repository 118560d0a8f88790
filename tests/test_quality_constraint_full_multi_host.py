"""The drivers of the quality constraint's six further limits on a decomposed mesh (smoothmesh_amd/halo.py
set_quality_constraint_limits, DESIGN.md "Mesh quality" 10.17), without a GPU.  As tests/test_quality_constraint_driver_errors.py: two
gloo processes on the CPU with the oracle's rank engine standing in for the HIP engine, the constraint's calls scripted.  With
minVolRatio on the owner cells' volumes move with the cell centres: one more collective per pass, which a rank whose pass call has
failed must go on answering, or its peer hangs in it (the process group's 30 s time-out then ends the test as a failure).  Also:
the old set_quality_constraint keeps its ValueError on the object that accepts set_quality_constraint_limits."""
import datetime
import json
import os
import sys

import pytest

from test_halo_gloo import _free_port
from test_quality_constraint_driver_errors import SCRIPTS, _stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIMITS = ("minTetQuality", "minTwist", "minTriangleTwist", "minFaceWeight", "minVolRatio", "minDeterminant")


def _stub_full(rank, what, seen):
    """the parent's stub with the new entry: it notes the limits and the volume buffers it is given"""
    class StubFull(_stub(rank, what)):
        def set_quality_constraint_limits_coupled(self, coupling, sendT, recvT, sendCc, recvCc, sendVc=0, recvVc=0, maxNonOrtho=65.0,
                                                  maxInternalSkewness=4.0, maxBoundarySkewness=20.0, passes=2, **more):
            assert set(more) == set(NEW_LIMITS), more
            seen.update(more=more, vc=bool(sendVc) and bool(recvVc))
            self.passes, self.pending = passes, True

        def set_quality_constraint_coupled(self, *a, **k):
            raise AssertionError("set_quality_constraint_limits goes through the new entry")
    return StubFull


def _worker(rank, world, port, what, relTol, ratio, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))
    sub = hex_subdomain((5, 4, 4), (2, 1, 1), rank, jitter=0.3, seed=9)
    seen = {}
    ds = DistributedSmoother(sub, engine_factory=_stub_full(rank, what, seen), torch_device=torch.device("cpu"))
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    widths = []
    swap = ds._quality_swap

    def counted_swap(pats, send, width):
        widths.append(width)
        return swap(pats, send, width)
    ds._quality_swap = counted_swap
    refused = ""
    try:
        ds.set_quality_constraint(passes=2, minVolRatio=0.1)
    except ValueError as ex:
        refused = str(ex)
    ds.set_quality_constraint_limits(passes=2, minVolRatio=0.1 if ratio else None, minDeterminant=0.05)
    out = "no error"
    try:
        ds.iterate(5, relTol)
    except Exception as ex:  # noqa: BLE001 -- the outcome under test
        out = f"{type(ex).__name__}: {ex}"
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(out=out, widths=widths, refused=refused, more=seen["more"], vc=seen["vc"]), f)
    dist.barrier()                      # both ranks are out of iterate() and in step: nobody hangs behind
    dist.destroy_process_group()


@pytest.mark.parametrize("relTol", [0.0, 1e-9])
@pytest.mark.parametrize("what", list(SCRIPTS))
def test_a_failure_inside_a_pass_on_one_rank_raises_on_every_rank_while_volumes_move(tmp_path, oracle_lib, what, relTol):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), what, relTol, True, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2))
    assert r1["out"] == f"RuntimeError: scripted failure in quality_constraint_pass_{SCRIPTS[what][0]}", (r0, r1)
    assert r0["out"].startswith("RuntimeError: another rank"), (r0, r1)
    # the same collectives on both ranks, the failed one included: Cc (3 doubles per face) and Vc (1) side by side, every time
    assert r0["widths"] == r1["widths"] and len(r0["widths"]) >= 4
    assert r0["widths"] == [3, 1] * (len(r0["widths"]) // 2)
    for r in (r0, r1):
        assert r["vc"] and r["more"]["minVolRatio"] == 0.1 and r["more"]["minDeterminant"] == 0.05 and r["more"]["minTwist"] is None
        # the old entry on the same object: its refusal, by name
        assert r["refused"].startswith("set_quality_constraint: minVolRatio is not available on a decomposed mesh")


def test_volumes_stay_home_while_the_ratio_limit_is_off(tmp_path, oracle_lib):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), "faces_later", 0.0, False, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2))
    assert r0["widths"] == r1["widths"] and set(r0["widths"]) == {3}
    assert not r0["vc"] and not r1["vc"] and r0["more"]["minVolRatio"] is None


def test_the_local_smoother_has_both_methods():
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    import inspect
    for cls in (DistributedSmoother, LocalMultiSmoother):
        names = list(inspect.signature(cls.set_quality_constraint_limits).parameters)
        assert names == ["self", "maxNonOrtho", "maxInternalSkewness", "maxBoundarySkewness", "passes", *NEW_LIMITS]
        sig = inspect.signature(cls.set_quality_constraint_limits)
        assert [sig.parameters[k].default for k in names[1:]] == [65.0, 4.0, 20.0, 2] + [None] * 6


def test_combined_records_sum_the_six_counts():
    from smoothmesh_amd.engine import QualityConstraintRecordFull as R
    from smoothmesh_amd.halo import combine_quality_constraint_records
    a = R(iteration=1, passes=1, fullRevert=0, nBadCells=2, nPointsReverted=3, nTangledCells=0, nNonOrthoFaces=1, nSkewFaces=0, nLowTetFaces=1,
          nLowTwistFaces=2, nLowTriangleTwistFaces=3, nLowWeightFaces=4, nLowVolRatioFaces=5, nUnderdeterminedCells=6)
    b = R(iteration=1, passes=1, fullRevert=0, nBadCells=1, nPointsReverted=0, nTangledCells=1, nNonOrthoFaces=0, nSkewFaces=2, nLowTetFaces=10,
          nLowTwistFaces=20, nLowTriangleTwistFaces=30, nLowWeightFaces=40, nLowVolRatioFaces=50, nUnderdeterminedCells=60)
    (c,) = combine_quality_constraint_records([[a], [b]])
    assert c == R(iteration=1, passes=1, fullRevert=0, nBadCells=3, nPointsReverted=3, nTangledCells=1, nNonOrthoFaces=1, nSkewFaces=2,
                  nLowTetFaces=11, nLowTwistFaces=22, nLowTriangleTwistFaces=33, nLowWeightFaces=44, nLowVolRatioFaces=55, nUnderdeterminedCells=66)
