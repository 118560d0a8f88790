"""The host side of the quality constraint's scaling passes on a decomposed mesh (DESIGN.md "Mesh quality", 10.20) without a GPU:
the set-up tables of smoothmesh_amd/halo.py (scale_edge_info, scale_tables) on cut blocks against a count on the undecomposed mesh,
the record combination, the new methods' one owner on the base the two smoothers share, the refusals that need no device, and
DistributedSmoother's pass loop when a call of the scaling protocol fails on ONE rank (as
tests/test_quality_constraint_driver_errors.py: two gloo processes on the CPU, the oracle's rank engine standing in for the HIP
engine with the constraint's calls scripted and the engine's own rules about their order kept)."""
import datetime
import inspect
import os
import sys

import numpy as np
import pytest

from test_halo_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(mesh, grid):
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.engine import HostTopology
    from smoothmesh_amd.halo import HaloTables, scale_edge_info, scale_tables
    subs = decompose(mesh, grid_partition(mesh, grid), int(np.prod(grid)))
    cands = [s.processor_patch_point_lists() for s in subs]
    tabs = [HaloTables(s.rank, s.pointProcAddressing, cands) for s in subs]
    rows = [HostTopology(s.mesh).addressing("pointPoints") for s in subs]
    infos = [scale_edge_info(t, r) for t, r in zip(tabs, rows)]
    return subs, tabs, rows, infos, [scale_tables(t, r, infos) for t, r in zip(tabs, rows)]


@pytest.mark.parametrize("grid,sharers,holders", [((2, 1, 1), 2, 2), ((2, 2, 1), 4, 4), ((4, 3, 1), 4, 4)])
def test_tables_against_the_undecomposed_mesh(grid, sharers, holders):
    """every edge of the whole mesh at a shared point is counted on exactly one rank, from either end; sharedDeg is the degree in
    the whole mesh; the cuts cover a point with four sharers and an edge held by four ranks"""
    from smoothmesh_amd.engine import HostTopology
    from smoothmesh_amd.meshgen import hex_block
    mesh = hex_block(9, 7, 3, jitter=0.2, seed=5)
    subs, tabs, rows, infos, out = _tables(mesh, grid)
    goff, gval = (np.asarray(a, np.int64) for a in HostTopology(mesh).addressing("pointPoints"))
    gdeg = np.diff(goff)
    directed = {}                                          # (global p, global q) of every counted entry -> how often
    uncounted = 0
    for s, t, (off, val), (rowOff, rowPt, deg) in zip(subs, tabs, rows, out):
        ppa = np.asarray(s.pointProcAddressing, np.int64)
        assert rowOff.dtype == rowPt.dtype == deg.dtype == np.int32 and len(rowOff) == len(t.sharedLocal) + 1 and len(deg) == len(t.sharedLocal)
        assert rowOff[0] == 0 and rowOff[-1] == len(rowPt) and (np.diff(rowOff) >= 0).all()
        assert np.array_equal(deg, gdeg[ppa[t.sharedLocal]])                       # the degree in the whole mesh
        for i, p in enumerate(t.sharedLocal):
            row = [int(q) for q in val[off[p]:off[p + 1]]]
            counted = [int(q) for q in rowPt[rowOff[i]:rowOff[i + 1]]]
            it = iter(row)
            assert all(q in it for q in counted)                                   # a sub-sequence of the row: row order kept
            uncounted += len(row) - len(counted)
            for q in counted:
                directed[(int(ppa[p]), int(ppa[q]))] = directed.get((int(ppa[p]), int(ppa[q])), 0) + 1
    shared = np.unique(np.concatenate([np.asarray(s.pointProcAddressing, np.int64)[t.sharedLocal] for s, t in zip(subs, tabs)]))
    want = {(int(p), int(q)) for p in shared for q in gval[goff[p]:goff[p + 1]]}
    assert set(directed) == want and set(directed.values()) == {1}
    assert uncounted > 0
    # what the cut is for
    assert max(int(np.diff(t.combOffsets).max()) for t in tabs) == sharers
    held = {}
    for info in infos:
        for k in map(tuple, info["keys"].tolist()):
            held[k] = held.get(k, 0) + 1
    assert max(held.values()) == holders
    # an entry with an unshared end is always counted: per rank, the counted entries are at least those
    for t, (off, val), (rowOff, rowPt, deg), info in zip(tabs, rows, out, infos):
        assert (np.diff(rowOff) >= info["unshared"]).all() and (deg >= np.diff(rowOff)).all()


def test_tables_of_a_rank_without_shared_points():
    from smoothmesh_amd.meshgen import hex_block
    subs, tabs, rows, infos, out = _tables(hex_block(4, 3, 3), (1, 1, 1))
    rowOff, rowPt, deg = out[0]
    assert rowOff.tolist() == [0] and len(rowPt) == 0 and len(deg) == 0 and infos[0]["keys"].shape == (0, 4) and infos[0]["names"].shape == (0, 2)


def test_combined_scaled_records():
    from smoothmesh_amd.engine import QualityConstraintRecordScaled as R
    from smoothmesh_amd.halo import combine_quality_constraint_records_scaled
    base = dict(iteration=3, passes=2, fullRevert=0, nTangledCells=0, nNonOrthoFaces=0, nScalePasses=2)
    a = R(nBadCells=2, nPointsReverted=3, nSkewFaces=1, nPointsScaled=5, minScale=0.5625, **base)
    b = R(nBadCells=0, nPointsReverted=4, nSkewFaces=0, nPointsScaled=7, minScale=0.75, **base)
    (c,) = combine_quality_constraint_records_scaled([[a], [b]])
    assert c == R(nBadCells=2, nPointsReverted=7, nSkewFaces=1, nPointsScaled=12, minScale=0.5625, **base)
    b.nScalePasses = 1                                     # a global value: the ranks agree on it
    with pytest.raises(AssertionError):
        combine_quality_constraint_records_scaled([[a], [b]])


def test_the_new_methods_have_one_owner():
    from smoothmesh_amd.halo import DistributedSmoother, LocalMultiSmoother
    methods = ("set_quality_constraint_scaling", "quality_constraint_records_scaled", "quality_constraint_state_scaled", "_constraint_passes")
    shared = [b for b in DistributedSmoother.__mro__[1:] if b in LocalMultiSmoother.__mro__[1:] and b is not object]
    assert shared, "no shared base"
    for m in methods:
        assert m not in vars(DistributedSmoother) and m not in vars(LocalMultiSmoother), m
        assert getattr(DistributedSmoother, m) is getattr(LocalMultiSmoother, m) and any(m in vars(b) for b in shared), m
    sig = inspect.signature(DistributedSmoother.set_quality_constraint_scaling).parameters
    assert [(k, sig[k].default) for k in ("scalePasses", "errorReduction", "nSmoothScale")] == [("scalePasses", 0), ("errorReduction", 0.75), ("nSmoothScale", 4)]
    # what moves S is each smoother's own
    assert "_move_scales" in vars(DistributedSmoother) and "_move_scales" in vars(LocalMultiSmoother)
    assert DistributedSmoother.scale_passes == 0 and LocalMultiSmoother.scale_passes == 0


@pytest.mark.parametrize("cls", ["LocalMultiSmoother", "DistributedSmoother"])
def test_refusals_that_need_no_device(cls):
    """the quality constraint not on: by name, before anything of the smoother but that is looked at; the keywords on
    set_quality_constraint keep their ValueError (tests/test_quality_constraint_scaled_host.py pins its wording)"""
    from smoothmesh_amd import halo
    smoother = object.__new__(getattr(halo, cls))
    smoother.quality_passes = None
    with pytest.raises(RuntimeError, match="set_quality_constraint_scaling: the quality constraint is off; set_quality_constraint first"):
        smoother.set_quality_constraint_scaling(2)
    with pytest.raises(ValueError, match="is not available on a decomposed mesh"):
        smoother.set_quality_constraint(scalePasses=2)


# ---- a failure inside the scaling calls of a pass, on one rank ------------------------------------------------------------
FAIL_AT = 2          # the iteration (1-based) whose pass fails on rank 1
S, N_SWEEPS, P = 1, 2, 1
# what -> (the call that raises, the pass it raises in, the sweep it raises in)
SCRIPTS = {"scale_first": ("scale", 0, 0), "scale_later": ("scale", 1, 0), "sweep_first": ("sweep", 0, 0), "sweep_second": ("sweep", 0, 1),
           "sweep_later_pass": ("sweep", 1, 1), "end_scaled": ("end", 0, 0)}


def _stub(rank, what):
    from oracle.oracle_ffi import OracleRankEngine
    call, at, sweep = SCRIPTS[what]

    class Stub(OracleRankEngine):
        due, k, stage, iteration, S, n, sweeps = False, 0, 0, 0, 0, 0, 0

        def quality_coupling(self, r=None):
            return (0 if r is None else int(r)), []

        def set_quality_constraint_coupled(self, coupling, sendT, recvT, sendCc, recvCc, maxNonOrtho=65.0, maxInternalSkewness=4.0,
                                           maxBoundarySkewness=20.0, passes=2):
            self.passes, self.pending = passes, True

        def quality_constraint_coupled_exempt(self):
            assert self.pending
            self.pending = False

        def set_quality_constraint_scaling_coupled(self, rowOffsets, rowPoints, sharedDeg, sendS, recvS, scalePasses=0, errorReduction=0.75, nSmoothScale=4):
            assert not self.due and not self.pending
            if scalePasses > 0:
                assert len(rowOffsets) == len(sharedDeg) + 1 and rowOffsets[-1] == len(rowPoints) and len(sharedDeg) > 0 and min(sharedDeg) > 0
            self.S, self.n = int(scalePasses), int(nSmoothScale)

        def iter_begin(self):
            if self.due:
                raise RuntimeError("smgpu_iter_begin: the coupled quality constraint has not finished the passes of the last iteration")
            super().iter_begin()

        def iter_end(self):
            super().iter_end()
            self.due, self.k, self.stage = True, 0, 0
            self.iteration += 1

        def _fails(self, name, sweep_index=0):
            return call == name and rank == 1 and self.iteration == FAIL_AT and self.k == at and sweep_index == sweep

        def quality_constraint_pass_begin(self):
            assert self.due and self.stage == 0
            self.stage = 1

        def quality_constraint_pass_faces(self):
            assert self.stage == 1
            self.stage = 2
            return 1 if (rank == 0 and self.k <= 1) else 0           # two marked passes: one that scales, one that reverts

        def quality_constraint_pass_scale(self, total):
            assert self.stage == 2 and total > 0 and self.S > 0
            if self._fails("scale"):
                raise RuntimeError("scripted failure in quality_constraint_pass_scale")
            self.stage, self.sweeps = 3, (self.n if self.k < self.S + self.passes else 0)

        def quality_constraint_pass_sweep(self):
            assert self.stage == 3 and self.sweeps > 0
            if self._fails("sweep", self.n - self.sweeps):
                raise RuntimeError("scripted failure in quality_constraint_pass_sweep")
            self.sweeps -= 1

        def quality_constraint_pass_end(self, total):
            assert self.stage == (3 if total > 0 and self.S > 0 else 2) and (total == 0 or self.sweeps == 0)
            if self._fails("end"):
                raise RuntimeError("scripted failure in quality_constraint_pass_end")
            self.stage = 0
            if total == 0 or self.k == self.S + self.passes:
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
    ds.set_quality_constraint(passes=P)
    ds.set_quality_constraint_scaling(S, 0.75, N_SWEEPS)
    assert (ds.scale_passes, ds.scale_sweeps) == (S, N_SWEEPS) and ds.state.sendS.shape == (ds.tables.nSend,) and ds.tables.nSend > 0
    out = "no error"
    try:
        ds.iterate(5, relTol)
    except Exception as ex:  # noqa: BLE001 -- the outcome under test
        out = f"{type(ex).__name__}: {ex}"
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(out)
    dist.barrier()                      # both ranks are out of iterate() and in step: nobody hangs behind
    dist.destroy_process_group()


@pytest.mark.parametrize("what,relTol", [(w, 0.0) for w in SCRIPTS] + [("sweep_second", 1e-9)])
def test_a_failure_inside_the_scaling_calls_on_one_rank_raises_on_every_rank(tmp_path, oracle_lib, what, relTol):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), what, relTol, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = ((tmp_path / f"rank{r}.txt").read_text() for r in range(2))
    assert r1 == f"RuntimeError: scripted failure in quality_constraint_pass_{SCRIPTS[what][0]}", (r0, r1)
    assert r0.startswith("RuntimeError: another rank"), (r0, r1)


def _worker_setup_failure(rank, world, port, out_dir):
    """rank 1's engine refuses the scaling call: both ranks raise from set_quality_constraint_scaling and scaling is off on both"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))
    Base = _stub(rank, "scale_first")

    class Refusing(Base):
        def set_quality_constraint_scaling_coupled(self, rowOffsets, rowPoints, sharedDeg, sendS, recvS, scalePasses=0, errorReduction=0.75, nSmoothScale=4):
            if rank == 1 and scalePasses > 0:
                raise RuntimeError("scripted refusal of set_quality_constraint_scaling_coupled")
            super().set_quality_constraint_scaling_coupled(rowOffsets, rowPoints, sharedDeg, sendS, recvS, scalePasses, errorReduction, nSmoothScale)

    sub = hex_subdomain((5, 4, 4), (2, 1, 1), rank, jitter=0.3, seed=9)
    ds = DistributedSmoother(sub, engine_factory=Refusing, torch_device=torch.device("cpu"))
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    ds.set_quality_constraint(passes=P)
    out = "no error"
    try:
        ds.set_quality_constraint_scaling(S, 0.75, N_SWEEPS)
    except Exception as ex:  # noqa: BLE001 -- the outcome under test
        out = f"{type(ex).__name__}: {ex}"
    out += f" | scale_passes {ds.scale_passes} engine S {ds.engine.S}"
    ds.iterate(2, 0.0)                  # the unscaled pass loop still runs, in step
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(out)
    dist.barrier()
    dist.destroy_process_group()


def test_a_refused_set_up_on_one_rank_leaves_scaling_off_on_every_rank(tmp_path, oracle_lib):
    import torch.multiprocessing as mp
    mp.spawn(_worker_setup_failure, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = ((tmp_path / f"rank{r}.txt").read_text() for r in range(2))
    assert r1 == "RuntimeError: scripted refusal of set_quality_constraint_scaling_coupled | scale_passes 0 engine S 0", (r0, r1)
    assert r0.startswith("RuntimeError: another rank") and r0.endswith("| scale_passes 0 engine S 0"), (r0, r1)
