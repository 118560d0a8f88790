"""The tangle constraint on a decomposed mesh (include/smgpu.h smgpu_set_tangle_constraint_coupled / smgpu_tangle_pass_begin /
smgpu_tangle_pass_end, csrc/kernels_quality_tangle.hpp, DESIGN.md "Mesh quality" 10.13) through the two smoothers of halo.py, against
its CPU restatement (tests/tangle_multi_reference.py, pinned against the serial restatement by tests/test_tangle_multi_reference.py):
per-rank and combined records exactly and the points of every iteration at the project's decomposed tolerance, copies of shared
points bit-identical; the invariant through the existing report; a constraint that never fires leaves the run untouched, the
look-ahead geometry included; the look-ahead while points are reverted; DistributedSmoother on one rank against the serial engine
and on two processes; numbering, clearing and refusals."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_linf
from tangle_multi_reference import FIELDS
from test_gpu_multirank import _copies_identical, _hex_case
from test_tangle_multi_reference import MULTI_CASES, multi_mesh, multi_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (variant, the reference's constraints, passes, overlap, environment): both variants and the constraints off / on at the default
# passes, in order and with an exchange stream; fewer passes, the direct geometry kernels and the other tile shapes on the
# unconstrained .com run
SETTINGS = [("com", False, 2, False, {}), ("com", True, 2, True, {}), ("org", False, 2, True, {}), ("org", True, 2, False, {}),
            ("com", False, 0, True, {}), ("com", False, 1, False, {}), ("com", False, 2, True, {"SMGPU_TILES": "0"}),
            ("com", False, 2, False, {"SMGPU_GEOM_T": "64"}), ("com", False, 2, True, {"SMGPU_GEOM_T": "256"})]


def _records(recs):
    return [{k: getattr(r, k) for k in FIELDS} for r in recs]


def _smoother(ref, variant, overlap, passes, env, monkeypatch):
    from smoothmesh_amd.halo import LocalMultiSmoother
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ms = LocalMultiSmoother(ref.subs, device=0, overlap=overlap)
    for st in ms.states:
        st.eng.set_foam_variant(variant)
    ms.set_params(ref.prm)
    if passes is not None:
        ms.set_tangle_constraint(passes)
    return ms


def _close(ms):
    for st in ms.states:
        st.eng.close()


# ---- 1. the smoother = the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,constraints,passes,overlap,env", SETTINGS)
@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_local_multi_smoother_equals_reference(oracle_lib, monkeypatch, name, variant, constraints, passes, overlap, env):
    n = MULTI_CASES[name][3]
    want = multi_reference(oracle_lib, name, variant, constraints, passes)
    ref = want["ref"]
    ms = _smoother(ref, variant, overlap, passes, env, monkeypatch)
    st = ms.tangle_state()
    assert st.on and st.passes == passes and st.nExemptCells == sum(ref.nExemptCells) and st.iteration == 0
    for k in range(n):
        got = ms.iterate(1, 0.0)
        assert got[0] == 1 and int(got[2][0]) == int(want["frz"][k])
        pts = ms.get_points()
        for r, p in enumerate(pts):
            err = rel_linf(p, want["pts"][k][r])
            print(name, k, r, err)
            assert err <= 1e-13, (k, r, err)
        _copies_identical(ref.subs, pts)
    from smoothmesh_amd.halo import combine_tangle_records
    raw = ms.tangle_records(per_rank=True)
    assert [_records(r) for r in raw] == want["per_rank"]
    assert _records(combine_tangle_records(raw)) == want["recs"]
    assert ms.tangle_records() == []                                                # a read clears
    assert ms.tangle_state().iteration == n
    if not constraints:
        assert any(r["nBadCells"] > 0 for r in want["recs"]), "the mesh does not tangle: the case tests nothing"
    _close(ms)


# ---- 2. the invariant, through the existing report ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_invariant_through_the_report(oracle_lib, monkeypatch, name):
    want = multi_reference(oracle_lib, name, "com", False, 2)
    ms = _smoother(want["ref"], "com", True, 2, {}, monkeypatch)
    q0 = ms.mesh_quality()
    for _ in range(MULTI_CASES[name][3]):
        assert ms.iterate(1, 0.0)[0] == 1
        q = ms.mesh_quality()
        assert q.nNonPositiveVolume <= q0.nNonPositiveVolume and q.nWrongOrientedFaces <= q0.nWrongOrientedFaces
    assert any(r.nBadCells > 0 for r in ms.tangle_records())
    # ... and without the constraint the same run tangles
    free = _smoother(want["ref"], "com", True, None, {}, monkeypatch)
    assert free.iterate(MULTI_CASES[name][3], 0.0)[0] == MULTI_CASES[name][3]
    q = free.mesh_quality()
    assert q.nWrongOrientedFaces > q0.nWrongOrientedFaces
    _close(ms), _close(free)


# ---- 3. a constraint that never fires leaves the run untouched ---------------------------------------------------------
@pytest.mark.parametrize("layers", [False, True])
def test_constraint_that_never_fires_leaves_the_run_untouched(oracle_lib, layers):
    """(16, 12, 12) sub-domains cut (2, 2, 1) with an exchange stream: several geometry tiles per rank, so smgpu_iter_ahead
    recomputes the interior ones for the next iteration while the passes are still to come"""
    from smoothmesh_amd import LayerParams
    from smoothmesh_amd.halo import LocalMultiSmoother
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 1), (16, 12, 12), False)
    runs = []
    for on in (False, True):
        ms = LocalMultiSmoother(subs, device=0, overlap=True)
        ms.set_params(prm)
        if layers:
            assert ms.set_layers(LayerParams(layerPatches=("xmin",), layerExpansionRatio=1.2), prm.minEdgeLength)
        if on:
            ms.set_tangle_constraint()
            assert ms.tangle_state().nExemptCells == 0
        ms.states[0].eng.enable_timing(True)
        n, res, frz = ms.iterate(8, 0.0)
        assert n == 8
        geom = {c["name"]: c["launches"] for c in ms.states[0].eng.counters()}["k_geom_tile"]
        if not layers:
            assert geom == 16                              # 1 + 7 + 8: the look-ahead is live (tests/test_gpu_multirank.py)
        if on:
            assert _records(ms.tangle_records()) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0) for k in range(1, 9)]
        runs.append((res, frz, ms.get_points(), geom))
        _close(ms)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


# ---- 4. the look-ahead while points are reverted -----------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SMGPU_GEOM_T": "64"}])
def test_look_ahead_geometry_is_not_trusted_behind_a_revert(oracle_lib, monkeypatch, env):
    """dented_block_tiles() cut (4, 1, 1), the reference's constraints off, with an exchange stream: smgpu_iter_ahead is active
    while points are reverted from iteration 8 on.  The bits of the run in order, where no geometry is computed ahead."""
    want = multi_reference(oracle_lib, "tiles_411", "com", False, 2)
    out = {}
    for overlap in (False, True):
        ms = _smoother(want["ref"], "com", overlap, 2, env, monkeypatch)
        n, res, frz = ms.iterate(12, 0.0)
        assert n == 12
        out[overlap] = (res, frz, ms.get_points(), _records(ms.tangle_records()))
        print(env, overlap, [st.eng.debug_halo_tiles() for st in ms.states])
        _close(ms)
    a, b = out[False], out[True]
    assert a[3] == b[3] == want["recs"] and any(r["nPointsReverted"] > 0 for r in a[3][7:])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


def _wide_dented_block():
    """the dent of dented_block_tiles() in a block twice as long in x (25 x 10 x 8 points, the same spacing of 0.25): cut (2, 1, 1),
    rank 0 spans several geometry tiles and the dent lies three cells and more away from the processor plane x = 3 -- in cells whose
    tiles hold no shared point, the ones smgpu_iter_ahead recomputes.  On the CPU (tests/tangle_multi_reference.py): 4 bad cells
    and 9 points reverted in every iteration from 8 on, the serial restatement's records, margin 2.9e-3"""
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(24, 9, 7, lengths=(6.0, 2.25, 1.75))
    assert m.nPoints == 2000 and m.nCells == 1512
    m.points = m.points.copy()
    for z, to in ((0.0, 0.75), (0.25, 0.8), (0.5, 0.85), (0.75, 0.9)):
        p = int(np.argmin(np.abs(m.points - [0.5, 0.5, z]).sum(axis=1)))
        assert np.array_equal(m.points[p], [0.5, 0.5, z])
        m.points[p] = [0.5, 0.5, to]
    return m


@pytest.mark.parametrize("geomT", ["64", "128"])
def test_look_ahead_over_interior_tiles_behind_a_revert(oracle_lib, monkeypatch, geomT):
    """the same hazard where the look-ahead has tiles to compute: the points that go back belong to interior tiles of rank 0, whose
    geometry for the next iteration smgpu_iter_ahead has already left behind.  A look-ahead that were trusted would smooth iteration
    9 on the geometry of the points iteration 8 rejected."""
    from tangle_multi_reference import MARGIN, TangleMultiReference
    ref = TangleMultiReference(oracle_lib, _wide_dented_block(), (2, 1, 1), 2, "com", False, maxStepLength=0.03, minEdgeLength=1e-4)
    want = ref.run(12)
    assert ref.minMargin > MARGIN
    assert [r["nPointsReverted"] for r in want["recs"]] == [0] * 7 + [9] * 5
    out = {}
    for overlap in (False, True):
        ms = _smoother(ref, "com", overlap, 2, {"SMGPU_GEOM_T": geomT}, monkeypatch)
        tiles = ms.states[0].eng.debug_halo_tiles()
        print(geomT, overlap, tiles)
        assert tiles["geom_interior"] > 0 and tiles["geom_shared"] > 0
        ms.states[0].eng.enable_timing(True)
        n, res, frz = ms.iterate(12, 0.0)
        assert n == 12
        geom = {c["name"]: c["launches"] for c in ms.states[0].eng.counters()}["k_geom_tile"]
        out[overlap] = (res, frz, ms.get_points(), _records(ms.tangle_records()), geom)
        _close(ms)
    a, b = out[False], out[True]
    # in order: one launch per iteration.  With an exchange stream: the look-ahead of every iteration, the shared tiles alone where
    # it is trusted (iterations 2 .. 8) and every tile where it is not (iteration 1, and 9 .. 12 behind a revert)
    assert a[4] == 12 and b[4] == 12 + 12
    assert a[3] == b[3] == want["recs"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p, q, w in zip(a[2], b[2], want["pts"][-1]):
        assert np.array_equal(p, q)
        assert rel_linf(p, w) <= 1e-13


# ---- 5. DistributedSmoother ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_distributed_smoother_on_one_rank_equals_the_serial_engine(overlap):
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.halo import DistributedSmoother
    from test_gpu_quality_trace import _engine
    m, over = multi_mesh("tiles_411"), MULTI_CASES["tiles_411"][2]
    ser = _engine(m, "com", False, **over)
    ser.set_tangle_constraint(2)
    ser_run = ser.iterate(12, 0.0)
    assert ser_run[0] == 12
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        sub = decompose(m, np.zeros(m.nCells, np.int32), 1)[0]
        ds = DistributedSmoother(sub, device=0, overlap=overlap)
        ds.set_params(default_params(ser.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False, **over))
        ds.set_tangle_constraint(2)
        assert ds.tangle_state().nExemptCells == 0
        n_d, res_d, frz_d = ds.iterate(12, 0.0)
        assert n_d == 12 and np.array_equal(res_d, ser_run[1]) and np.array_equal(frz_d, ser_run[2])   # the loop's own statistics
        recs = ds.tangle_records()
        assert recs == ser.tangle_records() and any(r.nPointsReverted > 0 for r in recs)
        back = np.empty_like(ser.get_points())
        back[sub.pointProcAddressing] = ds.get_points()
        assert np.array_equal(back, ser.get_points())
        ds.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [False, True])
def test_distributed_history_with_a_constraint_that_never_fires(overlap):
    """relTol <= 0 through DistributedSmoother: the stats history is set, so smgpu_iter_end parks the iteration's reduction for the
    next geometry launch (deferN) with the constraint's evaluation queued in between.  The residual and frozen histories, and
    the points, of the run without the constraint, by bits; several geometry tiles, so with an exchange stream the look-ahead is
    live as well."""
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import DistributedSmoother
    from smoothmesh_amd.meshgen import hex_subdomain
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        runs = []
        for on in (False, True):
            ds = DistributedSmoother(hex_subdomain((14, 12, 10), (1, 1, 1), 0, jitter=0.3, seed=5), device=0, overlap=overlap)
            ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
            if on:
                ds.set_tangle_constraint()
            n, res, frz = ds.iterate(9, 0.0)
            assert n == 9
            if on:
                assert _records(ds.tangle_records()) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0) for k in range(1, 10)]
            runs.append((res, frz, ds.get_points()))
            ds.close()
        a, b = runs
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert len(set(a[0].tolist())) == 9              # nine different residuals: a record that slipped by one iteration would show
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["", "push"])
def test_distributed_smoother_two_processes(exchange):
    """One process per rank (torch.distributed.run) with the real engines, two ranks sharing one GPU through the gloo debug
    transport: the count reduced by all_reduce, exchange T staged like exchange F (scripts/check_dist_tangle.py).  "push": the
    peer-store transport, where A and F are stored by the ranks' kernels and T alone still travels by the host's exchange."""
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", SMGPU_PUSH_TIMEOUT_S="10")
    env.pop("SMOOTHMESH_EXCHANGE", None)
    if exchange:
        env["SMOOTHMESH_EXCHANGE"] = exchange
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29543" if exchange else "29541", os.path.join(ROOT, "scripts", "check_dist_tangle.py")],
                       capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok ") == 4 and "BAD" not in r.stdout
    assert r.stdout.count("[peer stores]") == (4 if exchange else 0)


# ---- 6. numbering, clearing, refusals ----------------------------------------------------------------------------------
def test_numbering_across_calls_and_clearing(oracle_lib, monkeypatch):
    want = multi_reference(oracle_lib, "dented_112", "com", False, 2)
    ref = want["ref"]
    ms = _smoother(ref, "com", False, 2, {}, monkeypatch)
    assert ms.iterate(3, 0.0)[0] == 3 and ms.iterate(5, 0.0)[0] == 5
    assert _records(ms.tangle_records()) == want["recs"]
    assert ms.tangle_state().iteration == 8
    # switching it on again restarts the numbering
    ms.set_tangle_constraint(1)
    assert ms.tangle_state().iteration == 0 and ms.tangle_state().passes == 1
    assert ms.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in ms.tangle_records()] == [1, 2]
    ms.clear_tangle_constraint()
    assert not ms.tangle_state().on and ms.tangle_records() == []
    # after switching it off: launch for launch and bit for bit a fresh smoother's iterations from the same points
    fresh = _smoother(ref, "com", False, None, {}, monkeypatch)
    for a, b in zip(ms.states, fresh.states):
        b.eng.set_points(a.eng.get_points())
        a.eng.enable_timing(True), b.eng.enable_timing(True)
        a.eng.reset_counters(), b.eng.reset_counters()
    ra, rb = ms.iterate(4, 0.0), fresh.iterate(4, 0.0)
    assert ra[0] == rb[0] == 4 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    for a, b in zip(ms.states, fresh.states):
        assert np.array_equal(a.eng.get_points(), b.eng.get_points())
        assert {c["name"]: c["launches"] for c in a.eng.counters()} == {c["name"]: c["launches"] for c in b.eng.counters()}
    _close(ms), _close(fresh)


def test_refusals(oracle_lib, monkeypatch):
    import torch
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality_trace import _engine
    want = multi_reference(oracle_lib, "dented_112", "com", False, 2)
    ms = _smoother(want["ref"], "com", False, None, {}, monkeypatch)
    with pytest.raises(SmgpuError, match="passes < 0"):
        ms.set_tangle_constraint(-1)
    assert not ms.tangle_state().on
    eng = ms.states[0].eng
    # the serial entry on an engine with a halo: its old message
    with pytest.raises(SmgpuError, match="not available on an engine with a halo"):
        eng.set_tangle_constraint()
    with pytest.raises(SmgpuError, match="coupled tangle constraint is not on"):
        eng.tangle_pass_begin()
    ms.set_tangle_constraint(2)
    with pytest.raises(SmgpuError, match="smgpu_tangle_pass_end without smgpu_tangle_pass_begin"):
        eng.tangle_pass_end(0)
    with pytest.raises(SmgpuError, match="no iteration waits for its passes"):
        eng.tangle_pass_begin()
    eng.iter_begin()
    with pytest.raises(SmgpuError, match="between smgpu_iter_begin and smgpu_iter_end"):
        eng.set_tangle_constraint_coupled(ms.states[0].sendT.data_ptr(), ms.states[0].recvT.data_ptr(), 2)
    _close(ms)
    # the coupled entry on an engine without a halo
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(SmgpuError, match="the engine has no halo"):
        e.set_tangle_constraint_coupled(t.data_ptr(), t.data_ptr(), 2)
    assert not e.tangle_state().on
    e.close()
    # boundary point smoothing
    from test_gpu_boundary import _decomposed_boundary_case
    from smoothmesh_amd.halo import LocalMultiSmoother
    mo, orcs, subs, prm, set_up = _decomposed_boundary_case(oracle_lib, (2, 1, 1), False, False)
    mb = LocalMultiSmoother(subs, device=0, overlap=False)
    set_up(mb)
    with pytest.raises(SmgpuError, match="boundary point smoothing"):
        mb.set_tangle_constraint()
    _close(mb)
