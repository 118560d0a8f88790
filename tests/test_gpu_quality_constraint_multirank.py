"""The quality constraint on a decomposed mesh (include/smgpu.h smgpu_set_quality_constraint_coupled / smgpu_quality_constraint_pass_*,
csrc/kernels_quality_constraint.hpp k_qc_faces<true>, DESIGN.md "Mesh quality" 10.15) through the two smoothers of halo.py, against
its CPU restatement (tests/quality_constraint_multi_reference.py, pinned against the serial restatement by
tests/test_quality_constraint_multi_reference.py): per-rank and combined records exactly and the points of every iteration at the
project's decomposed tolerance, copies of shared points bit-identical; the invariant through the decomposed report and its sets,
which runs on the same slot table between the iterations; all criteria off against the coupled tangle constraint; a constraint
that never fires; the look-ahead behind a revert; DistributedSmoother on one rank against the serial engine and on two processes;
numbering, clearing and refusals."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_linf
from quality_constraint_multi_reference import FIELDS, OFF, SHARED
from test_gpu_multirank import _copies_identical, _hex_case
from test_gpu_tangle import CASES
from test_quality_constraint_multi_reference import MULTI_CASES, limits_of, multi_mesh, multi_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (variant, the reference's constraints, passes, overlap, environment): as tests/test_gpu_tangle_multirank.py
SETTINGS = [("com", False, 2, False, {}), ("com", True, 2, True, {}), ("org", False, 2, True, {}), ("org", True, 2, False, {}),
            ("com", False, 0, True, {}), ("com", False, 1, False, {}), ("com", False, 2, True, {"SMGPU_TILES": "0"}),
            ("com", False, 2, False, {"SMGPU_GEOM_T": "64"}), ("com", False, 2, True, {"SMGPU_GEOM_T": "256"})]
NEVER = dict(maxNonOrtho=179.9, maxInternalSkewness=1e9, maxBoundarySkewness=1e9)


def _records(recs, fields=FIELDS):
    return [{k: getattr(r, k) for k in fields} for r in recs]


def _smoother(ref, variant, overlap, passes, env, monkeypatch, limits=None, tangle=False):
    from smoothmesh_amd.halo import LocalMultiSmoother
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ms = LocalMultiSmoother(ref.subs, device=0, overlap=overlap)
    for st in ms.states:
        st.eng.set_foam_variant(variant)
    ms.set_params(ref.prm)
    if tangle:
        ms.set_tangle_constraint(passes)
    elif passes is not None:
        ms.set_quality_constraint(passes=passes, **limits)
    return ms


def _close(ms):
    for st in ms.states:
        st.eng.close()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


# ---- 1. the smoother = the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,constraints,passes,overlap,env", SETTINGS)
@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_local_multi_smoother_equals_reference(oracle_lib, monkeypatch, name, variant, constraints, passes, overlap, env):
    from smoothmesh_amd.halo import combine_quality_constraint_records
    n = MULTI_CASES[name][3]
    want = multi_reference(oracle_lib, name, variant, constraints, passes)
    ref = want["ref"]
    lim = limits_of(name)
    ms = _smoother(ref, variant, overlap, passes, env, monkeypatch, lim)
    st = ms.quality_constraint_state()
    assert st.on and st.passes == passes and st.iteration == 0
    assert (st.maxNonOrtho, st.maxInternalSkewness, st.maxBoundarySkewness) == (lim["maxNonOrtho"], lim["maxInternalSkewness"], lim["maxBoundarySkewness"])
    assert st.nExemptCells == sum(ref.nExemptCells) and st.nExemptFaces == sum(ref.nExemptFaces)
    assert [s.eng.quality_constraint_state().nExemptFaces for s in ms.states] == ref.nExemptFaces      # counted once, on the lower rank
    for k in range(n):
        got = ms.iterate(1, 0.0)
        assert got[0] == 1 and int(got[2][0]) == int(want["frz"][k])
        pts = ms.get_points()
        for r, p in enumerate(pts):
            err = rel_linf(p, want["pts"][k][r])
            print(name, k, r, err)
            assert err <= 1e-13, (k, r, err)
        _copies_identical(ref.subs, pts)
    raw = ms.quality_constraint_records(per_rank=True)
    assert [_records(r) for r in raw] == want["per_rank"]
    assert _records(combine_quality_constraint_records(raw)) == want["recs"]
    assert ms.quality_constraint_records() == []                                    # a read clears
    assert ms.quality_constraint_state().iteration == n
    _close(ms)


# ---- 2. the invariant, through the decomposed report and its sets ------------------------------------------------------
@pytest.mark.parametrize("name", ["dented_221", "tiles_611_both", "cavity_811"])
def test_invariant_through_the_report(oracle_lib, monkeypatch, name):
    """after every iteration the coupled report and the coupled sets run on the engines, with a recvCc of their own on the same
    slot table: every face over a limit is an exempt one, on every rank; the same run without the constraint violates that"""
    want = multi_reference(oracle_lib, name, "com", False, 2)
    ref, lim, n = want["ref"], limits_of(name), MULTI_CASES[name][3]
    thr = dict(nonOrthThreshold=min(lim["maxNonOrtho"], 180.0))

    def over_a_limit(ms):
        """per rank the faces over a limit that are not exempt, by the report's sets under the constraint's limits: processor
        faces are judged as internal faces, and are members on the lower rank"""
        si = ms.quality_sets(skewThreshold=lim["maxInternalSkewness"], **thr) if lim["maxInternalSkewness"] > 0.0 or lim["maxNonOrtho"] < 180.0 else None
        sb = ms.quality_sets(skewThreshold=lim["maxBoundarySkewness"], **thr) if lim["maxBoundarySkewness"] > 0.0 else None
        out = []
        for r, s in enumerate(ref.subs):
            F, Fi = s.mesh.nFaces, s.mesh.nInternalFaces
            proc = np.zeros(F, bool)
            for st, sz, _ in ref.couplings[r][1]:
                proc[st:st + sz] = True
            inner = proc.copy()
            inner[:Fi] = True
            bad = np.zeros(F, bool)
            if lim["maxNonOrtho"] < 180.0:
                bad[si[r]["nonOrthoFaces"]] = True
            if lim["maxInternalSkewness"] > 0.0:
                f = si[r]["skewFaces"]
                bad[f[inner[f]]] = True
            if lim["maxBoundarySkewness"] > 0.0:
                f = sb[r]["skewFaces"]
                bad[f[~inner[f]]] = True
            out.append(int((bad & ~ref.exemptFaces[r]).sum()))
        return out

    ms = _smoother(ref, "com", True, 2, {}, monkeypatch, lim)
    q0 = ms.mesh_quality(skewThreshold=max(lim["maxInternalSkewness"], 1e-300), **thr)
    for k in range(n):
        assert ms.iterate(1, 0.0)[0] == 1
        q = ms.mesh_quality(skewThreshold=max(lim["maxInternalSkewness"], 1e-300), **thr)
        assert q.nNonPositiveVolume <= q0.nNonPositiveVolume and q.nWrongOrientedFaces <= q0.nWrongOrientedFaces
        assert over_a_limit(ms) == [0] * len(ref.subs), k
        for r, p in enumerate(ms.get_points()):                                      # the reports left the run as it was
            assert rel_linf(p, want["pts"][k][r]) <= 1e-13
    assert _records(ms.quality_constraint_records()) == want["recs"]
    assert any(r["nNonOrthoFaces"] + r["nSkewFaces"] > 0 for r in want["recs"])
    # ... and without the constraint the same run goes over a limit
    free = _smoother(ref, "com", True, None, {}, monkeypatch)
    assert free.iterate(n, 0.0)[0] == n
    assert sum(over_a_limit(free)) > 0
    _close(ms), _close(free)


# ---- 3. all criteria off: the coupled tangle constraint ------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name", ["dented_221", "tiles_431"])
def test_all_criteria_off_is_the_coupled_tangle_constraint(oracle_lib, monkeypatch, name, overlap):
    want = multi_reference(oracle_lib, name, "com", False, 2)
    n = MULTI_CASES[name][3]
    a = _smoother(want["ref"], "com", overlap, 2, {}, monkeypatch, OFF)
    b = _smoother(want["ref"], "com", overlap, 2, {}, monkeypatch, tangle=True)
    ra, rb = a.iterate(n, 0.0), b.iterate(n, 0.0)
    assert ra[0] == rb[0] == n and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    for p, q in zip(a.get_points(), b.get_points()):
        assert np.array_equal(p, q)
    qa, tb = a.quality_constraint_records(per_rank=True), b.tangle_records(per_rank=True)
    assert [_records(r, SHARED) for r in qa] == [_records(r, SHARED) for r in tb]
    assert any(r.nBadCells > 0 for rr in tb for r in rr)
    assert all(r.nTangledCells == r.nBadCells and r.nNonOrthoFaces == r.nSkewFaces == 0 for rr in qa for r in rr)
    _close(a), _close(b)


# ---- 4. a constraint that never fires leaves the run untouched ---------------------------------------------------------
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
            ms.set_quality_constraint(**NEVER)
            st = ms.quality_constraint_state()
            assert st.nExemptCells == 0 and st.nExemptFaces == 0
        ms.states[0].eng.enable_timing(True)
        n, res, frz = ms.iterate(8, 0.0)
        assert n == 8
        geom = {c["name"]: c["launches"] for c in ms.states[0].eng.counters()}["k_geom_tile"]
        if not layers:
            assert geom == 16                              # 1 + 7 + 8: the look-ahead is live (tests/test_gpu_multirank.py)
        if on:
            assert _records(ms.quality_constraint_records()) == [dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0, nTangledCells=0,
                                                                       nNonOrthoFaces=0, nSkewFaces=0) for k in range(1, 9)]
        runs.append((res, frz, ms.get_points(), geom))
        _close(ms)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


# ---- 5. the look-ahead while points are reverted -----------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SMGPU_GEOM_T": "64"}])
def test_look_ahead_geometry_is_not_trusted_behind_a_revert(oracle_lib, monkeypatch, env):
    """dented_block_tiles() cut (6, 1, 1) with an exchange stream: smgpu_iter_ahead is active while points are reverted.  The bits
    of the run in order, where no geometry is computed ahead."""
    want = multi_reference(oracle_lib, "tiles_611", "com", False, 2)
    out = {}
    for overlap in (False, True):
        ms = _smoother(want["ref"], "com", overlap, 2, env, monkeypatch, limits_of("tiles_611"))
        n, res, frz = ms.iterate(12, 0.0)
        assert n == 12
        out[overlap] = (res, frz, ms.get_points(), _records(ms.quality_constraint_records()))
        _close(ms)
    a, b = out[False], out[True]
    assert a[3] == b[3] == want["recs"] and any(r["nPointsReverted"] > 0 for r in a[3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


# ---- 6. DistributedSmoother ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relTol", [0.0, 1e-300])
@pytest.mark.parametrize("overlap", [False, True])
def test_distributed_smoother_on_one_rank_equals_the_serial_engine(overlap, relTol):
    """relTol <= 0: the stats history is set and the iteration's reduction is parked behind the passes; relTol > 0 (never met): the
    host reads the residual every iteration"""
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.halo import DistributedSmoother
    from test_gpu_quality_trace import _engine
    m, over, lim = multi_mesh("tiles_611_both"), CASES["dented_tiles"][1], limits_of("tiles_611_both")
    ser = _engine(m, "com", False, **over)
    ser.set_quality_constraint(passes=2, **lim)
    ser_run = ser.iterate(12, relTol)
    assert ser_run[0] == 12
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        sub = decompose(m, np.zeros(m.nCells, np.int32), 1)[0]
        ds = DistributedSmoother(sub, device=0, overlap=overlap)
        ds.set_params(default_params(ser.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False, **over))
        ds.set_quality_constraint(passes=2, **lim)
        sd, ss = ds.quality_constraint_state(), ser.quality_constraint_state()
        assert (sd.nExemptCells, sd.nExemptFaces) == (ss.nExemptCells, ss.nExemptFaces) and sd.nExemptFaces > 0
        n_d, res_d, frz_d = ds.iterate(12, relTol)
        assert n_d == 12 and np.array_equal(res_d, ser_run[1]) and np.array_equal(frz_d, ser_run[2])   # the loop's own statistics
        recs = ds.quality_constraint_records()
        assert recs == ser.quality_constraint_records() and any(r.fullRevert for r in recs) and any(r.nPointsReverted > 0 for r in recs)
        back = np.empty_like(ser.get_points())
        back[sub.pointProcAddressing] = ds.get_points()
        assert np.array_equal(back, ser.get_points())
        ds.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["", "push"])
def test_distributed_smoother_two_processes(tmp_path, exchange):
    """One process per rank with the real engines, two ranks sharing one GPU through the gloo debug transport, each under a time
    limit of its own: Cc moved by _quality_swap, the count reduced by all_reduce, exchange T staged like exchange F
    (scripts/check_dist_quality_constraint.py).  "push": the peer-store transport, where Cc and T still travel by the host."""
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", SMGPU_PUSH_TIMEOUT_S="10",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    env.pop("SMOOTHMESH_EXCHANGE", None)
    if exchange:
        env["SMOOTHMESH_EXCHANGE"] = exchange
    script = os.path.join(ROOT, "scripts", "check_dist_quality_constraint.py")
    procs = []
    for rank in range(2):
        with open(tmp_path / f"rank{rank}.txt", "w") as f:
            procs.append(subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, script], stdout=f, stderr=subprocess.STDOUT,
                                          env=dict(env, RANK=str(rank), LOCAL_RANK=str(rank))))
    codes = [p.wait() for p in procs]
    out = "".join((tmp_path / f"rank{rank}.txt").read_text() for rank in range(2))
    print(out)
    assert codes == [0, 0], out[-6000:]
    assert out.count(": ok ") == 4 and "BAD" not in out
    assert out.count("[peer stores]") == (4 if exchange else 0)


# ---- 7. numbering, clearing, refusals ----------------------------------------------------------------------------------
def test_numbering_across_calls_and_clearing(oracle_lib, monkeypatch):
    want = multi_reference(oracle_lib, "dented_211", "com", False, 2)
    ref, lim = want["ref"], limits_of("dented_211")
    ms = _smoother(ref, "com", False, 2, {}, monkeypatch, lim)
    assert ms.iterate(3, 0.0)[0] == 3 and ms.iterate(5, 0.0)[0] == 5
    assert _records(ms.quality_constraint_records()) == want["recs"]
    assert ms.quality_constraint_state().iteration == 8
    # switching it on again restarts the numbering
    ms.set_quality_constraint(passes=1, **lim)
    assert ms.quality_constraint_state().iteration == 0 and ms.quality_constraint_state().passes == 1
    assert ms.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in ms.quality_constraint_records()] == [1, 2]
    ms.clear_quality_constraint()
    assert not ms.quality_constraint_state().on and ms.quality_constraint_records() == []
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
    want = multi_reference(oracle_lib, "dented_211", "com", False, 2)
    lim = limits_of("dented_211")
    ms = _smoother(want["ref"], "com", False, None, {}, monkeypatch)
    with pytest.raises(SmgpuError, match="passes < 0"):
        ms.set_quality_constraint(passes=-1)
    with pytest.raises(SmgpuError, match="a limit is NaN"):
        ms.set_quality_constraint(maxInternalSkewness=float("nan"))
    assert not ms.quality_constraint_state().on
    s0 = ms.states[0]
    eng = s0.eng
    # the serial entry on an engine with a halo: its old message; the trace and the guard stay refused there
    with pytest.raises(SmgpuError, match="not available on an engine with a halo"):
        eng.set_quality_constraint()
    with pytest.raises(SmgpuError, match="not available on an engine with a halo"):
        eng.set_quality_trace(1)
    with pytest.raises(SmgpuError):
        eng.set_quality_guard()
    # calls out of order
    with pytest.raises(SmgpuError, match="coupled quality constraint is not on"):
        eng.quality_constraint_pass_begin()
    with pytest.raises(SmgpuError, match="no coupled quality constraint waits for its exempt faces"):
        eng.quality_constraint_coupled_exempt()
    # a null buffer that is needed
    coupling = eng.quality_coupling(0)
    assert coupling[1]
    with pytest.raises(SmgpuError, match="null exchange buffer"):
        eng.set_quality_constraint_coupled(coupling, s0.sendF.data_ptr(), s0.recvF.data_ptr(), 0, 0)
    with pytest.raises(SmgpuError, match="null exchange buffer"):
        eng.set_quality_constraint_coupled(coupling, 0, s0.recvF.data_ptr(), s0.sendA.data_ptr(), s0.recvA.data_ptr())
    # two patches to one neighbour, as the coupled report
    st, sz, nb = coupling[1][0]
    with pytest.raises(SmgpuError, match="two processor patches to rank"):
        eng.set_quality_constraint_coupled((0, [(st, sz - 1, nb), (st + sz - 1, 1, nb)]), s0.sendF.data_ptr(), s0.recvF.data_ptr(),
                                           s0.sendA.data_ptr(), s0.recvA.data_ptr())
    assert not eng.quality_constraint_state().on
    # pending: the exempt faces have not been taken
    ms.set_quality_constraint(**lim)
    eng.set_quality_constraint_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr(), **lim)
    assert not eng.quality_constraint_state().on
    with pytest.raises(SmgpuError, match="waits for its exempt faces"):
        eng.iter_begin()
    with pytest.raises(SmgpuError, match="the exempt faces have not been taken"):
        eng.quality_constraint_pass_begin()
    ms.set_quality_constraint(**lim)
    assert ms.quality_constraint_state().on
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_end without smgpu_quality_constraint_pass_faces"):
        eng.quality_constraint_pass_end(0)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_faces without smgpu_quality_constraint_pass_begin"):
        eng.quality_constraint_pass_faces()
    with pytest.raises(SmgpuError, match="no iteration waits for its passes"):
        eng.quality_constraint_pass_begin()
    # the two constraints together, in either order, and a new halo under the constraint
    with pytest.raises(SmgpuError, match="the quality constraint is on"):
        eng.set_tangle_constraint_coupled(s0.sendT.data_ptr(), s0.recvT.data_ptr(), 2)
    with pytest.raises(RuntimeError, match="the quality constraint is on"):
        ms.set_tangle_constraint()
    t = s0.t
    with pytest.raises(SmgpuError, match="smgpu_halo_configure: the coupled quality constraint is on"):
        eng.halo_configure(t.sharedLocal, t.sendShared, t.nRecv, t.combOffsets, t.combSlots, s0.sendA.data_ptr(), s0.recvA.data_ptr(),
                           s0.sendF.data_ptr(), s0.recvF.data_ptr(), s0.localStats.data_ptr(), sendL=s0.sendL.data_ptr(), recvL=s0.recvL.data_ptr())
    ms.clear_quality_constraint()
    ms.set_tangle_constraint()
    with pytest.raises(RuntimeError, match="the tangle constraint is on"):
        ms.set_quality_constraint()
    with pytest.raises(SmgpuError, match="the tangle constraint is on"):
        eng.set_quality_constraint_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr())
    ms.clear_tangle_constraint()
    # between smgpu_iter_begin and smgpu_iter_end; and smgpu_iter_begin while passes are due
    ms.set_quality_constraint(**lim)
    eng.iter_begin()
    with pytest.raises(SmgpuError, match="between smgpu_iter_begin and smgpu_iter_end"):
        eng.set_quality_constraint_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr())
    _close(ms)
    # the coupled entry on an engine without a halo
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    z = torch.zeros(16, dtype=torch.float64, device="cuda")
    with pytest.raises(SmgpuError, match="the engine has no halo"):
        e.set_quality_constraint_coupled((0, []), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert not e.quality_constraint_state().on
    e.close()
    # boundary point smoothing
    from test_gpu_boundary import _decomposed_boundary_case
    from smoothmesh_amd.halo import LocalMultiSmoother
    mo, orcs, subs, prm, set_up = _decomposed_boundary_case(oracle_lib, (2, 1, 1), False, False)
    mb = LocalMultiSmoother(subs, device=0, overlap=False)
    set_up(mb)
    with pytest.raises(SmgpuError, match="boundary point smoothing"):
        mb.set_quality_constraint()
    _close(mb)


def test_passes_are_due_before_the_next_iteration(oracle_lib, monkeypatch):
    from smoothmesh_amd import SmgpuError
    want = multi_reference(oracle_lib, "dented_211", "com", False, 2)
    ms = _smoother(want["ref"], "com", False, 2, {}, monkeypatch, limits_of("dented_211"))
    for st in ms.states:
        st.eng.iter_begin()
    for st in ms.states:
        st.eng.iter_interior()
    ms._exchange("A")
    for st in ms.states:
        st.eng.iter_mid()
    for st in ms.states:
        st.eng.iter_ahead()
    ms._exchange("F")
    for st in ms.states:
        st.eng.iter_end()
    eng = ms.states[0].eng
    with pytest.raises(SmgpuError, match="has not finished the passes of the last iteration"):
        eng.iter_begin()
    with pytest.raises(SmgpuError, match="between the passes of an iteration"):
        eng.quality_constraint_records()
    eng.quality_constraint_pass_begin()
    with pytest.raises(SmgpuError, match="the pass in hand has not been closed"):
        eng.quality_constraint_pass_begin()
    ms.states[1].eng.quality_constraint_pass_begin()
    ms._move_cc()
    total = sum(st.eng.quality_constraint_pass_faces() for st in ms.states)
    with pytest.raises(SmgpuError, match="nBadGlobal < 0"):
        eng.quality_constraint_pass_end(-1)
    assert total == want["recs"][0]["nBadCells"] > 0
    _close(ms)
