"""The quality constraint's tet, twist, weight, ratio and determinant limits on a decomposed mesh (include/smgpu.h
smgpu_set_quality_constraint_limits_coupled, csrc/kernels_quality_limits.hpp Coupled = true, DESIGN.md "Mesh quality" 10.17) through the two
smoothers of halo.py, against the CPU restatement (tests/quality_constraint_full_multi_reference.py, pinned against the serial
restatement by tests/test_quality_constraint_full_multi_reference.py): per-rank and combined full records exactly, the per-rank
exempt counts, the points of every iteration at the project's decomposed tolerance, copies of shared points bit-identical; the
invariant through the decomposed -allGeometry and -meshQuality sets at the constraint's limits; all six off against the old coupled
entry, launch counters included; one rank through DistributedSmoother against the serial engine by bits; a constraint that never
fires; numbering, clearing, refusals; two gloo processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_linf
from quality_constraint_full_multi_reference import FIELDS_FULL, MORE
from quality_constraint_multi_reference import FIELDS, OFF
from test_gpu_multirank import _copies_identical, _hex_case
from test_gpu_quality_constraint_multirank import _close, _free_port, _records
from test_quality_constraint_full_multi_reference import FULL_MULTI_CASES, _over_and_n, full_limits_of, full_multi_mesh, full_multi_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every row under the first setting; the two rows whose processor faces fail all five face criteria, and the volume ratio alone,
# under the others: (variant, the reference's constraints, passes, environment)
FIRST = ("com", False, 2, {})
OTHERS = [("com", True, 2, {}), ("org", False, 2, {}), ("org", True, 2, {}), ("com", False, 0, {}), ("com", False, 1, {}),
          ("com", False, 2, {"SMGPU_TILES": "0"}), ("com", False, 2, {"SMGPU_GEOM_T": "64"}), ("com", False, 2, {"SMGPU_GEOM_T": "256"})]
RUNS = [(name, *FIRST) for name in FULL_MULTI_CASES] + [(name, *s) for s in OTHERS for name in ("all_811", "ratio_811")]
NEVER = dict(maxNonOrtho=179.9, maxInternalSkewness=1e9, maxBoundarySkewness=1e9, minTetQuality=-1e9, minTwist=-0.999, minTriangleTwist=-0.999,
             minFaceWeight=1e-9, minVolRatio=1e-9, minDeterminant=1e-12)


def _split(lim):
    """the limits as set_quality_constraint_limits takes them: a new limit at its off value becomes None"""
    return {k: (None if k in MORE and v is not None and v <= MORE[k][0] else v) for k, v in lim.items()}


def _smoother(ref, variant, passes, env, monkeypatch, limits=None, old=False, overlap=False):
    from smoothmesh_amd.halo import LocalMultiSmoother
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ms = LocalMultiSmoother(ref.subs, device=0, overlap=overlap)
    for st in ms.states:
        st.eng.set_foam_variant(variant)
    ms.set_params(ref.prm)
    if old:
        ms.set_quality_constraint(passes=passes, **limits)
    elif passes is not None:
        ms.set_quality_constraint_limits(passes=passes, **_split(limits))
    return ms


# ---- 1. the smoother = the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,constraints,passes,env", RUNS)
def test_local_multi_smoother_equals_reference(oracle_lib, monkeypatch, name, variant, constraints, passes, env):
    from smoothmesh_amd.halo import combine_quality_constraint_records
    n = _over_and_n(name)[1]
    want = full_multi_reference(oracle_lib, name, variant, constraints, passes)
    ref, lim = want["ref"], full_limits_of(name)
    ms = _smoother(ref, variant, passes, env, monkeypatch, lim)
    st = ms.quality_constraint_state()
    assert st.on and st.passes == passes and st.iteration == 0
    assert all(getattr(st, k) == ref.more[k] for k in MORE)
    assert st.nExemptCells == sum(ref.nExemptCells) and st.nExemptFaces == sum(ref.nExemptFaces)
    assert st.nExemptDeterminantCells == sum(ref.nExemptDeterminantCells)
    per = [s.eng.quality_constraint_state() for s in ms.states]
    assert [s.nExemptFaces for s in per] == ref.nExemptFaces                      # counted once, on the lower rank
    assert [s.nExemptDeterminantCells for s in per] == ref.nExemptDeterminantCells     # the rank's own
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
    assert [_records(r, FIELDS_FULL) for r in raw] == want["per_rank"]
    assert _records(combine_quality_constraint_records(raw), FIELDS_FULL) == want["recs"]
    assert ms.quality_constraint_records() == []                                    # a read clears
    assert ms.quality_constraint_state().iteration == n
    _close(ms)


# ---- 2. the invariant, through the decomposed reports' sets ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_811", "determinant_811"])
def test_invariant_through_the_report_sets(oracle_lib, monkeypatch, name):
    """after every iteration the decomposed -allGeometry and -meshQuality sets run on the engines at the constraint's limits, with
    exchange buffers of their own: every face and cell under a limit is an exempt one, on every rank; the same run without the
    constraint violates that"""
    want = full_multi_reference(oracle_lib, name, "com", False, 2)
    ref, lim, n = want["ref"], full_limits_of(name), _over_and_n(name)[1]

    def under_a_limit(ms):
        more = ref.more                                                              # (a limit that is off: its off value, which no value is under)
        g = ms.quality_geometry_sets(weightThreshold=more["minFaceWeight"], volRatioThreshold=more["minVolRatio"], determinantThreshold=more["minDeterminant"])
        t = ms.quality_motion_sets(tetThreshold=more["minTetQuality"], twistThreshold=more["minTwist"], triangleTwistThreshold=more["minTriangleTwist"])
        out = []
        for r, s in enumerate(ref.subs):
            bad = np.zeros(s.mesh.nFaces, bool)
            for sets, names in ((g, ("lowWeightFaces", "lowVolRatioFaces")), (t, ("lowQualityTetFaces", "twistedFaces", "lowTriangleTwistFaces"))):
                for nm in names:
                    bad[sets[r][nm]] = True
            cells = np.zeros(s.mesh.nCells, bool)
            cells[g[r]["underdeterminedCells"]] = True
            out.append(int((bad & ~ref.exemptFaces[r]).sum()) + int((cells & ~ref.exemptDet[r]).sum()))
        return out

    ms = _smoother(ref, "com", 2, {}, monkeypatch, lim)
    for k in range(n):
        assert ms.iterate(1, 0.0)[0] == 1
        assert under_a_limit(ms) == [0] * len(ref.subs), k
        for r, p in enumerate(ms.get_points()):                                      # the reports left the run as it was
            assert rel_linf(p, want["pts"][k][r]) <= 1e-13
    assert _records(ms.quality_constraint_records(), FIELDS_FULL) == want["recs"]
    assert any(sum(r[MORE[k][1]] for k in MORE) > 0 for r in want["recs"])
    # ... and without the constraint the same run goes under a limit
    free = _smoother(ref, "com", None, {}, monkeypatch)
    assert free.iterate(n, 0.0)[0] == n
    assert sum(under_a_limit(free)) > 0
    _close(ms), _close(free)


# ---- 3. equivalence (a): all six off through the new entry is the old coupled entry ----------------------------------------
@pytest.mark.parametrize("env", [{}, {"SMGPU_TILES": "0"}])
def test_all_six_off_is_the_old_coupled_entry(oracle_lib, monkeypatch, env):
    from test_quality_constraint_multi_reference import MULTI_CASES, limits_of, multi_reference
    name = "cavity_811"
    want = multi_reference(oracle_lib, name, "com", False, 2)
    n, lim = MULTI_CASES[name][3], limits_of(name)
    a = _smoother(want["ref"], "com", 2, env, monkeypatch, {**lim, **{k: None for k in MORE}})
    b = _smoother(want["ref"], "com", 2, env, monkeypatch, lim, old=True)
    sa, sb = a.quality_constraint_state(), b.quality_constraint_state()
    assert sa == sb and sa.nExemptDeterminantCells == 0
    for x in a.states + b.states:
        x.eng.enable_timing(True)
        x.eng.reset_counters()
    ra, rb = a.iterate(n, 0.0), b.iterate(n, 0.0)
    assert ra[0] == rb[0] == n and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    for p, q in zip(a.get_points(), b.get_points()):
        assert np.array_equal(p, q)
    for x, y in zip(a.states, b.states):
        assert {c["name"]: c["launches"] for c in x.eng.counters()} == {c["name"]: c["launches"] for c in y.eng.counters()}
    qa, qb = a.quality_constraint_records(per_rank=True), b.quality_constraint_records(per_rank=True)
    assert qa == qb and [_records(r) for r in qa] == want["per_rank"]
    assert any(r.nNonOrthoFaces + r.nSkewFaces > 0 for rr in qa for r in rr)
    assert all(getattr(r, MORE[k][1]) == 0 for rr in qa for r in rr for k in MORE)
    assert a.quality_constraint_state() == b.quality_constraint_state()
    _close(a), _close(b)


def test_old_coupled_entry_leaves_the_six_new_counts_zero(oracle_lib, monkeypatch):
    """under smgpu_set_quality_constraint_coupled one close kernel writes the whole slot: dented_tiles cut (6, 1, 1), which ends
    iterations with reverting passes and with the full revert, drained through the full getter: the six counts of 10.16 are
    exactly 0 in every record of every rank"""
    from test_quality_constraint_multi_reference import MULTI_CASES, limits_of, multi_reference
    name = "tiles_611_both"
    want = multi_reference(oracle_lib, name, "com", False, 2)
    n = MULTI_CASES[name][3]
    ms = _smoother(want["ref"], "com", 2, {}, monkeypatch, limits_of(name), old=True)
    assert ms.iterate(n, 0.0)[0] == n
    raw = ms.quality_constraint_records(per_rank=True)                          # (smgpu_get_quality_constraint_records_full)
    assert [_records(r) for r in raw] == want["per_rank"]
    assert any(r.fullRevert for rr in raw for r in rr) and any(r.passes > 0 and not r.fullRevert for rr in raw for r in rr)
    assert all(getattr(r, MORE[k][1]) == 0 for rr in raw for r in rr for k in MORE)
    _close(ms)


# ---- 4. a constraint that is on and never fires leaves the run untouched ---------------------------------------------------
def test_constraint_that_never_fires_leaves_the_run_untouched(oracle_lib):
    """(16, 12, 12) sub-domains cut (2, 2, 1) with an exchange stream: several geometry tiles per rank, so smgpu_iter_ahead
    recomputes the interior ones for the next iteration while the passes are still to come"""
    from smoothmesh_amd.halo import LocalMultiSmoother
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 1), (16, 12, 12), False)
    runs = []
    for on in (False, True):
        ms = LocalMultiSmoother(subs, device=0, overlap=True)
        ms.set_params(prm)
        if on:
            ms.set_quality_constraint_limits(**NEVER)
            st = ms.quality_constraint_state()
            assert st.on and st.nExemptCells == 0 and st.nExemptFaces == 0 and st.nExemptDeterminantCells == 0 and st.minVolRatio == 1e-9
        ms.states[0].eng.enable_timing(True)
        n, res, frz = ms.iterate(8, 0.0)
        assert n == 8
        geom = {c["name"]: c["launches"] for c in ms.states[0].eng.counters()}["k_geom_tile"]
        assert geom == 16                                  # 1 + 7 + 8: the look-ahead is live (tests/test_gpu_multirank.py)
        if on:
            assert _records(ms.quality_constraint_records(), FIELDS_FULL) == [dict(dict.fromkeys(FIELDS_FULL, 0), iteration=k) for k in range(1, 9)]
        runs.append((res, frz, ms.get_points(), geom))
        _close(ms)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


# ---- 5. equivalence (b): DistributedSmoother on one rank is the serial engine ------------------------------------------------
@pytest.mark.parametrize("relTol", [0.0, 1e-300])
def test_distributed_smoother_on_one_rank_equals_the_serial_engine(relTol):
    """relTol <= 0: the iteration's reduction is parked behind the passes; relTol > 0 (never met): the host reads the residual
    every iteration"""
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.halo import DistributedSmoother
    from test_gpu_quality_trace import _engine
    name = "all_811"
    m, (over, n), lim = full_multi_mesh(name), _over_and_n(name), _split(full_limits_of(name))
    ser = _engine(m, "com", False, **over)
    ser.set_quality_constraint(passes=2, **lim)
    ser_run = ser.iterate(n, relTol)
    assert ser_run[0] == n
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        sub = decompose(m, np.zeros(m.nCells, np.int32), 1)[0]
        ds = DistributedSmoother(sub, device=0, overlap=False)
        ds.set_params(default_params(ser.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False, **over))
        with pytest.raises(ValueError, match="minVolRatio is not available on a decomposed mesh"):
            ds.set_quality_constraint(passes=2, minVolRatio=0.1)
        ds.set_quality_constraint_limits(passes=2, **lim)
        sd, ss = ds.quality_constraint_state(), ser.quality_constraint_state()
        assert ss.iteration == n and sd.iteration == 0
        ss.iteration = 0                                       # (the serial engine has run already)
        assert sd == ss and sd.nExemptFaces > 0 and sd.nExemptDeterminantCells > 0
        n_d, res_d, frz_d = ds.iterate(n, relTol)
        assert n_d == n and np.array_equal(res_d, ser_run[1]) and np.array_equal(frz_d, ser_run[2])   # the loop's own statistics
        recs = ds.quality_constraint_records()
        assert recs == ser.quality_constraint_records() and any(r.nPointsReverted > 0 for r in recs)
        assert any(r.nLowVolRatioFaces > 0 for r in recs) and any(r.nLowWeightFaces > 0 for r in recs) and any(r.nLowTetFaces > 0 for r in recs)
        back = np.empty_like(ser.get_points())
        back[sub.pointProcAddressing] = ds.get_points()
        assert np.array_equal(back, ser.get_points())
        ds.close()
    finally:
        dist.destroy_process_group()


def test_distributed_smoother_two_processes(tmp_path):
    """One process per rank with the real engines, two ranks sharing one GPU through the gloo debug transport, each a fresh child
    under a time limit of its own: Cc and Vc moved by _quality_swap (scripts/check_dist_quality_constraint_limits.py)"""
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    env.pop("SMOOTHMESH_EXCHANGE", None)
    script = os.path.join(ROOT, "scripts", "check_dist_quality_constraint_limits.py")
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


# ---- 6. numbering, clearing, refusals ----------------------------------------------------------------------------------
def test_numbering_across_calls_and_clearing(oracle_lib, monkeypatch):
    name = "ratio_811"
    want = full_multi_reference(oracle_lib, name, "com", False, 2)
    ref, lim, n = want["ref"], full_limits_of(name), _over_and_n(name)[1]
    ms = _smoother(ref, "com", 2, {}, monkeypatch, lim)
    assert ms.iterate(3, 0.0)[0] == 3 and ms.iterate(n - 3, 0.0)[0] == n - 3
    assert _records(ms.quality_constraint_records(), FIELDS_FULL) == want["recs"]
    assert ms.quality_constraint_state().iteration == n
    # switching it on again restarts the numbering; the old entry on the same object keeps its refusal, and takes over when asked
    ms.set_quality_constraint_limits(passes=1, **_split(lim))
    assert ms.quality_constraint_state().iteration == 0 and ms.quality_constraint_state().passes == 1
    assert ms.iterate(2, 0.0)[0] == 2
    assert [r.iteration for r in ms.quality_constraint_records()] == [1, 2]
    with pytest.raises(ValueError, match="set_quality_constraint: minVolRatio is not available on a decomposed mesh"):
        ms.set_quality_constraint(minVolRatio=0.11)
    assert ms.quality_constraint_state().on and ms.quality_constraint_state().minVolRatio == 0.11
    ms.clear_quality_constraint()
    st = ms.quality_constraint_state()
    assert not st.on and st.minVolRatio == 0.0 and st.nExemptDeterminantCells == 0 and ms.quality_constraint_records() == []
    # after switching it off: launch for launch and bit for bit a fresh smoother's iterations from the same points
    fresh = _smoother(ref, "com", None, {}, monkeypatch)
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
    name = "ratio_811"
    want = full_multi_reference(oracle_lib, name, "com", False, 2)
    lim = _split(full_limits_of(name))
    ms = _smoother(want["ref"], "com", None, {}, monkeypatch)
    api = "smgpu_set_quality_constraint_limits_coupled"
    with pytest.raises(SmgpuError, match=api + ": passes < 0"):
        ms.set_quality_constraint_limits(passes=-1)
    for k in ("maxInternalSkewness", *MORE):
        with pytest.raises(SmgpuError, match=api + ": a limit is NaN"):
            ms.set_quality_constraint_limits(**{k: float("nan")})
    assert not ms.quality_constraint_state().on
    s0 = ms.states[0]
    eng = s0.eng
    coupling = eng.quality_coupling(0)
    assert coupling[1]
    z = torch.zeros(4096, dtype=torch.float64, device="cuda")
    bufs = (s0.sendF.data_ptr(), s0.recvF.data_ptr(), s0.sendA.data_ptr(), s0.recvA.data_ptr())
    # a null buffer that is needed: Cc always, Vc while minVolRatio is on and only then
    with pytest.raises(SmgpuError, match=api + ": null exchange buffer"):
        eng.set_quality_constraint_limits_coupled(coupling, bufs[0], bufs[1], 0, 0)
    with pytest.raises(SmgpuError, match=api + ": null exchange buffer"):
        eng.set_quality_constraint_limits_coupled(coupling, 0, bufs[1], bufs[2], bufs[3])
    for vc in ((0, 0), (z.data_ptr(), 0), (0, z.data_ptr())):
        with pytest.raises(SmgpuError, match=api + r": null exchange buffer \(minVolRatio is on"):
            eng.set_quality_constraint_limits_coupled(coupling, *bufs, *vc, minVolRatio=0.1)
    assert not eng.quality_constraint_state().on
    # two patches to one neighbour, as the coupled report
    st, sz, nb = coupling[1][0]
    with pytest.raises(SmgpuError, match="two processor patches to rank"):
        eng.set_quality_constraint_limits_coupled((0, [(st, sz - 1, nb), (st + sz - 1, 1, nb)]), *bufs)
    # pending: the exempt faces have not been taken; the serial entries keep refusing an engine with a halo
    ms.set_quality_constraint_limits(**lim)
    eng.set_quality_constraint_limits_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr(),
                                              s0.sendVc.data_ptr(), s0.recvVc.data_ptr(), **lim)
    assert not eng.quality_constraint_state().on
    with pytest.raises(SmgpuError, match="waits for its exempt faces"):
        eng.iter_begin()
    with pytest.raises(SmgpuError, match="the exempt faces have not been taken"):
        eng.quality_constraint_pass_begin()
    with pytest.raises(SmgpuError, match="not available on an engine with a halo"):
        eng.set_quality_constraint(minVolRatio=0.1)
    ms.set_quality_constraint_limits(**lim)
    assert ms.quality_constraint_state().on
    # the other entry while this one is on, and the other way round; the tangle forms, in either order; a new halo
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_coupled: the quality constraint is on through smgpu_set_quality_constraint_limits_coupled"):
        eng.set_quality_constraint_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr())
    with pytest.raises(SmgpuError, match="the quality constraint is on"):
        eng.set_tangle_constraint_coupled(s0.sendT.data_ptr(), s0.recvT.data_ptr(), 2)
    with pytest.raises(RuntimeError, match="the quality constraint is on"):
        ms.set_tangle_constraint()
    t = s0.t
    with pytest.raises(SmgpuError, match="smgpu_halo_configure: the coupled quality constraint is on"):
        eng.halo_configure(t.sharedLocal, t.sendShared, t.nRecv, t.combOffsets, t.combSlots, s0.sendA.data_ptr(), s0.recvA.data_ptr(),
                           s0.sendF.data_ptr(), s0.recvF.data_ptr(), s0.localStats.data_ptr(), sendL=s0.sendL.data_ptr(), recvL=s0.recvL.data_ptr())
    ms.clear_quality_constraint()
    ms.set_quality_constraint(**{k: v for k, v in lim.items() if k not in MORE})
    with pytest.raises(SmgpuError, match=api + ": the quality constraint is on through smgpu_set_quality_constraint_coupled"):
        eng.set_quality_constraint_limits_coupled(coupling, s0.sendT.data_ptr(), s0.recvT.data_ptr(), s0.sendCc.data_ptr(), s0.recvCc.data_ptr())
    ms.clear_quality_constraint()
    ms.set_tangle_constraint()
    with pytest.raises(RuntimeError, match="the tangle constraint is on"):
        ms.set_quality_constraint_limits()
    with pytest.raises(SmgpuError, match=api + ": the tangle constraint is on"):
        eng.set_quality_constraint_limits_coupled(coupling, *bufs)
    ms.clear_tangle_constraint()
    # between smgpu_iter_begin and smgpu_iter_end
    ms.set_quality_constraint_limits(**lim)
    eng.iter_begin()
    with pytest.raises(SmgpuError, match=api + ": between smgpu_iter_begin and smgpu_iter_end"):
        eng.set_quality_constraint_limits_coupled(coupling, *bufs)
    _close(ms)
    # an engine without a halo
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    with pytest.raises(SmgpuError, match=api + ": the engine has no halo"):
        e.set_quality_constraint_limits_coupled((0, []), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert not e.quality_constraint_state().on
    e.close()
    # boundary point smoothing
    from test_gpu_boundary import _decomposed_boundary_case
    from smoothmesh_amd.halo import LocalMultiSmoother
    mo, orcs, subs, prm, set_up = _decomposed_boundary_case(oracle_lib, (2, 1, 1), False, False)
    mb = LocalMultiSmoother(subs, device=0, overlap=False)
    set_up(mb)
    with pytest.raises(SmgpuError, match=api + ": not available on an engine with boundary point smoothing"):
        mb.set_quality_constraint_limits(minDeterminant=0.01)
    _close(mb)
