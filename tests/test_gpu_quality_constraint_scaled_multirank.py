"""The quality constraint's scaling passes on a decomposed mesh (include/smgpu.h smgpu_set_quality_constraint_scaling_coupled,
smgpu_quality_constraint_pass_scale / _pass_sweep, csrc/kernels_quality_scale_coupled.hpp, DESIGN.md "Mesh quality" 10.20) through
the two smoothers of halo.py, against the CPU restatement (tests/quality_constraint_scaled_multi_reference.py, pinned against the
serial restatement by tests/test_quality_constraint_scaled_multi_reference.py) on its rows and settings: per-rank and combined records
exactly, minScale included -- its arithmetic is fixed by the contract --, the points of every iteration to rel_linf <= 1e-13 (the
bound of tests/test_gpu_quality_constraint_multirank.py against its helper), copies of shared points bit-identical.  Then the
arrangements by bits (overlap, SMGPU_QS_MAX_GRID), SMGPU_TILES=0, the equivalences of the contract, a clean run's launches, the
invariant through the decomposed report, the further limits, switching, refusals, and DistributedSmoother on one rank against the
serial engine's scaled run and on two processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_linf
from test_gpu_multirank import _copies_identical, _hex_case
from test_gpu_quality_constraint_multirank import NEVER, _close, _free_port, _smoother
from test_gpu_tangle import CASES
from test_quality_constraint_multi_reference import MULTI_CASES, limits_of, multi_mesh, multi_reference
from test_quality_constraint_scaled_multi_reference import ROWS, SETTINGS, scaled_multi_reference, scaling_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda s: "S%d_r%g_n%d_P%d" % s   # noqa: E731


def _records(recs, fields):
    return [{k: getattr(r, k) for k in fields} for r in recs]


def _scaled(ref, setting, monkeypatch, variant="com", overlap=False, env=None, limits=None, method="set_quality_constraint"):
    """a LocalMultiSmoother on the reference's sub-domains with the constraint and the scaling passes of `setting` on"""
    from smoothmesh_amd.halo import LocalMultiSmoother
    with monkeypatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        ms = LocalMultiSmoother(ref.subs, device=0, overlap=overlap)
        for st in ms.states:
            st.eng.set_foam_variant(variant)
        ms.set_params(ref.prm)
        getattr(ms, method)(passes=setting[3], **limits)
        if setting[0] is not None:
            ms.set_quality_constraint_scaling(**scaling_of(setting))      # (reads SMGPU_QS_MAX_GRID)
    return ms


def _assert_equals_reference(ms, want, n):
    from smoothmesh_amd.halo import combine_quality_constraint_records_scaled
    ref = want["ref"]
    fields = list(want["per_rank"][0][0])
    for k in range(n):
        got = ms.iterate(1, 0.0)
        assert got[0] == 1 and int(got[2][0]) == int(want["frz"][k])
        pts = ms.get_points()
        for r, p in enumerate(pts):
            err = rel_linf(p, want["pts"][k][r])
            print(k, r, err)
            assert err <= 1e-13, (k, r, err)
        _copies_identical(ref.subs, pts)
    raw = ms.quality_constraint_records_scaled(per_rank=True)
    assert [_records(r, fields) for r in raw] == want["per_rank"]
    assert _records(combine_quality_constraint_records_scaled(raw), list(want["recs"][0])) == want["recs"]
    assert ms.quality_constraint_records_scaled() == []                             # a read clears


# ---- 1. the smoother = the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
@pytest.mark.parametrize("name", ROWS)
def test_local_multi_smoother_equals_reference(oracle_lib, monkeypatch, name, setting):
    want = scaled_multi_reference(oracle_lib, name, setting)
    ms = _scaled(want["ref"], setting, monkeypatch, overlap=SETTINGS.index(setting) % 2 == 1, limits=limits_of(name))
    st = ms.quality_constraint_state_scaled()
    assert st.on and st.passes == setting[3] and (st.scalePasses, st.errorReduction, st.nSmoothScale) == setting[:3]
    assert st.nExemptCells == sum(want["ref"].nExemptCells) and st.nExemptFaces == sum(want["ref"].nExemptFaces)
    _assert_equals_reference(ms, want, MULTI_CASES[name][3])
    assert ms.quality_constraint_state_scaled().iteration == MULTI_CASES[name][3]
    _close(ms)


@pytest.mark.parametrize("variant,constraints", [("org", False), ("com", True), ("org", True)])
@pytest.mark.parametrize("name", ["tiles_611_both", "cavity_811"])
def test_foam_variants_and_the_references_constraints(oracle_lib, monkeypatch, name, variant, constraints):
    setting = (2, 0.75, 4, 2)
    want = scaled_multi_reference(oracle_lib, name, setting, variant, constraints)
    ms = _scaled(want["ref"], setting, monkeypatch, variant=variant, overlap=True, limits=limits_of(name))
    _assert_equals_reference(ms, want, MULTI_CASES[name][3])
    _close(ms)


def test_without_tiles(oracle_lib, monkeypatch):
    name, setting = "tiles_611_both", (1, 0.75, 2, 1)
    want = scaled_multi_reference(oracle_lib, name, setting)
    ms = _scaled(want["ref"], setting, monkeypatch, env={"SMGPU_TILES": "0"}, limits=limits_of(name))
    _assert_equals_reference(ms, want, MULTI_CASES[name][3])
    assert any(r["fullRevert"] for r in want["recs"]) and any(r["nPointsScaled"] > 0 for r in want["recs"])
    _close(ms)


# ---- 2. arrangements, by bits ---------------------------------------------------------------------------------------------
def _run(ms, n):
    out = ms.iterate(n, 0.0)
    assert out[0] == n
    return out[1], out[2], ms.get_points(), ms.quality_constraint_records_scaled(per_rank=True)


def _same_bits(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


def test_overlap_gives_the_same_bits(oracle_lib, monkeypatch):
    name, setting = "tiles_611", (1, 0.75, 2, 1)
    ref, n = multi_reference(oracle_lib, name)["ref"], MULTI_CASES[name][3]
    runs = []
    for overlap in (False, True):
        ms = _scaled(ref, setting, monkeypatch, overlap=overlap, limits=limits_of(name))
        runs.append(_run(ms, n))
        _close(ms)
    _same_bits(*runs)
    assert any(r.nPointsScaled > 0 for rr in runs[0][3] for r in rr)


@pytest.mark.parametrize("grid", [1, 3])
def test_several_trips_per_lane_give_the_same_bits(oracle_lib, monkeypatch, grid):
    """SMGPU_QS_MAX_GRID caps the sweep, the partial sums, the combine and the apply at 1 and 3 workgroups: on cavity_interface cut
    (2, 2, 1) lanes of the point kernels make a second trip under either cap"""
    name, setting = "cavity_221", (2, 0.75, 4, 2)
    ref, n = multi_reference(oracle_lib, name)["ref"], MULTI_CASES[name][3]
    assert max(s.mesh.nPoints for s in ref.subs) > 3 * 256
    a = _scaled(ref, setting, monkeypatch, limits=limits_of(name))
    b = _scaled(ref, setting, monkeypatch, env={"SMGPU_QS_MAX_GRID": str(grid)}, limits=limits_of(name))
    ra, rb = _run(a, n), _run(b, n)
    _same_bits(ra, rb)
    assert any(r.nPointsScaled > 0 for rr in ra[3] for r in rr)
    _close(a), _close(b)


# ---- 3. the equivalences ------------------------------------------------------------------------------------------------
def _counters(ms):
    return [{c["name"]: c["launches"] for c in st.eng.counters()} for st in ms.states]


def test_scale_passes_zero_is_the_run_as_it_is(oracle_lib, monkeypatch):
    """S = 0 after having been on, and a smoother that never made the call: points, records through the old getters, launches"""
    name = "tiles_611_both"
    want = multi_reference(oracle_lib, name)
    ref, lim, n = want["ref"], limits_of(name), MULTI_CASES[name][3]
    a = _scaled(ref, (2, 0.75, 4, 2), monkeypatch, limits=lim)
    a.set_quality_constraint_scaling(0)
    assert a.quality_constraint_state_scaled().scalePasses == 0 and a.scale_passes == 0
    b = _smoother(ref, "com", False, 2, {}, monkeypatch, lim)
    for ms in (a, b):
        for st in ms.states:
            st.eng.enable_timing(True)
            st.eng.reset_counters()
    ra, rb = a.iterate(n, 0.0), b.iterate(n, 0.0)
    assert ra[0] == rb[0] == n and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    for p, q in zip(a.get_points(), b.get_points()):
        assert np.array_equal(p, q)
    assert _counters(a) == _counters(b)
    qa, qb = a.quality_constraint_records(per_rank=True), b.quality_constraint_records(per_rank=True)
    assert qa == qb and [_records(r, list(want["per_rank"][0][0])) for r in qa] == want["per_rank"]
    assert any(r.fullRevert for r in qa[0])
    _close(a), _close(b)


def test_clean_run_adds_no_launch(oracle_lib):
    """constraint on, nothing bad: with the scaling passes on the launch counters and the bits are those with scaling off"""
    from smoothmesh_amd.halo import LocalMultiSmoother
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 1), (16, 12, 12), False)
    runs = []
    for S in (0, 2):
        ms = LocalMultiSmoother(subs, device=0, overlap=True)
        ms.set_params(prm)
        ms.set_quality_constraint(**NEVER)
        ms.set_quality_constraint_scaling(S, 0.75, 4)
        for st in ms.states:
            st.eng.enable_timing(True)
            st.eng.reset_counters()
        n, res, frz = ms.iterate(8, 0.0)
        assert n == 8
        recs = ms.quality_constraint_records_scaled()
        assert [(r.iteration, r.passes, r.fullRevert, r.nBadCells, r.nPointsReverted, r.nScalePasses, r.nPointsScaled) for r in recs] == \
            [(k, 0, 0, 0, 0, 0, 0) for k in range(1, 9)]
        assert all(r.minScale == (1.0 if S else 0.0) for r in recs)
        runs.append((res, frz, ms.get_points(), _counters(ms)))
        _close(ms)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    for p, q in zip(a[2], b[2]):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("name,S,P", [("tiles_611_both", 1, 1), ("cavity_811", 2, 0), ("dented_221", 1, 1)])
def test_factor_zero_without_sweeps_is_the_constraint_with_the_passes_added(oracle_lib, monkeypatch, name, S, P):
    ref, lim, n = multi_reference(oracle_lib, name)["ref"], limits_of(name), MULTI_CASES[name][3]
    a = _scaled(ref, (S, 0.0, 0, P), monkeypatch, limits=lim)
    b = _smoother(ref, "com", False, S + P, {}, monkeypatch, lim)
    for k in range(n):
        assert a.iterate(1, 0.0)[0] == 1 and b.iterate(1, 0.0)[0] == 1
        for p, q in zip(a.get_points(), b.get_points()):
            assert np.array_equal(p, q), k
    qa, qb = a.quality_constraint_records_scaled(per_rank=True), b.quality_constraint_records(per_rank=True)
    old = ("iteration", "passes", "fullRevert", "nBadCells", "nPointsReverted", "nTangledCells", "nNonOrthoFaces", "nSkewFaces")
    assert [_records(r, old) for r in qa] == [_records(r, old) for r in qb]
    assert all(r.nPointsScaled == 0 for rr in qa for r in rr) and any(r.nPointsReverted > 0 for rr in qa for r in rr)
    _close(a), _close(b)


# ---- 4. the invariant, through the decomposed report and its sets ------------------------------------------------------
@pytest.mark.parametrize("name,setting", [("tiles_611_both", (1, 0.75, 2, 1)), ("cavity_811", (2, 0.75, 4, 2))])
def test_invariant_through_the_report(oracle_lib, monkeypatch, name, setting):
    """after every iteration, by the report's sets under the constraint's limits: every face over a limit is an exempt one, on
    every rank, and no cell or face has become tangled (as tests/test_gpu_quality_constraint_multirank.py measures it)"""
    want = scaled_multi_reference(oracle_lib, name, setting)
    ref, lim, n = want["ref"], limits_of(name), MULTI_CASES[name][3]
    thr = dict(nonOrthThreshold=min(lim["maxNonOrtho"], 180.0))

    def over_a_limit(ms):
        si = ms.quality_sets(skewThreshold=lim["maxInternalSkewness"], **thr) if lim["maxInternalSkewness"] > 0.0 or lim["maxNonOrtho"] < 180.0 else None
        sb = ms.quality_sets(skewThreshold=lim["maxBoundarySkewness"], **thr) if lim["maxBoundarySkewness"] > 0.0 else None
        out = []
        for r, s in enumerate(ref.subs):
            F, Fi = s.mesh.nFaces, s.mesh.nInternalFaces
            inner = np.zeros(F, bool)
            for st, sz, _ in ref.couplings[r][1]:
                inner[st:st + sz] = True
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

    ms = _scaled(ref, setting, monkeypatch, overlap=True, limits=lim)
    q0 = ms.mesh_quality(skewThreshold=max(lim["maxInternalSkewness"], 1e-300), **thr)
    for k in range(n):
        assert ms.iterate(1, 0.0)[0] == 1
        q = ms.mesh_quality(skewThreshold=max(lim["maxInternalSkewness"], 1e-300), **thr)
        assert q.nNonPositiveVolume <= q0.nNonPositiveVolume and q.nWrongOrientedFaces <= q0.nWrongOrientedFaces
        assert over_a_limit(ms) == [0] * len(ref.subs), k
        for r, p in enumerate(ms.get_points()):                                      # the reports left the run as it was
            assert rel_linf(p, want["pts"][k][r]) <= 1e-13
    assert _records(ms.quality_constraint_records_scaled(), list(want["recs"][0])) == want["recs"]
    assert any(r["nPointsScaled"] > 0 for r in want["recs"])
    _close(ms)


# ---- 5. the further limits ----------------------------------------------------------------------------------------------------
def test_with_the_six_further_limits(oracle_lib, monkeypatch):
    from quality_constraint_scaled_multi_reference import QualityConstraintScaledMultiReference
    from test_quality_constraint_full_multi_reference import FULL_MULTI_CASES, _over_and_n, full_limits_of, full_multi_mesh
    name, setting = "all_221", (3, 0.5, 2, 1)
    over, n = _over_and_n(name)[0], 4
    lim = full_limits_of(name)
    want = QualityConstraintScaledMultiReference(oracle_lib, full_multi_mesh(name), FULL_MULTI_CASES[name][1], lim, setting[3], "com", False,
                                                 **scaling_of(setting), **over).run(n)
    ms = _scaled(want["ref"], setting, monkeypatch, limits={k: (None if v in (-1e30, -1.0) else v) for k, v in lim.items()},
                 method="set_quality_constraint_limits")
    _assert_equals_reference(ms, want, n)
    assert any(r["nPointsScaled"] > 0 for r in want["recs"]) and any(r["nLowVolRatioFaces"] + r["nLowWeightFaces"] > 0 for r in want["recs"])
    _close(ms)


def test_with_the_last_four_limits_the_ranks_add_up_to_the_serial_engine(monkeypatch):
    """no decomposed restatement holds the limits of 10.18: against the serial engine's scaled run on the undecomposed mesh, as
    tests/test_gpu_quality_constraint_all_multirank.py compares the unscaled one"""
    from quality_constraint_all_reference import FIELDS_ALL
    from quality_constraint_reference import OFF
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose, grid_partition
    from smoothmesh_amd.halo import LocalMultiSmoother
    from test_gpu_quality_trace import _engine
    from test_quality_constraint_all_reference import LIMITS
    case, grid, S, r, nS, P = "all", (8, 1, 1), 2, 0.75, 2, 1
    name = LIMITS[case][0]
    m, (_, over, n), lim = CASES[name][0](), CASES[name], {**OFF, **LIMITS[case][1]}
    subs = decompose(m, np.asarray(grid_partition(m, grid)), int(np.prod(grid)))
    ser = _engine(m, "com", False, **over)
    ser.set_quality_constraint(passes=P, **lim, scalePasses=S, errorReduction=r, nSmoothScale=nS)
    ms = LocalMultiSmoother(subs, device=0, overlap=False)
    ms.set_params(default_params(ser.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False, **over))
    ms.set_quality_constraint_limits_all(passes=P, **lim)
    ms.set_quality_constraint_scaling(S, r, nS)
    fields = FIELDS_ALL + ("nScalePasses", "nPointsScaled", "minScale")
    scaled = 0
    for k in range(n):
        assert ser.iterate(1, 0.0)[0] == 1 and ms.iterate(1, 0.0)[0] == 1
        (want,) = _records(ser.quality_constraint_records_scaled(), fields)
        (got,) = _records(ms.quality_constraint_records_scaled(), fields)
        assert got == want, (k, got, want)
        scaled += want["nPointsScaled"]
        out = np.empty((m.nPoints, 3))
        pts = ms.get_points()
        for s, p in zip(subs, pts):
            out[np.asarray(s.pointProcAddressing)] = np.asarray(p).reshape(-1, 3)
        assert np.max(np.abs(out - ser.get_points())) <= 1e-12, k
        _copies_identical(subs, pts)
    assert scaled > 0
    _close(ms)
    ser.close()


# ---- 6. switching, clearing -------------------------------------------------------------------------------------------------
def test_switching_on_off_on_between_calls_and_clearing(oracle_lib, monkeypatch):
    name, setting = "tiles_611_both", (1, 0.75, 2, 1)
    want = scaled_multi_reference(oracle_lib, name, setting)
    ref, lim = want["ref"], limits_of(name)
    plain = multi_reference(oracle_lib, name, "com", False, setting[3])
    ms = _scaled(ref, setting, monkeypatch, limits=lim)
    assert ms.iterate(2, 0.0)[0] == 2
    for r, p in enumerate(ms.get_points()):
        assert rel_linf(p, want["pts"][1][r]) <= 1e-13
    ms.set_quality_constraint_scaling(0)
    ms.set_quality_constraint_scaling(**scaling_of(setting))
    assert ms.iterate(len(want["pts"]) - 2, 0.0)[0] == len(want["pts"]) - 2
    for r, p in enumerate(ms.get_points()):
        assert rel_linf(p, want["pts"][-1][r]) <= 1e-13
    assert _records(ms.quality_constraint_records_scaled(), list(want["recs"][0])) == want["recs"]
    # re-enabling the constraint switches the scaling off: the unscaled run from the same points
    for st, sub in zip(ms.states, ref.subs):
        st.eng.set_points(sub.mesh.points)
    ms.set_quality_constraint(passes=setting[3], **lim)
    assert ms.quality_constraint_state_scaled().scalePasses == 0 and ms.scale_passes == 0
    assert ms.iterate(len(plain["pts"]), 0.0)[0] == len(plain["pts"])
    for r, p in enumerate(ms.get_points()):
        assert rel_linf(p, plain["pts"][-1][r]) <= 1e-13
    ms.set_quality_constraint_scaling(**scaling_of(setting))
    ms.clear_quality_constraint()
    st = ms.quality_constraint_state_scaled()
    assert not st.on and st.scalePasses == 0 and ms.scale_passes == 0
    with pytest.raises(RuntimeError, match="the quality constraint is off"):
        ms.set_quality_constraint_scaling(1)
    _close(ms)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(oracle_lib, monkeypatch):
    import torch
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.meshgen import hex_block
    from test_gpu_quality_trace import _engine
    ref, lim = multi_reference(oracle_lib, "dented_211")["ref"], limits_of("dented_211")
    ms = _smoother(ref, "com", False, None, {}, monkeypatch)
    s0 = ms.states[0]
    eng = s0.eng
    z = torch.zeros(max(s0.t.nSend, s0.t.nRecv, 1), dtype=torch.float64, device="cuda")
    api = "smgpu_set_quality_constraint_scaling_coupled"
    # the coupled quality constraint not on; the coupled tangle constraint
    with pytest.raises(SmgpuError, match=api + ": the coupled quality constraint is off"):
        eng.set_quality_constraint_scaling_coupled([0] * (s0.t.nSend + 1), [], [0] * s0.t.nSend, z.data_ptr(), z.data_ptr(), 1)
    with pytest.raises(RuntimeError, match="set_quality_constraint_scaling: the quality constraint is off"):
        ms.set_quality_constraint_scaling(1)
    ms.set_tangle_constraint()
    with pytest.raises(SmgpuError, match=api + ": the coupled tangle constraint is on"):
        eng.set_quality_constraint_scaling_coupled(None, None, None, 0, 0, 0)
    ms.clear_tangle_constraint()
    # the serial entry keeps its own refusal of a halo engine, in its wording
    with pytest.raises(SmgpuError, match="smgpu_set_quality_constraint_scaling: not available on an engine with a halo"):
        eng.set_quality_constraint_scaling(1)
    ms.set_quality_constraint(passes=1, **lim)
    # bad values, as 10.19; the overflow; a failure leaves scaling off on every rank
    for kw, msg in ((dict(scalePasses=-1), "scalePasses < 0"), (dict(scalePasses=1, errorReduction=1.0), "errorReduction is outside"),
                    (dict(scalePasses=1, errorReduction=float("nan")), "errorReduction is outside"), (dict(scalePasses=1, nSmoothScale=-1), "nSmoothScale < 0"),
                    (dict(scalePasses=2147483647), "scalePasses \\+ passes is above 2147483647")):
        with pytest.raises(SmgpuError, match=api + ": " + msg):
            ms.set_quality_constraint_scaling(**kw)
        assert ms.scale_passes == 0 and all(st.eng.quality_constraint_state_scaled().scalePasses == 0 for st in ms.states)
    # null or inconsistent tables and buffers
    off, pts, deg = s0.scaleTables
    with pytest.raises(SmgpuError, match=api + ": null exchange buffer"):
        eng.set_quality_constraint_scaling_coupled(off, pts, deg, 0, z.data_ptr(), 1)
    with pytest.raises(SmgpuError, match=api + ": rowPoints out of range"):
        eng.set_quality_constraint_scaling_coupled(off, np.full_like(pts, s0.sub.mesh.nPoints), deg, z.data_ptr(), z.data_ptr(), 1)
    with pytest.raises(SmgpuError, match=api + ": sharedDeg is below"):
        eng.set_quality_constraint_scaling_coupled(off, pts, np.zeros_like(deg), z.data_ptr(), z.data_ptr(), 1)
    assert eng.quality_constraint_state_scaled().scalePasses == 0
    # the pass protocol out of order
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_scale: the scaling passes are off"):
        eng.quality_constraint_pass_scale(1)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_sweep: the scaling passes are off"):
        eng.quality_constraint_pass_sweep()
    ms.set_quality_constraint_scaling(1, 0.75, 1)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_scale without smgpu_quality_constraint_pass_faces"):
        eng.quality_constraint_pass_scale(1)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_sweep without smgpu_quality_constraint_pass_scale"):
        eng.quality_constraint_pass_sweep()
    # between smgpu_iter_begin and smgpu_iter_end, then with passes due
    for st in ms.states:
        st.eng.iter_begin()
    with pytest.raises(SmgpuError, match=api + ": between smgpu_iter_begin and smgpu_iter_end"):
        eng.set_quality_constraint_scaling_coupled(None, None, None, 0, 0, 0)
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
    with pytest.raises(SmgpuError, match=api + ": the passes of an iteration are due"):
        eng.set_quality_constraint_scaling_coupled(None, None, None, 0, 0, 0)
    for st in ms.states:
        st.eng.quality_constraint_pass_begin()
    ms._move_cc()
    total = sum(st.eng.quality_constraint_pass_faces() for st in ms.states)
    assert total > 0
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_end: the scaling passes are on and cells are bad"):
        eng.quality_constraint_pass_end(total)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_scale: nBadGlobal <= 0"):
        eng.quality_constraint_pass_scale(0)
    ms._move_marks()
    for st in ms.states:
        st.eng.quality_constraint_pass_scale(total)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_scale: called twice in one pass"):
        eng.quality_constraint_pass_scale(total)
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_end: 1 sweeps of the pass are due"):
        eng.quality_constraint_pass_end(total)
    ms._move_scales()
    for st in ms.states:
        st.eng.quality_constraint_pass_sweep()
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_sweep: no sweep of the pass is due"):
        eng.quality_constraint_pass_sweep()
    with pytest.raises(SmgpuError, match="smgpu_quality_constraint_pass_end: nBadGlobal differs"):
        eng.quality_constraint_pass_end(total + 1)
    assert [st.eng.quality_constraint_pass_end(total) for st in ms.states] == [False] * len(ms.states)
    _close(ms)
    # an engine without a halo
    e = _engine(hex_block(6, 5, 4, jitter=0.3))
    e.set_quality_constraint()
    with pytest.raises(SmgpuError, match=api + ": the engine has no halo"):
        e.set_quality_constraint_scaling_coupled([0], [], [], z.data_ptr(), z.data_ptr(), 1)
    e.close()
    # boundary point smoothing
    from test_gpu_boundary import _decomposed_boundary_case
    from smoothmesh_amd.halo import LocalMultiSmoother
    mo, orcs, subs, prm, set_up = _decomposed_boundary_case(oracle_lib, (2, 1, 1), False, False)
    mb = LocalMultiSmoother(subs, device=0, overlap=False)
    set_up(mb)
    with pytest.raises(SmgpuError, match=api + ": not available on an engine with boundary point smoothing"):
        mb.states[0].eng.set_quality_constraint_scaling_coupled(None, None, None, 0, 0, 0)
    _close(mb)


# ---- 8. DistributedSmoother -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_distributed_smoother_on_one_rank_equals_the_serial_engines_scaled_run(overlap):
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import decompose
    from smoothmesh_amd.halo import DistributedSmoother
    from test_gpu_quality_trace import _engine
    m, over, lim = multi_mesh("tiles_611_both"), CASES["dented_tiles"][1], limits_of("tiles_611_both")
    sc = dict(scalePasses=1, errorReduction=0.75, nSmoothScale=2)
    ser = _engine(m, "com", False, **over)
    ser.set_quality_constraint(passes=1, **lim, **sc)
    ser_run = ser.iterate(6, 0.0)
    assert ser_run[0] == 6
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        sub = decompose(m, np.zeros(m.nCells, np.int32), 1)[0]
        ds = DistributedSmoother(sub, device=0, overlap=overlap)
        ds.set_params(default_params(ser.mesh_stats()[0], edgeAngleConstraint=False, faceAngleConstraint=False, **over))
        ds.set_quality_constraint(passes=1, **lim)
        ds.set_quality_constraint_scaling(**sc)
        sd, ss = ds.quality_constraint_state_scaled(), ser.quality_constraint_state_scaled()
        ss.iteration = 0                                       # (the serial engine has run already)
        assert sd == ss and sd.scalePasses == 1
        n_d, res_d, frz_d = ds.iterate(6, 0.0)
        assert n_d == 6 and np.array_equal(res_d, ser_run[1]) and np.array_equal(frz_d, ser_run[2])
        recs = ds.quality_constraint_records_scaled()
        assert recs == ser.quality_constraint_records_scaled()
        assert any(r.fullRevert for r in recs) and any(r.nPointsScaled > 0 for r in recs) and any(r.nPointsReverted > 0 and not r.fullRevert for r in recs)
        back = np.empty_like(ser.get_points())
        back[sub.pointProcAddressing] = ds.get_points()
        assert np.array_equal(back, ser.get_points())
        ds.close()
    finally:
        dist.destroy_process_group()
    ser.close()


def test_distributed_smoother_two_processes(tmp_path):
    """One process per rank with the real engines, two ranks sharing one GPU through the gloo debug transport, each under a time
    limit of its own: exchange S staged like exchange T (scripts/check_dist_quality_constraint_scaled.py)"""
    env = dict(os.environ, SMOOTHMESH_SHARE_GPU="1", SMOOTHMESH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    env.pop("SMOOTHMESH_EXCHANGE", None)
    script = os.path.join(ROOT, "scripts", "check_dist_quality_constraint_scaled.py")
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
