"""The f32 angle filters (smoothmesh_amd/csrc/kernels_filter.hpp) held to their error budget, element by element.

The filters' verdicts are read back (debug fields "eaMaybe" / "faMaybe") on one iteration state while the thresholds are walked
across chosen elements: a ladder of offsets around the element's exact value (the oracle's, with the engine's acos) and the true
threshold put on the element itself.  On every run and for every element of the mesh:
  1. soundness, exact: what a filter calls GOOD is on the good side of the TRUE threshold; an edge without an angle is never GOOD;
  2. budget: the margin a GOOD verdict has consumed stays within the bound the header derives for that form (filter_probe.BUDGET);
  3. parity: frozen points and the active set are the oracle's;
  4. with the true threshold on an element, the filter leaves that element to the exact kernel.
Each case prints one line "FILTER_BOUNDARY {...}" with its measurements (DESIGN.md section 4.2 holds a table of them)."""
import json
import math
import re

import numpy as np
import pytest

import filter_probe as fp

pytestmark = pytest.mark.gpu

_TILES = re.compile(r"\[smgpu\] tiles: geom T=(\d+) .* smooth T=(\d+) ")
_EDGE_TILES = "[smgpu] edge tiles: n="
FORMS = ("k_ea_filter_tile", "k_edge_angle_filter", "k_fa_filter_tile", "k_fa_edges_filter")
_REF = {}


@pytest.fixture(scope="module")
def device_acos(oracle_lib):
    prev = oracle_lib.set_acos_variant("device")      # both sides see the same bits: a tie is a tie on both
    yield oracle_lib
    oracle_lib.set_acos_variant(prev)


def _reference(case, oracle_lib):
    if case not in _REF:
        _REF[case] = fp.Reference(fp.case_mesh(case), oracle_lib)
    return _REF[case]


def _engine(ref, case, form, monkeypatch, capfd):
    """one engine on which the form under test is the one that runs -- confirmed from the set-up lines, not assumed"""
    from smoothmesh_amd import SmoothEngine
    from test_gpu_tile_shapes import _needs
    monkeypatch.setenv("SMGPU_DEBUG_FILTERED", "1")
    monkeypatch.setenv("SMGPU_VERBOSE", "1")
    if form == "k_edge_angle_filter":
        monkeypatch.setenv("SMGPU_SMOOTH_T", "128")
    if form == "k_fa_edges_filter":
        monkeypatch.setenv("SMGPU_EDGE_CAPF", str(_needs(ref.mesh)["ef"] - 1))
    if case == "fan":
        # not under test here, and every form gives the oracle's sets: the one-wave replay of the face-angle walk takes 20 ms per
        # pass on this mesh (valence 22 on the axis), the fixed-point form 0.3 ms -- 480 passes per test
        monkeypatch.setenv("SMGPU_WALK", "fix")
    capfd.readouterr()
    e = SmoothEngine(ref.mesh)
    err = capfd.readouterr().err
    m = _TILES.search(err)
    assert m, err
    if form.startswith("k_e"):
        assert int(m.group(2)) == (256 if form == "k_ea_filter_tile" else 128), err
    else:
        assert (_EDGE_TILES in err) == (form == "k_fa_filter_tile"), err
    return e


class _Runner:
    def __init__(self, e, ref, form, eager):
        """eager: the budget is asserted on every pass (else by the caller, once it knows that the filter decides anything here)"""
        self.e, self.ref, self.ea, self.eager, self.budget = e, ref, form.startswith("k_e"), eager, fp.BUDGET[form]
        self.runs = 0
        self.used = {"ea": 0.0} if self.ea else {"min": 0.0, "max": 0.0}

    def __call__(self, minAngle, maxAngle):
        """one pass at these thresholds: assertions 1, 2 (where it holds unconditionally) and 3 on the whole mesh, in that order --
        a filter that is wrong is named before the wrong decision it causes; returns the marks and the thresholds"""
        e, ref = self.e, self.ref
        e.set_params(ref.params(minAngle, maxAngle))
        e.debug_propose()
        self.runs += 1
        th = fp.host_thresholds(minAngle, maxAngle)
        at = "minAngle=%r maxAngle=%r" % (minAngle, maxAngle)
        with np.errstate(invalid="ignore"):
            if self.ea:
                maybe = e.debug_field("eaMaybe").astype(bool)
                good = ~maybe & ~ref.frozenLen
                bad = good & ~(ref.eaMinN >= th["smallAngle"])
                assert not bad.any(), "GOOD points below the true threshold: %s, %s" % (np.flatnonzero(bad)[:8], at)
                self.used["ea"] = max(self.used["ea"], float(np.nanmax(ref.cosEa[good] - th["thrEA"], initial=0.0)))
            else:
                maybe = e.debug_field("faMaybe").astype(bool)
                good = ~maybe[ref.edges[:, 0]] | ~maybe[ref.edges[:, 1]]
                bad = good & (ref.noAngle | ~(ref.edgeMin > th["smallAngle"]) | ~(ref.edgeMax < th["largeAngle"]))
                assert not bad.any(), "GOOD edges outside the true thresholds or without an angle: %s, %s" % (np.flatnonzero(bad)[:8], at)
                self.used["min"] = max(self.used["min"], float(np.nanmax(ref.cosMin[good] - th["faCosLo"], initial=0.0)))
                self.used["max"] = max(self.used["max"], float(np.nanmax(th["faCosHi"] - ref.cosMax[good], initial=0.0)))
        if self.eager:
            self.check_budget(at)
        frozen, active = ref.decisions(minAngle, maxAngle)
        assert np.array_equal(e.debug_field("isFrozenPoint").astype(bool), frozen), "frozen set differs from the oracle's, " + at
        assert np.array_equal(e.debug_field("faActive").astype(bool), active), "active set differs from the oracle's, " + at
        return maybe, th

    def check_budget(self, at=""):
        for side, used in self.used.items():      # (both sides of a face-angle form, whichever is probed: every run sees the whole mesh)
            assert used <= self.budget, "%s: a GOOD verdict consumed %.3e of the margin, the header's bound is %.3e %s" % (side, used, self.budget, at)


def _family(run, ref, side):
    """the probes of one family: side "ea" (points, minAngle), "min" / "max" (edges, minAngle / maxAngle).
    -> measurements; asserts 4 on the probed elements (1 and 3 are asserted by every run)"""
    if side == "ea":
        cands, x, exact = ref.ea_candidates(), ref.cosEa, ref.eaMinN
        angles = lambda w: (fp.degrees_for_thrEA(w), 160.0)
        offset = lambda th, el: th["thrEA"] - x[el]
    elif side == "min":
        cands, x, exact = ref.fa_candidates("min"), ref.cosMin, ref.edgeMin
        angles = lambda w: (fp.degrees_for_faCosLo(w), 179.0)
        offset = lambda th, el: th["faCosLo"] - x[el]
    else:
        cands, x, exact = ref.fa_candidates("max"), ref.cosMax, ref.edgeMax
        angles = lambda w: (1.0, fp.degrees_for_faCosHi(w))
        offset = lambda th, el: x[el] - th["faCosHi"]
    sgn = -1.0 if side == "max" else 1.0
    on = lambda deg: (deg, 160.0 if side == "ea" else 179.0) if side != "max" else (1.0, deg)
    eligible = []
    ref.prefetch([angles(x[el] + sgn * fp.LADDER[0]) for el, p in cands])
    for el, p in cands:                       # the ladder's first rung on every candidate: the selection
        maybe, th = run(*angles(x[el] + sgn * fp.LADDER[0]))
        if not maybe[p]:
            eligible.append((el, p))
    probes = fp._spread(eligible, fp.N_PROBES)
    ref.prefetch([angles(x[el] + sgn * d) for el, p in probes for d in fp.LADDER[1:]]
                 + [on(deg) for el, p in probes for deg in fp.degrees_at_angle(exact[el])])
    goodFrom = []                             # per probe: the smallest positive offset (as achieved) at which it is GOOD
    eaten = 0.0                               # the largest negative offset at which a probe was still GOOD
    for el, p in probes:
        first = fp.LADDER[0]
        for d in fp.LADDER[1:]:
            maybe, th = run(*angles(x[el] + sgn * d))
            got = offset(th, el)
            if not maybe[p]:
                if got > 0:
                    first = min(first, got)
                else:
                    eaten = max(eaten, -got)
        goodFrom.append(first)
        for deg in fp.degrees_at_angle(exact[el]):
            maybe, th = run(*on(deg))
            marked = maybe[p] if side == "ea" else maybe[ref.edges[el]].all()
            assert marked, "%s element %d decided by the filter with the true threshold on it (%r degrees)" % (side, el, deg)
    return dict(candidates=len(cands), eligible=len(eligible), probed=len(probes), good_from_smallest=min(goodFrom, default=None),
                good_from_largest=max(goodFrom, default=None), good_at_negative_offset=eaten)


# (form, probe family): the face-angle forms are probed from the small and from the large threshold in tests of their own
FAMILIES = [(FORMS[0], "ea"), (FORMS[1], "ea"), (FORMS[2], "min"), (FORMS[2], "max"), (FORMS[3], "min"), (FORMS[3], "max")]


@pytest.mark.parametrize("form,side", FAMILIES, ids=["%s-%s" % fs for fs in FAMILIES])
@pytest.mark.parametrize("case", fp.CASES)
def test_filter_verdicts_on_the_threshold(device_acos, monkeypatch, capfd, case, form, side):
    """one form of a filter on one mesh, probed from one threshold (module docstring); filter_probe.CASES: the jittered block, the
    same block stretched, shifted and scaled, the castellated cavity mesh (polygonal faces, ring sums around pi) and the 20-spoke
    fan (rows longer than the tile filters' preloaded chunks).  Stretched and scaled, the filters may decide little or nothing:
    the share of candidates they decide at +2e-3 is printed, and the budget and the floor of 24 probes hold where it is not zero
    (stretched) or are left out (scaled); soundness and parity hold everywhere."""
    ref = _reference(case, device_acos)
    e = _engine(ref, case, form, monkeypatch, capfd)
    run = _Runner(e, ref, form, fp.asserts_budget(case))
    report = dict(case=case, form=form, families={})
    try:
        report["families"][side] = _family(run, ref, side)
        if side == "max":
            for angles in ((35.0, 180.0), (35.0, 200.0)):
                run(*angles)
            if case == "cavity":
                # largest angles just below pi and above it: no ladder (its rungs would ask for cos(large) < -1), the true threshold on them
                below, above, pb, pa = ref.near_pi_edges()
                assert len(below) >= 16 and len(above) >= 16
                for el in list(pb) + list(pa):
                    for deg in fp.degrees_at_angle(ref.edgeMax[el]):
                        maybe, th = run(1.0, deg)
                        assert maybe[ref.edges[el]].all(), "edge %d (largest angle %r) decided with the true threshold on it" % (el, ref.edgeMax[el])
                report["near_pi_probes"] = len(pb) + len(pa)
    finally:
        report["runs"], report["consumed"], report["budget"] = run.runs, run.used, fp.BUDGET[form]
        with capfd.disabled():
            print("\nFILTER_BOUNDARY " + json.dumps(report))
        e.close()
    fams = report["families"].values()
    decides = all(f["eligible"] > 0 for f in fams)
    if fp.asserts_budget(case) or (case.startswith("stretch") and decides):
        for side, f in report["families"].items():
            assert f["eligible"] >= fp.N_PROBES, "%s: only %d of %d candidates are GOOD at +2e-3" % (side, f["eligible"], f["candidates"])
        run.check_budget()


def test_verdict_fields_fail_when_the_filter_did_not_run(monkeypatch):
    """"eaMaybe" / "faMaybe" are the latest pass's verdicts or an error, never the bytes of an earlier pass"""
    from smoothmesh_amd import SmgpuError, SmoothEngine, default_params
    mesh = fp.case_mesh("block")
    e = SmoothEngine(mesh)
    e.set_params(default_params(e.mesh_stats()[0]))
    for name in ("eaMaybe", "faMaybe"):
        with pytest.raises(SmgpuError, match="did not run"):
            e.debug_field(name)
    monkeypatch.setenv("SMGPU_DEBUG_FILTERED", "1")
    e.debug_propose()
    n = mesh.nPoints
    ea, fa = e.debug_field("eaMaybe"), e.debug_field("faMaybe")
    assert ea.shape == fa.shape == (n,) and set(np.unique(ea)) <= {0.0, 1.0} and set(np.unique(fa)) <= {0.0, 1.0}
    assert 0 < (ea == 0).sum() and 0 < (fa == 0).sum()          # a decent block at the default thresholds: the filters decide
    monkeypatch.setenv("SMGPU_DEBUG_FILTERED", "0")
    e.debug_propose()                                             # exact kernels on everything: the marks above are now stale
    for name in ("eaMaybe", "faMaybe"):
        with pytest.raises(SmgpuError, match="did not run"):
            e.debug_field(name)
    e.set_params(default_params(e.mesh_stats()[0], edgeAngleConstraint=False))
    monkeypatch.setenv("SMGPU_DEBUG_FILTERED", "1")
    e.debug_propose()
    with pytest.raises(SmgpuError, match="did not run"):
        e.debug_field("eaMaybe")
    assert e.debug_field("faMaybe").shape == (n,)
    e.close()
