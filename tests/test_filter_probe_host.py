"""The probe helper of the filter boundary tests (tests/filter_probe.py) without a GPU: the inverse of the host's threshold
preparation lands where it is asked to, and the fixtures hold what the GPU tests need -- checked with the oracle alone."""
import math

import numpy as np
import pytest

import filter_probe as fp


def test_model_at_the_default_parameters():
    """known answers of the model: the f32 values makePrm and runConstraints produce for minAngle 35, maxAngle 160"""
    th = fp.host_thresholds(35.0, 160.0)
    assert th["smallAngle"] == math.pi * 35.0 / 180.0 and th["largeAngle"] == math.pi * 160.0 / 180.0
    assert th["thrEA"] == float(np.float32(math.cos(th["smallAngle"])) - np.float32(1.0e-3))
    assert abs(th["thrEA"] - (math.cos(th["smallAngle"]) - 1e-3)) <= 1.2e-7
    assert abs(th["faCosLo"] - (math.cos(th["smallAngle"]) - 2.02e-3)) <= 6e-8 + 1e-10     # (kFaMargin is the f32 nearest to 2e-3)
    assert abs(th["faCosHi"] - (math.cos(th["largeAngle"]) + 2.02e-3)) <= 6e-8 + 1e-10
    assert th["faCosHi"] < th["faCosLo"]


def test_out_of_range_parameters_leave_the_face_angle_filter_undecided():
    assert fp.host_thresholds(180.0, 160.0)["faCosLo"] == -2.0 and fp.host_thresholds(35.0, 0.0)["faCosHi"] == 2.0
    assert fp.host_thresholds(-5.0, 200.0)["faCosLo"] == float(np.float32(1.0 - fp.FA_M))
    assert fp.host_thresholds(-5.0, 200.0)["faCosHi"] == float(np.float32(-1.0 + fp.FA_M))


def test_inverse_achieves_the_wanted_threshold():
    """over the range the probes use (element cosines in (-0.99, 0.99), offsets up to 2e-3): the achieved threshold is within
    2e-7 of the wanted one -- two f32 roundings of values of magnitude at most 1 allow 6e-8 each"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for x in np.concatenate([np.linspace(-0.99, 0.99, 397), rng.uniform(-0.99, 0.99, 400)]):
        for d in fp.LADDER:
            w = x + d
            worst = max(worst, abs(fp.host_thresholds(fp.degrees_for_thrEA(w), 160.0)["thrEA"] - w),
                        abs(fp.host_thresholds(fp.degrees_for_faCosLo(w), 179.0)["faCosLo"] - w),
                        abs(fp.host_thresholds(1.0, fp.degrees_for_faCosHi(x - d))["faCosHi"] - (x - d)))
    assert worst <= 2e-7, worst


def test_degrees_at_an_angle():
    rng = np.random.default_rng(6)
    for x in rng.uniform(0.05, 1.9 * math.pi, 500):
        lo, mid, hi = fp.degrees_at_angle(x)
        assert lo < mid < hi and np.nextafter(lo, np.inf) == mid and np.nextafter(mid, np.inf) == hi
        err = [abs(math.pi * d / 180.0 - x) for d in (lo, mid, hi)]
        assert err[1] <= err[0] and err[1] <= err[2] and err[1] <= 2.0 * np.spacing(x)


@pytest.fixture(scope="module")
def device_acos(oracle_lib):
    prev = oracle_lib.set_acos_variant("device")
    yield oracle_lib
    oracle_lib.set_acos_variant(prev)


@pytest.mark.parametrize("case", fp.CASES)
def test_fixtures_hold_enough_probes(device_acos, case):
    """the pre-checks of the GPU tests: at least 24 candidate elements per probe family on every mesh"""
    ref = fp.Reference(fp.case_mesh(case), device_acos)
    assert len(ref.ea_candidates()) >= fp.N_PROBES
    assert len(ref.fa_candidates("min")) >= fp.N_PROBES and len(ref.fa_candidates("max")) >= fp.N_PROBES
    for e, p in ref.fa_candidates("min") + ref.fa_candidates("max"):
        assert p in ref.edges[e]
    if case == "cavity":
        below, above, pb, pa = ref.near_pi_edges()
        assert len(below) >= 16 and len(above) >= 16, (len(below), len(above))
        assert len(pb) == 8 and len(pa) == 8
    if case == "block":
        # the decisions move with the thresholds, and come back: the cache of Reference.decisions is keyed by them
        f0, a0 = ref.decisions(35.0, 160.0)
        f1, a1 = ref.decisions(80.0, 100.0)
        assert f1.sum() > f0.sum() and a1.sum() > a0.sum()
        ref._dec.clear()
        f2, a2 = ref.decisions(35.0, 160.0)
        assert np.array_equal(f0, f2) and np.array_equal(a0, a2)
