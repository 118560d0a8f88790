"""The CPU restatement of the quality constraint's scaling passes on a decomposed mesh
(tests/quality_constraint_scaled_multi_reference.py; DESIGN.md "Mesh quality", 10.20) against the serial restatement on the
undecomposed mesh (tests/quality_constraint_scaled_reference.py, 10.19): the combined records are equal, the gathered points lie
within 1e-12 -- the bound of tests/test_quality_constraint_multi_reference.py: the rows' orders and the fold over the ranks differ,
so the decomposed run is the serial run to rounding, not to the bit -- and the copies of shared points are identical.  Equality of
the records is a condition on the inputs, as the margins are.  Rows: MULTI_CASES of tests/test_quality_constraint_multi_reference.py.
Also the two equivalences of the contract by ==, and the ctypes mirror of smgpu_quality_scale_coupling against the header."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from quality_constraint_multi_reference import FACE_MARGIN, MARGIN
from quality_constraint_scaled_multi_reference import QualityConstraintScaledMultiReference
from quality_constraint_scaled_reference import reference_run
from test_gpu_tangle import CASES
from test_quality_constraint_multi_reference import MULTI_CASES, limits_of, multi_mesh, multi_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["dented_211", "dented_221", "tiles_611", "tiles_611_both", "tiles_431", "cavity_221", "cavity_811"]
# (S, r, n, P)
SETTINGS = [(2, 0.5, 1, 2), (2, 0.75, 4, 2), (3, 0.5, 2, 1), (1, 0.75, 2, 1), (1, 0.75, 0, 0)]


def scaling_of(setting):
    S, r, n, _ = setting
    return dict(scalePasses=S, errorReduction=r, nSmoothScale=n)


@functools.lru_cache(maxsize=None)
def scaled_multi_reference(oracle_lib, name, setting, variant="com", constraints=False):
    """computed once per configuration and shared (tests/test_gpu_quality_constraint_scaled_multirank.py too)"""
    case, grid, _, n, _ = MULTI_CASES[name]
    r = QualityConstraintScaledMultiReference(oracle_lib, multi_mesh(name), grid, limits_of(name), setting[3], variant, constraints,
                                              **scaling_of(setting), **CASES[case][1]).run(n)
    ref = r["ref"]
    assert ref.minMargin > MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    return r


@functools.lru_cache(maxsize=None)
def _serial(oracle_lib, name, setting, constraints=False):
    case, _, _, n, _ = MULTI_CASES[name]
    return reference_run(oracle_lib, multi_mesh(name), n, limits=limits_of(name), passes=setting[3], constraints=constraints, scaling=scaling_of(setting),
                         **CASES[case][1])


def _assert_is_serial(ser, mul):
    ref = mul["ref"]
    for a, b in zip(mul["recs"], ser["recs"]):
        assert a == {k: b[k] for k in a}, (a, b)
        assert all(v == 0 for k, v in b.items() if k not in a), b        # (the limits of 10.18 are off)
    assert len(mul["recs"]) == len(ser["recs"])
    worst = 0.0
    for ps, pm in zip(ser["pts"], mul["pts"]):
        g = ref.gather(pm)
        worst = max(worst, float(np.max(np.abs(g - ps))))
        for r, p in enumerate(pm):      # copies of a shared point are identical
            assert np.array_equal(g[ref.ppa[r]], p)
    assert worst <= 1e-12, worst
    return worst


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "S%d_r%g_n%d_P%d" % s)
@pytest.mark.parametrize("name", ROWS)
def test_decomposed_scaled_run_is_the_serial_run(oracle_lib, name, setting):
    ser, mul = _serial(oracle_lib, name, setting), scaled_multi_reference(oracle_lib, name, setting)
    worst = _assert_is_serial(ser, mul)
    print(f"{name} {setting}: largest point difference {worst:.3e}, uncounted row entries {mul['ref'].uncounted}")
    # a condition on the inputs: every row has row entries that are not counted (edges between shared points held by several ranks)
    assert mul["ref"].uncounted > 0
    assert any(r["nBadCells"] > 0 for r in mul["recs"]), "no cell is ever bad: the row tests nothing"


def test_some_run_scales_reverts_and_ends_in_a_full_revert(oracle_lib):
    """conditions on the inputs, over the rows and settings: one run does all three"""
    recs = scaled_multi_reference(oracle_lib, "tiles_611_both", (1, 0.75, 2, 1))["recs"]
    assert any(r["nPointsScaled"] > 0 for r in recs) and any(r["nPointsReverted"] > 0 and not r["fullRevert"] for r in recs)
    assert any(r["fullRevert"] for r in recs)
    assert any(r["nScalePasses"] > 0 for r in recs)
    # every count of passes stays within its setting, and somewhere an iteration is accepted with every scale above 0
    every = [(setting, r) for name in ROWS for setting in SETTINGS for r in scaled_multi_reference(oracle_lib, name, setting)["recs"]]
    assert all(r["passes"] <= setting[0] + setting[3] and r["nScalePasses"] <= setting[0] for setting, r in every)
    assert any(0.0 < r["minScale"] < 1.0 for _, r in every)


@pytest.mark.parametrize("name", ["dented_221", "tiles_611_both"])
def test_scale_passes_zero_is_the_constraint_without_them(oracle_lib, name):
    case, grid, _, n, _ = MULTI_CASES[name]
    a = QualityConstraintScaledMultiReference(oracle_lib, multi_mesh(name), grid, limits_of(name), 2, "com", False, scalePasses=0, **CASES[case][1]).run(n)
    b = multi_reference(oracle_lib, name)
    assert [[{k: r[k] for k in q} for r, q in zip(ra, rb)] for ra, rb in zip(a["per_rank"], b["per_rank"])] == b["per_rank"]
    assert all(r["nScalePasses"] == 0 and r["nPointsScaled"] == 0 and r["minScale"] == 0.0 for rr in a["per_rank"] for r in rr)
    for pa, pb in zip(a["pts"], b["pts"]):
        assert all(np.array_equal(p, q) for p, q in zip(pa, pb))


@pytest.mark.parametrize("name", ["dented_221", "tiles_611_both", "cavity_811"])
def test_no_reduction_and_no_sweeps_is_the_constraint_with_more_passes(oracle_lib, name):
    """S > 0, r = 0, n = 0: the accepted points of the coupled constraint with passes = S + P"""
    case, grid, _, n, _ = MULTI_CASES[name]
    a = QualityConstraintScaledMultiReference(oracle_lib, multi_mesh(name), grid, limits_of(name), 1, "com", False, scalePasses=1, errorReduction=0.0,
                                              nSmoothScale=0, **CASES[case][1]).run(n)
    b = multi_reference(oracle_lib, name, "com", False, 2)
    for pa, pb in zip(a["pts"], b["pts"]):
        assert all(np.array_equal(p, q) for p, q in zip(pa, pb))
    shared = ("iteration", "passes", "fullRevert", "nBadCells", "nPointsReverted", "nTangledCells", "nNonOrthoFaces", "nSkewFaces")
    assert [[{k: r[k] for k in shared} for r in rr] for rr in a["per_rank"]] == [[{k: r[k] for k in shared} for r in rr] for rr in b["per_rank"]]
    assert all(r["nPointsScaled"] == 0 and r["minScale"] in (0.0, 1.0) for rr in a["per_rank"] for r in rr)
    assert any(r["nPointsReverted"] > 0 for r in a["recs"])


def test_the_reference_constraints_on(oracle_lib):
    setting = (2, 0.75, 4, 2)
    _assert_is_serial(_serial(oracle_lib, "tiles_611", setting, True), scaled_multi_reference(oracle_lib, "tiles_611", setting, "com", True))


def test_ctypes_mirror_of_the_descriptor_has_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    cname, mirror = "smgpu_quality_scale_coupling", _ffi.QualityScaleCoupling
    body = f'    printf("size %zu\\n", sizeof({cname}));\n' + "".join(f'    printf("{n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    got = {a: int(v) for a, v in (line.split() for line in out if line)}
    assert got == {"size": C.sizeof(mirror), **{n: getattr(mirror, n).offset for n, _ in mirror._fields_}}
    assert got == dict(size=40, rowOffsets=0, rowPoints=8, sharedDeg=16, sendS=24, recvS=32)
    for sym in ("smgpu_set_quality_constraint_scaling_coupled", "smgpu_quality_constraint_pass_scale", "smgpu_quality_constraint_pass_sweep"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them
