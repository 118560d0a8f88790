"""The CPU restatement of the quality constraint's six further limits on a decomposed mesh
(tests/quality_constraint_full_multi_reference.py; DESIGN.md "Mesh quality", 10.17) against the serial restatement
(tests/quality_constraint_full_reference.py) on the undecomposed mesh: combined full records exactly, gathered points within 1e-12
(the bound of tests/test_quality_constraint_multi_reference.py), the invariant after every iteration.  The rows were chosen on the
CPU with the helper, under the conditions asserted here: each of tet quality, twist, weight and volume ratio has a row with
non-exempt bad verdicts on processor faces, whose two cells lie on two ranks -- a verdict without recvCc / recvVc is wrong there --
and the determinant has rows in which cells on the cut have another verdict or exemption under the serial face rule.  Also the
ctypes mirror of smgpu_quality_constraint_halo_desc_full against the header."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import tangle_reference
from quality_constraint_full_multi_reference import FACE_LIMITS, MORE, MORE_MARGIN, SUMMED_FULL, QualityConstraintFullMultiReference
from quality_constraint_full_reference import FIELDS_FULL, reference_run
from quality_constraint_multi_reference import FACE_MARGIN, FIELDS, OFF, QualityConstraintMultiReference
from test_gpu_tangle import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, maxBoundarySkewness=0.5, minTetQuality=1e-4, minTwist=0.05, minTriangleTwist=0.05,
           minFaceWeight=0.32, minVolRatio=0.11, minDeterminant=0.124)
# name -> (mesh, cut, the limits (a criterion not named is off), the face criteria that must give verdicts on processor faces).
# 10.16's limits on cavity_interface; cut (8,1,1) runs through the polyhedral interface, cut (2,2,1) does not.  minFaceWeight is
# 0.30 on (8,1,1): at 0.32 that cut leaves four points whose step is at the rounding level counted as moved on one mesh and not on
# the other, so nPointsReverted of the two restatements differs by 4 -- a tie in a count, which the inputs have to stay away from.
FULL_MULTI_CASES = {
    "tet_811": ("cavity_interface", (8, 1, 1), dict(minTetQuality=1e-4), ("minTetQuality",)),
    "twist_811": ("cavity_interface", (8, 1, 1), dict(minTwist=0.05), ("minTwist",)),
    "triangle_twist_811": ("cavity_interface", (8, 1, 1), dict(minTriangleTwist=0.05), ("minTriangleTwist",)),
    "weight_811": ("cavity_interface", (8, 1, 1), dict(minFaceWeight=0.30), ("minFaceWeight",)),
    "ratio_811": ("cavity_interface", (8, 1, 1), dict(minVolRatio=0.11), ("minVolRatio",)),
    "determinant_811": ("cavity_interface", (8, 1, 1), dict(minDeterminant=0.035), ()),
    "weight_221": ("cavity_interface", (2, 2, 1), dict(minFaceWeight=0.32), ()),
    "ratio_221": ("cavity_interface", (2, 2, 1), dict(minVolRatio=0.11), ()),
    "tiles_weight_611": ("dented_tiles", (6, 1, 1), dict(minFaceWeight=0.425), ()),
    "all_221": ("cavity_interface", (2, 2, 1), ALL, ()),
    "all_811": ("cavity_interface", (8, 1, 1), dict(ALL, minFaceWeight=0.30), ("minTetQuality", "minTwist", "minTriangleTwist", "minFaceWeight", "minVolRatio")),
    "block_211": ("block", (2, 1, 1), dict(minDeterminant=0.9), ()),
    "jittered_block_211": ("jittered_block", (2, 1, 1), dict(minDeterminant=0.9), ()),
}
BLOCKS = {"block": 0.0, "jittered_block": 0.3}


@functools.lru_cache(maxsize=None)
def full_multi_mesh(name):
    case = FULL_MULTI_CASES[name][0]
    if case in BLOCKS:
        from smoothmesh_amd.meshgen import hex_block
        return hex_block(6, 5, 4, jitter=BLOCKS[case])
    return CASES[case][0]()


def _over_and_n(name):
    case = FULL_MULTI_CASES[name][0]
    return ({}, 6) if case in BLOCKS else (CASES[case][1], CASES[case][2])


def full_limits_of(name):
    return {**OFF, **FULL_MULTI_CASES[name][2]}


@functools.lru_cache(maxsize=None)
def full_multi_reference(oracle_lib, name, variant="com", constraints=False, passes=2):
    """computed once per configuration and shared (tests/test_gpu_quality_constraint_full_multirank.py too)"""
    over, n = _over_and_n(name)
    r = QualityConstraintFullMultiReference(oracle_lib, full_multi_mesh(name), FULL_MULTI_CASES[name][1], full_limits_of(name), passes, variant,
                                            constraints, **over).run(n)
    ref = r["ref"]
    assert ref.minMargin > tangle_reference.MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    assert all(g > MORE_MARGIN for g in ref.minGap.values()), ref.minGap
    return r


@functools.lru_cache(maxsize=None)
def _serial(oracle_lib, name, constraints=False, passes=2):
    over, n = _over_and_n(name)
    return reference_run(oracle_lib, full_multi_mesh(name), n, limits=full_limits_of(name), passes=passes, constraints=constraints, **over)


def _assert_is_serial(ser, mul):
    ref = mul["ref"]
    assert mul["recs"] == ser["recs"]
    assert all(list(c) == list(FIELDS_FULL) for c in mul["recs"])
    assert sum(ref.nExemptCells) == ser["ref"].nExemptCells and sum(ref.nExemptFaces) == ser["ref"].nExemptFaces
    assert sum(ref.nExemptDeterminantCells) == ser["ref"].nExemptDeterminantCells
    for ps, pm in zip(ser["pts"], mul["pts"]):
        assert np.max(np.abs(ref.gather(pm) - ps)) <= 1e-12
        for r, p in enumerate(pm):      # copies of a shared point are identical
            assert np.array_equal(ref.gather(pm)[ref.ppa[r]], p)


def _assert_invariant(mul):
    for pts in mul["pts"]:
        for faces, cells in mul["ref"].bad_now(pts):
            assert not faces.any() and not cells.any()


@pytest.mark.parametrize("name", list(FULL_MULTI_CASES))
def test_decomposed_run_is_the_serial_run(oracle_lib, name):
    ser, mul = _serial(oracle_lib, name), full_multi_reference(oracle_lib, name)
    _assert_is_serial(ser, mul)
    _assert_invariant(mul)
    ref, lim, procOn = mul["ref"], FULL_MULTI_CASES[name][2], FULL_MULTI_CASES[name][3]
    print(name, "processor-face verdicts", ref.procVerdictsMore, "determinant rule differs", ref.detRuleDiffers, "smallest gaps",
          {k: v for k, v in ref.minGap.items() if np.isfinite(v)}, "counts", {MORE[k][1]: max(c[MORE[k][1]] for c in mul["recs"]) for k in lim if k in MORE})
    if FULL_MULTI_CASES[name][0] not in BLOCKS:
        for k in lim:
            if k in MORE:
                assert any(c[MORE[k][1]] > 0 for c in mul["recs"]) or name.startswith("all_"), "no limit is met: the case tests nothing"
    # conditions on the inputs: the cut runs through faces that fail the criterion, their two cells on two ranks
    for k in FACE_LIMITS:
        assert (ref.procVerdictsMore[k] > 0) == (k in procOn), (k, ref.procVerdictsMore)


def test_every_face_criterion_that_crosses_ranks_has_a_row():
    covered = {k for row in FULL_MULTI_CASES.values() for k in row[3]}
    assert covered >= {"minTetQuality", "minTwist", "minFaceWeight", "minVolRatio"}


@pytest.mark.parametrize("name", ["block_211", "jittered_block_211", "determinant_811"])
def test_determinant_runs_over_the_processor_faces(oracle_lib, name):
    """cells on the cut have another determinant verdict under the serial face rule (a cube: 0.5 in place of 1); the exempt cells
    summed over the ranks are those of the undecomposed mesh"""
    ser, mul = _serial(oracle_lib, name), full_multi_reference(oracle_lib, name)
    ref = mul["ref"]
    assert ref.detRuleDiffers > 0
    assert sum(ref.nExemptDeterminantCells) == ser["ref"].nExemptDeterminantCells
    if name == "block_211":            # 6 x 5 x 4 cubes: the cells on the physical boundary and no other, none for lying on the cut
        m = full_multi_mesh(name)
        onBoundary = np.zeros(m.nCells, bool)
        onBoundary[m.owner[m.nInternalFaces:]] = True
        assert sum(ref.nExemptDeterminantCells) == int(onBoundary.sum()) == 120 - 4 * 3 * 2
        assert np.array_equal(ser["ref"].exemptDet, onBoundary)


def test_the_reference_constraints_on(oracle_lib):
    mul = full_multi_reference(oracle_lib, "all_811", "com", True, 2)
    _assert_is_serial(_serial(oracle_lib, "all_811", True, 2), mul)
    assert all(v > 0 for v in mul["ref"].procVerdictsMore.values())


@pytest.mark.parametrize("passes", [0, 1])
@pytest.mark.parametrize("name", ["weight_811", "all_221", "tiles_weight_611"])     # (rows whose full reverts count the same moved points on both meshes)
def test_fewer_passes(oracle_lib, name, passes):
    ser, mul = _serial(oracle_lib, name, False, passes), full_multi_reference(oracle_lib, name, "com", False, passes)
    _assert_is_serial(ser, mul)
    _assert_invariant(mul)
    if passes == 0:
        assert any(r["fullRevert"] for r in ser["recs"]), "no full revert: the case tests nothing"
    assert all(r["passes"] <= passes for rr in mul["per_rank"] for r in rr)


@pytest.mark.parametrize("name", ["all_221", "all_811"])
def test_all_nine_criteria_together(oracle_lib, name):
    mul = full_multi_reference(oracle_lib, name)
    ref = mul["ref"]
    assert all(ref.on.values()) and ref.maxNonOrtho < 180.0 and ref.maxInternalSkewness > 0.0 and ref.maxBoundarySkewness > 0.0
    assert sum(ref.nExemptDeterminantCells) == 4 and sum(ref.nExemptCells) == 0
    assert sum(c["nBadCells"] > 0 for c in mul["recs"]) >= 2


def test_all_six_off_is_the_parent_reference(oracle_lib):
    case, grid, n = "cavity_interface", (8, 1, 1), CASES["cavity_interface"][2]
    lim = {**OFF, **dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, maxBoundarySkewness=0.5)}
    m = CASES[case][0]()
    a = QualityConstraintFullMultiReference(oracle_lib, m, grid, {**lim, **{k: None for k in MORE}}, 2, "com", False, **CASES[case][1]).run(n)
    b = QualityConstraintMultiReference(oracle_lib, m, grid, lim, 2, "com", False, **CASES[case][1]).run(n)
    assert [[{k: c[k] for k in FIELDS} for c in rr] for rr in a["per_rank"]] == b["per_rank"] and any(c["nBadCells"] > 0 for c in b["recs"])
    assert [{k: c[k] for k in FIELDS} for c in a["recs"]] == b["recs"]
    assert all(c[MORE[k][1]] == 0 for c in a["recs"] for k in MORE)
    for pa, pb in zip(a["pts"], b["pts"]):
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert all(np.array_equal(x, y) for x, y in zip(a["ref"].exemptFaces, b["ref"].exemptFaces))
    assert a["ref"].nExemptFaces == b["ref"].nExemptFaces and sum(a["ref"].nExemptDeterminantCells) == 0
    # the off values themselves are off
    c = QualityConstraintFullMultiReference(oracle_lib, m, grid, {**lim, **{k: v[0] for k, v in MORE.items()}}, 2, "com", False, **CASES[case][1]).run(n)
    assert c["per_rank"] == a["per_rank"]
    assert set(SUMMED_FULL) | {"iteration", "passes", "fullRevert"} == set(FIELDS_FULL)


def test_ctypes_mirror_of_the_full_descriptor_has_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    cname, mirror, old = "smgpu_quality_constraint_halo_desc_full", _ffi.QualityConstraintHaloDescFull, _ffi.QualityConstraintHaloDesc
    body = f'    printf("size %zu\\n", sizeof({cname}));\n    printf("old %zu\\n", sizeof(smgpu_quality_constraint_halo_desc));\n'
    body += "".join(f'    printf("{n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    body += "".join(f'    printf("old_{n} %zu\\n", offsetof(smgpu_quality_constraint_halo_desc, {n}));\n' for n, _ in old._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    got = {a: int(v) for a, v in (line.split() for line in out if line)}
    new = {k: v for k, v in got.items() if k != "old" and not k.startswith("old_")}
    assert new == {"size": C.sizeof(mirror), **{n: getattr(mirror, n).offset for n, _ in mirror._fields_}}
    assert new == dict(size=56, sendT=0, recvT=8, sendCc=16, recvCc=24, coupling=32, sendVc=40, recvVc=48)
    # the old descriptor is its head, in the header and in the mirrors
    assert got["old"] == C.sizeof(old) == 40 == new["sendVc"]
    assert all(got[f"old_{n}"] == new[n] == getattr(old, n).offset for n, _ in old._fields_)
    assert mirror._fields_[:len(old._fields_)] == old._fields_
    assert "smgpu_set_quality_constraint_limits_coupled" in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports it
