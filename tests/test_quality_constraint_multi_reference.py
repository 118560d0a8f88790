"""The CPU restatement of the quality constraint on a decomposed mesh (tests/quality_constraint_multi_reference.py; DESIGN.md "Mesh
quality", 10.15) against the serial restatement (tests/quality_constraint_reference.py): cut into boxes, with the neighbour rank's
cell centre behind every processor face, the marks OR-ed over the copies of shared points and the verdict taken on the summed
count, the run has the records and the points of the undecomposed one.  The cuts are the ones at which a coupled implementation
can go wrong: bad faces that lie on the cut, with their two cells on two ranks.  Also the ctypes mirror of
smgpu_quality_constraint_halo_desc against the header."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from quality_constraint_multi_reference import FACE_MARGIN, MARGIN, OFF, SHARED, QualityConstraintMultiReference
from quality_constraint_reference import reference_run
from tangle_multi_reference import TangleMultiReference
from test_gpu_tangle import CASES
from test_quality_reference import tangled_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEW = dict(maxInternalSkewness=0.4)
BOTH = dict(maxInternalSkewness=0.4, maxBoundarySkewness=0.1)
CAVITY = dict(maxNonOrtho=40.0, maxInternalSkewness=0.5, maxBoundarySkewness=0.5)
# name -> (mesh of CASES, cut, the limits (a criterion not named is off), iterations, whether a processor face is ever found bad)
MULTI_CASES = {
    "dented_221": ("dented", (2, 2, 1), SKEW, 8, True),          # every bad face is a processor face, every bad cell on another rank
    "dented_211": ("dented", (2, 1, 1), SKEW, 8, True),
    "tiles_611": ("dented_tiles", (6, 1, 1), SKEW, 12, True),
    "tiles_611_both": ("dented_tiles", (6, 1, 1), BOTH, 6, True),
    "tiles_431": ("dented_tiles", (4, 3, 1), SKEW, 8, False),    # the marks alone cross the ranks
    "cavity_811": ("cavity_interface", (8, 1, 1), CAVITY, 10, True),   # non-orthogonality, on the polyhedral interface
    "cavity_221": ("cavity_interface", (2, 2, 1), CAVITY, 10, False),
}


@functools.lru_cache(maxsize=None)
def multi_mesh(name):
    return CASES[MULTI_CASES[name][0]][0]()


def limits_of(name):
    return {**OFF, **MULTI_CASES[name][2]}


@functools.lru_cache(maxsize=None)
def multi_reference(oracle_lib, name, variant="com", constraints=False, passes=2):
    """computed once per configuration and shared (tests/test_gpu_quality_constraint_multirank.py too)"""
    case, grid, _, n, _ = MULTI_CASES[name]
    r = QualityConstraintMultiReference(oracle_lib, multi_mesh(name), grid, limits_of(name), passes, variant, constraints, **CASES[case][1]).run(n)
    ref = r["ref"]
    assert ref.minMargin > MARGIN and ref.minCosGap > FACE_MARGIN and ref.minSkewGap > FACE_MARGIN
    return r


@functools.lru_cache(maxsize=None)
def _serial(oracle_lib, name, constraints, passes):
    case, _, _, n, _ = MULTI_CASES[name]
    return reference_run(oracle_lib, multi_mesh(name), n, limits=limits_of(name), passes=passes, constraints=constraints, **CASES[case][1])


def _assert_is_serial(ser, mul):
    ref = mul["ref"]
    assert mul["recs"] == ser["recs"]
    assert sum(ref.nExemptCells) == ser["ref"].nExemptCells and sum(ref.nExemptFaces) == ser["ref"].nExemptFaces
    for ps, pm in zip(ser["pts"], mul["pts"]):
        assert np.max(np.abs(ref.gather(pm) - ps)) <= 1e-12
        for r, p in enumerate(pm):      # copies of a shared point are identical
            assert np.array_equal(ref.gather(pm)[ref.ppa[r]], p)


@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_decomposed_run_is_the_serial_run(oracle_lib, name):
    ser, mul = _serial(oracle_lib, name, False, 2), multi_reference(oracle_lib, name)
    _assert_is_serial(ser, mul)
    ref = mul["ref"]
    assert any(r["nNonOrthoFaces"] + r["nSkewFaces"] > 0 for r in mul["recs"]), "no face is ever over a limit: the case tests nothing"
    # conditions on the inputs: where the cut is meant to run through bad faces, a verdict without recvCc would be another one
    assert (ref.procVerdicts > 0) == MULTI_CASES[name][4], ref.procVerdicts
    if name == "dented_221":
        assert ref.procOnlyCells > 0                               # cells bad through nothing but a processor face


def test_the_reference_constraints_on(oracle_lib):
    _assert_is_serial(_serial(oracle_lib, "tiles_611", True, 2), multi_reference(oracle_lib, "tiles_611", "com", True, 2))


@pytest.mark.parametrize("passes", [0, 1])
@pytest.mark.parametrize("name", ["dented_221", "tiles_611_both"])
def test_fewer_passes(oracle_lib, name, passes):
    ser, mul = _serial(oracle_lib, name, False, passes), multi_reference(oracle_lib, name, "com", False, passes)
    _assert_is_serial(ser, mul)
    if passes == 0 or name == "tiles_611_both":     # (one marked pass heals every iteration of dented_221)
        assert any(r["fullRevert"] for r in ser["recs"]), "no full revert: the case tests nothing"
    assert all(r["passes"] <= passes for rr in mul["per_rank"] for r in rr)


def test_full_revert_of_the_boundary_limit_run(oracle_lib):
    """dented_tiles cut (6,1,1) under both skewness limits ends iterations with the full revert at passes = 2 too"""
    mul = multi_reference(oracle_lib, "tiles_611_both")
    assert any(r["fullRevert"] for r in mul["recs"])
    for rr in mul["per_rank"]:          # ... on every rank, with or without bad cells of its own
        assert [r["fullRevert"] for r in rr] == [r["fullRevert"] for r in mul["recs"]]


@pytest.mark.parametrize("name", ["dented_221", "tiles_431"])
def test_all_criteria_off_is_the_tangle_constraint(oracle_lib, name):
    case, grid, _, n, _ = MULTI_CASES[name]
    q = QualityConstraintMultiReference(oracle_lib, multi_mesh(name), grid, OFF, 2, "com", False, **CASES[case][1]).run(n)
    t = TangleMultiReference(oracle_lib, multi_mesh(name), grid, 2, "com", False, **CASES[case][1]).run(n)
    assert [[{k: r[k] for k in SHARED} for r in rr] for rr in q["per_rank"]] == t["per_rank"]
    assert all(r["nTangledCells"] == r["nBadCells"] and r["nNonOrthoFaces"] == r["nSkewFaces"] == 0 for rr in q["per_rank"] for r in rr)
    for pq, pt in zip(q["pts"], t["pts"]):
        assert all(np.array_equal(a, b) for a, b in zip(pq, pt))
    assert any(r["nBadCells"] > 0 for r in t["recs"]), "the mesh does not tangle: the case tests nothing"


def test_exempt_elements_of_a_tangled_block(oracle_lib):
    m, over, n = tangled_block(), dict(maxStepLength=0.01), 6
    lim = {**OFF, "maxInternalSkewness": 0.4}
    ser = reference_run(oracle_lib, m, n, limits=lim, constraints=False, **over)
    mul = QualityConstraintMultiReference(oracle_lib, m, (2, 1, 1), lim, 2, "com", False, **over).run(n)
    _assert_is_serial(ser, mul)
    assert sum(mul["ref"].nExemptCells) == ser["ref"].nExemptCells > 0


def test_ctypes_mirror_of_the_descriptor_has_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    cname, mirror = "smgpu_quality_constraint_halo_desc", _ffi.QualityConstraintHaloDesc
    body = f'    printf("size %zu\\n", sizeof({cname}));\n' + "".join(f'    printf("{n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    got = {a: int(v) for a, v in (line.split() for line in out if line)}
    assert got == {"size": C.sizeof(mirror), **{n: getattr(mirror, n).offset for n, _ in mirror._fields_}}
    assert got == dict(size=40, sendT=0, recvT=8, sendCc=16, recvCc=24, coupling=32)
    for sym in ("smgpu_set_quality_constraint_coupled", "smgpu_quality_constraint_coupled_exempt", "smgpu_quality_constraint_pass_begin",
                "smgpu_quality_constraint_pass_faces", "smgpu_quality_constraint_pass_end"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them
