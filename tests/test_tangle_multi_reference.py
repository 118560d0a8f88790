"""The CPU restatement of the tangle constraint on a decomposed mesh (tests/tangle_multi_reference.py; DESIGN.md "Mesh quality",
10.13) against the serial restatement (tests/tangle_reference.py): cut into boxes, with the marks OR-ed over the copies of shared
points and the verdict taken on the summed count, the run has the records and the points of the undecomposed one.  The cuts are
the ones at which a coupled implementation can go wrong and an uncoupled one visibly does: a rank without a bad cell of its own
that must put back shared points the loop had moved.  Also the ctypes mirror of smgpu_tangle_halo_desc against the header."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tangle_multi_reference import MARGIN, TangleMultiReference
from tangle_reference import reference_run
from test_gpu_quality_guard import dented_block_tiles
from test_gpu_quality_trace import dented_block
from test_quality_reference import tangled_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENT = dict(maxStepLength=1.0, minEdgeLength=1e-4)
TILES = dict(maxStepLength=0.03, minEdgeLength=1e-4)
# name -> (mesh, cut, parameters that make it tangle, iterations)
MULTI_CASES = {
    "dented_112": (dented_block, (1, 1, 2), DENT, 8),
    "dented_221": (dented_block, (2, 2, 1), DENT, 8),
    "tiles_411": (dented_block_tiles, (4, 1, 1), TILES, 12),
    "tiles_431": (dented_block_tiles, (4, 3, 1), TILES, 12),
}
# the cuts in which a rank without a bad cell receives marks on moved points (the reference's constraints off)
FOREIGN = ("dented_112", "tiles_411", "tiles_431")


@functools.lru_cache(maxsize=None)
def multi_mesh(name):
    return MULTI_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def multi_reference(oracle_lib, name, variant="com", constraints=False, passes=2):
    """computed once per configuration and shared (tests/test_gpu_tangle_multirank.py too): TangleMultiReference.run"""
    _, grid, over, n = MULTI_CASES[name]
    r = TangleMultiReference(oracle_lib, multi_mesh(name), grid, passes, variant, constraints, **over).run(n)
    assert r["ref"].minMargin > MARGIN
    return r


@functools.lru_cache(maxsize=None)
def _serial(oracle_lib, name, constraints, passes):
    _, _, over, n = MULTI_CASES[name]
    return reference_run(oracle_lib, multi_mesh(name), n, passes=passes, constraints=constraints, **over)


@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("name", list(MULTI_CASES))
def test_decomposed_run_is_the_serial_run(oracle_lib, name, constraints):
    ser, mul = _serial(oracle_lib, name, constraints, 2), multi_reference(oracle_lib, name, "com", constraints, 2)
    ref = mul["ref"]
    assert mul["recs"] == ser["recs"]
    assert sum(ref.nExemptCells) == ser["ref"].nExemptCells == 0
    for ps, pm in zip(ser["pts"], mul["pts"]):
        assert np.max(np.abs(ref.gather(pm) - ps)) <= 1e-12
        for r, p in enumerate(pm):      # copies of a shared point are identical
            assert np.array_equal(ref.gather(pm)[ref.ppa[r]], p)
    assert any(r["nBadCells"] > 0 for r in mul["recs"]), "the mesh does not tangle: the case tests nothing"
    if not constraints and name in FOREIGN:
        # a condition on the inputs: some rank has no bad cell in a pass in which it receives marks on points the loop moved
        assert any(nMoved > 0 for _, _, _, _, nMoved in ref.foreign), ref.foreign


@pytest.mark.parametrize("passes", [0, 1])
def test_fewer_passes_full_reverts_reach_the_rank_without_bad_cells(oracle_lib, passes):
    ser, mul = _serial(oracle_lib, "dented_112", False, passes), multi_reference(oracle_lib, "dented_112", "com", False, passes)
    assert mul["recs"] == ser["recs"]
    full = [r["iteration"] for r in ser["recs"] if r["fullRevert"]]
    assert full, "no full revert: the case tests nothing"
    start = [s.mesh.points for s in mul["ref"].subs]
    clean_rank_reverted = False
    for it in full:
        before = start if it == 1 else mul["pts"][it - 2]
        for r in range(mul["ref"].world):
            assert mul["per_rank"][r][it - 1]["fullRevert"] == 1
            assert np.array_equal(mul["pts"][it - 1][r], np.asarray(before[r]).reshape(-1, 3))
            clean_rank_reverted |= mul["per_rank"][r][it - 1]["nBadCells"] == 0
    assert clean_rank_reverted
    for ps, pm in zip(ser["pts"], mul["pts"]):
        assert np.max(np.abs(mul["ref"].gather(pm) - ps)) <= 1e-12


def test_tangled_block_cells_are_exempt_on_their_ranks(oracle_lib):
    from smoothmesh_amd.decompose import shared_point_table
    m = tangled_block()
    ref = TangleMultiReference(oracle_lib, m, (2, 1, 1), 2, "com", False, maxStepLength=0.01)
    assert sum(ref.nExemptCells) == 4
    r = ref.run(6)
    for k, c in enumerate(r["recs"], start=1):
        assert c == dict(iteration=k, passes=0, fullRevert=0, nBadCells=0, nPointsReverted=0)
    orcs = [oracle_lib.Oracle(s.mesh) for s in ref.subs]
    for o in orcs:
        o.set_params(ref.prm)
    free = oracle_lib.MultiOracle(orcs, *shared_point_table(ref.subs))
    assert free.iterate(6, 0.0)[0] == 6
    for o, p in zip(orcs, r["pts"][-1]):
        assert np.array_equal(o.points(), p)


def test_ctypes_mirror_of_the_halo_desc_has_the_headers_layout(tmp_path):
    from smoothmesh_amd import _ffi
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    cname, mirror = "smgpu_tangle_halo_desc", _ffi.TangleHaloDesc
    body = f'    printf("size %zu\\n", sizeof({cname}));\n'
    body += "".join(f'    printf("{n} %zu\\n", offsetof({cname}, {n}));\n' for n, _ in mirror._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "smgpu.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    got = {a: int(v) for a, v in (line.split() for line in out if line)}
    want = {"size": C.sizeof(mirror), **{n: getattr(mirror, n).offset for n, _ in mirror._fields_}}
    assert got == want
    for sym in ("smgpu_set_tangle_constraint_coupled", "smgpu_tangle_pass_begin", "smgpu_tangle_pass_end"):
        assert sym in _ffi.SYMBOLS
    _ffi.lib()                                                     # the library exports them
