"""The HIP engine against THE REFERENCE ITSELF (oracle/_ref/libsmref.so: the reference's own source on the stand-in OpenFOAM,
built by __graft_entry__.build(); see test_reference_pin.py for what that pins and what it does not).

Engine points bit-equal to the reference's after every iteration and equal nFrozenPoints, under the condition that the
engine met no near tie (eng.near_ties()["total"] == 0: the engine's acos may differ from glibc's in the last bit, and only a
comparison whose sides are within a few ulp could then go the other way).  The condition is asserted, not assumed, and so is
the oracle's own census with std::acos on the CPU side.  The library is REQUIRED here: a missing library fails, it does not skip."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_pin_cases as rp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "smoothmesh_amd", "bin", "smoothMesh")


def _ref():
    from oracle import ref_ffi
    assert ref_ffi.available("com") and ref_ffi.available("org"), "oracle/_ref/libsmref.so is missing: __graft_entry__.build() makes it"
    return ref_ffi


def _engine_series(mesh, argv, variant):
    from smoothmesh_amd import SmoothEngine
    e = SmoothEngine(mesh)
    e.set_foam_variant(variant)
    prm, lay, layerEdgeLength, iters, relTol = rp.configure(mesh, argv, e.mesh_stats()[0])
    e.set_params(prm)
    on = False
    if lay is not None:
        lay.layerEdgeLength = layerEdgeLength
        on = e.set_layers(lay, prm.minEdgeLength)
    pts, frz, res = [], [], []
    for _ in range(iters):
        n, r, f = e.iterate(1, relTol)
        assert n == 1
        pts.append(e.get_points().copy()); frz.append(int(f[0])); res.append(float(r[0]))
        if r[0] < relTol:
            break
    return e, pts, np.array(frz, np.int64), res, on


def _pin(oracle_lib, mesh, text, variant="com", layers=None):
    ref = _ref()
    argv = rp.args(text)
    r = ref.run(mesh, argv, variant)
    # the oracle with std::acos, counting its near ties: the case must be free of them on the CPU already
    oracle_lib.set_acos_variant("glibc")
    oracle_lib.acos_census_window(4)
    oracle_lib.acos_census(True)
    try:
        pts_o, frz_o, res_o, _ = rp.oracle_series(oracle_lib, mesh, argv, variant)
        census = oracle_lib.acos_census(False)
    finally:
        oracle_lib.acos_census(False)
    rp.assert_same_run(r, pts_o, frz_o, res_o, "oracle: " + text)
    assert sum(census["near"].values()) == 0, census
    e, pts, frz, res, on = _engine_series(mesh, argv, variant)
    assert e.near_ties()["total"] == 0, e.near_ties()
    rp.assert_same_run(r, pts, frz, res, "engine: " + text)
    if layers is not None:
        assert on == layers and ("Enabled boundary layer treatment" in r.log) == layers
    return r


def test_constraints_on(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    nB = lambda m: m.nPoints - int(np.count_nonzero(m.find_internal_points()))
    m = hex_block(10, 9, 8, jitter=0.45, seed=3)
    r = _pin(oracle_lib, m, "-centroidalIters 10 -relTol 0 -minAngle 50 -maxAngle 140")
    assert r.nFrozenPoints.max() > nB(m)
    r = _pin(oracle_lib, m, "-centroidalIters 10 -relTol 0 -minEdgeLength 0.06 -totalMinFreeze true -relStepFrac 0.9")
    assert r.nFrozenPoints.max() > nB(m)


def test_layers(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    m = hex_block(10, 9, 8, jitter=0.3, seed=8)
    _pin(oracle_lib, m, "-centroidalIters 10 -relTol 0 -layerPatches '(\"x.*\" zmin)' -minLayers 0 -maxLayers 3 -layerMaxBlendingFraction 0.6 "
         "-layerExpansionRatio 1.2 -layerEdgeLength 0.05", layers=True)


@pytest.mark.parametrize("variant", ["com", "org"])
def test_polyhedral(oracle_lib, variant):
    from smoothmesh_amd.polymesh import cavity_mesh
    _pin(oracle_lib, cavity_mesh(10, jitter=0.3, seed=2), "-centroidalIters 8 -relTol 0 -layerPatches cavity -maxLayers 3", variant, layers=True)
    _pin(oracle_lib, rp.fan_mesh(12), "-centroidalIters 8 -relTol 0", variant)


def test_defaults(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    r = _pin(oracle_lib, hex_block(10, 9, 8, jitter=0.45, seed=3), "")
    assert "Residual reached relTol, stopping." in r.log


def test_block_30(oracle_lib):
    from smoothmesh_amd.meshgen import hex_block
    _pin(oracle_lib, hex_block(30, jitter=0.3, seed=7), "-centroidalIters 6 -relTol 0")


def test_front_end_log_lines(oracle_lib, tmp_path):
    """every line that the `smoothMesh` front-end prints like the reference, against the reference's ACTUAL line on the same
    case: the parameter block, the mesh summary, the per-iteration lines, the stopping and writing lines"""
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import write_case
    m = hex_block(8, 7, 6, jitter=0.3, seed=5)
    text = "-centroidalIters 40 -relTol 0.3 -minAngle 20 -layerPatches '(xmin \"y.*\")' -layerExpansionRatio 1.2"
    r = _ref().run(m, rp.args(text))
    write_case(str(tmp_path), m, binary=True, writeFormat="binary")
    out = subprocess.run([BIN, "-case", str(tmp_path)] + rp.args(text), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # a line "like the reference" = a line that, numbers aside, the reference prints too: it must then be the reference's line
    stem = lambda l: re.sub(r"[-+]?\d[\d.]*(e[-+]?\d+)?", "#", l.strip())
    skip = ("ClockTime",)
    want = {}
    for l in r.log.splitlines():
        if l.strip() and not l.startswith(skip):
            want.setdefault(stem(l), set()).add(l.strip())
    lines = out.stdout.splitlines()
    lines = lines[next(i for i, l in enumerate(lines) if l.startswith("Patches for boundary layer treatment")):]
    print("\n".join(lines))
    alike = [l.strip() for l in lines if l.strip() and not l.startswith(skip) and stem(l) in want]
    wrong = [l for l in alike if l not in want[stem(l)]]
    assert not wrong, (wrong, [sorted(want[stem(l)]) for l in wrong])
    # and the comparison covered the parameter block, the mesh summary, every iteration line, the stopping and the writing line
    n = len(r.nFrozenPoints)
    assert len([l for l in alike if l.startswith("Smoothing iteration=")]) == n
    for head in ("centroidalIters", "relTol", "minEdgeLength", "maxStepLength", "relStepFrac", "totalMinFreeze", "edgeAngleConstraint",
                 "faceAngleConstraint", "minAngle", "maxAngle", "layerMaxBlendingFraction", "layerEdgeLength", "layerExpansionRatio",
                 "minLayers", "maxLayers", "Mesh includes a total of", "- ", "Mesh minimum edge length", "Mesh maximum edge length",
                 "Patches for boundary layer treatment", "Patches for boundary point smoothing", "Enabled boundary layer treatment",
                 "Residual reached relTol, stopping.", "Writing new mesh to time"):
        assert any(l.startswith(head) for l in alike), head
