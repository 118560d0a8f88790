"""The oracle against THE REFERENCE ITSELF: oracle/_ref/libsmref.so is the reference's own source, compiled against the
stand-in OpenFOAM of oracle/foam_shim/ and executed in serial (oracle/ref_ffi.py, oracle/ref_driver.cpp).

Same mesh, same addressing, same geometry, same options on both sides, std::acos on both sides
(set_acos_variant("glibc")), -ffp-contract=off on both sides.  Required: BIT-EQUAL points after every iteration, equal
nFrozenPoints series, residuals equal as the reference prints them (six significant digits).  No tolerance anywhere.

What this pins is what the reference's program text decides (arithmetic, control flow, defaults, option handling, the freeze
walk, the layer treatment, the log).  What it does not pin is what OpenFOAM decides and the harness hands over: the
addressing orders, the primitiveMesh geometry, four recalled constants, parallel syncTools.  Boundary point
smoothing (constant/geometry/*.obj) is not part of the stand-in: no case here enables it.

The tests skip only where the library is absent AND the reference's source is absent too (then it cannot be built)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_pin_cases as rp


@pytest.fixture(scope="module")
def ref(oracle_lib):
    from oracle import ref_ffi
    if not (ref_ffi.available("com") and ref_ffi.available("org")):
        if not ref_ffi.source_present():
            pytest.skip("oracle/_ref/libsmref.so is absent and so is the reference's source: nothing to run")
        ref_ffi.build()
    assert ref_ffi.available("com") and ref_ffi.available("org")
    return ref_ffi


@pytest.fixture(autouse=True)
def glibc_acos(oracle_lib):
    oracle_lib.set_acos_variant("glibc")
    yield
    oracle_lib.set_acos_variant("glibc")


def _pin(ref, oracle_lib, mesh, text, variant="com", freezes=False, layers=None):
    argv = rp.args(text)
    r = ref.run(mesh, argv, variant)
    pts, frz, res, on = rp.oracle_series(oracle_lib, mesh, argv, variant)
    rp.assert_same_run(r, pts, frz, res, text)
    if freezes:      # a constrained case in which the walk freezes nothing proves nothing
        nBoundary = mesh.nPoints - int(np.count_nonzero(mesh.find_internal_points()))
        assert r.nFrozenPoints.max() - nBoundary > 0, (text, r.nFrozenPoints.tolist(), nBoundary)
    if layers is not None:
        assert on == layers and ("Enabled boundary layer treatment" in r.log) == layers
    assert "Boundary point smoothing is disabled" in r.log
    return r, pts, frz, res


def _block(jitter=0.45, seed=3, dims=(10, 9, 8)):
    from smoothmesh_amd.meshgen import hex_block
    return hex_block(*dims, jitter=jitter, seed=seed)


# ---- the constants and single functions ---------------------------------------------------------------------------------
def test_recalled_constants(ref, oracle_lib):
    """GREAT, VGREAT, SMALL, VSMALL, ROOTVSMALL are recalled values of OpenFOAM's doubleScalar.H on BOTH sides (VERDICT row a14):
    this reports what the stand-in holds and checks that the oracle and the stand-in hold the same"""
    c = ref.Functions().constants()
    print("stand-in constants:", c)
    assert c == {"GREAT": 1e15, "VGREAT": 1e300, "SMALL": 1e-15, "VSMALL": 1e-300, "ROOTVSMALL": 1e-150}


def test_angle_functions_bitwise(ref, oracle_lib):
    """edgeEdgeAngle (SM.C:766-786) and calcEdgeCenterEdgeAngle (SM.C:980-998) on random, clamped and degenerate-near arguments"""
    f = ref.Functions()
    rng = np.random.default_rng(11)
    for k in range(400):
        c, p1, p2 = rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-3, 4)
        if k % 4 == 0:
            p2 = c + (p1 - c) * rng.uniform(0.5, 2.0) * (1 if k % 8 else -1) + 1e-9 * rng.standard_normal(3)   # nearly (anti)parallel: the clamp
        assert f.edgeEdgeAngle(c, p1, p2) == oracle_lib.edgeEdgeAngle(c, p1, p2)
        u = [v / np.linalg.norm(v) for v in (c, p1, p2)]
        assert f.calcEdgeCenterEdgeAngle(*u) == oracle_lib.calcEdgeCenterEdgeAngle(*u)
    x = np.array([1.0, 0.0, 0.0])
    assert f.calcEdgeCenterEdgeAngle(x, x, x) == oracle_lib.calcEdgeCenterEdgeAngle(x, x, x) == 2.0 * np.arccos(0.99999)
    assert f.calcEdgeCenterEdgeAngle(x, -x, x) == oracle_lib.calcEdgeCenterEdgeAngle(x, -x, x)


def test_is_closer_point(ref, oracle_lib):
    """isCloserPoint / isSmallerByVectorElements (SM.C:222-272), with exact ties of length"""
    f = ref.Functions()
    rng = np.random.default_rng(5)
    base = [np.array(v, float) for v in ([1, 2, 2], [2, 1, 2], [2, 2, 1], [-1, 2, 2], [3, 0, 0], [0, 0, 3], [0, 0, 0], [1, 2, 2])]
    pairs = [(a, b) for a in base for b in base] + [tuple(rng.integers(-3, 4, size=(2, 3)).astype(float)) for _ in range(300)]
    for a, b in pairs:
        assert f.isCloserPoint(a, b) == oracle_lib.isCloserPoint(a, b), (a, b)
    assert f.isSmallerByVectorElements([1, 2, 3], [1, 2, 4]) and not f.isSmallerByVectorElements([1, 2, 3], [1, 2, 3])
    assert f.isSmallerByVectorElements([0, 9, 9], [1, 0, 0]) and not f.isSmallerByVectorElements([1, 0, 0], [0, 9, 9])


def test_ar_smoothing_ratio_known_values(ref):
    """calcARSmoothingRatio (SM.C:489-543): the blending ramps of internal and boundary points, as the reference computes them"""
    f = ref.Functions()
    e = lambda L: np.array([L, 0.0, 0.0])
    assert f.calcARSmoothingRatio(e(1), e(1.2), e(1.2 * 3.0), False, True) == 1.0
    assert f.calcARSmoothingRatio(e(1), e(1.2), e(1.2 * 2.25), False, True) == (2.25 - 1.5) / (3.0 - 1.5)
    assert f.calcARSmoothingRatio(e(1), e(1.6), e(1.6 * 3.0), False, True) == 0.0      # first two not similar
    assert f.calcARSmoothingRatio(e(1), e(1.2), e(1.2 * 3.0), True, True) == 0.0       # common cell
    assert f.calcARSmoothingRatio(e(0), e(1.2), e(3.0), False, True) == 0.0            # zero vector
    assert f.calcARSmoothingRatio(e(1), e(1.5), e(9), False, False) == 0.5             # boundary point ramp 1..2
    assert f.calcARSmoothingRatio(e(1), e(4), e(9), False, False) == 1.0


def test_final_projected_angle(ref, oracle_lib):
    """calcMinMaxFinalProjectedAngle (SM.C:1003-1037) = min / max over the cells of calcEdgeCenterEdgeAngle of the cell's face pair"""
    f = ref.Functions()
    rng = np.random.default_rng(2)
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None]
    p, c = unit(rng.standard_normal((5, 3))), unit(rng.standard_normal((4, 3)))
    f0, f1 = np.array([0, 1, 2, 3]), np.array([1, 2, 3, 4])
    lo, hi = f.calcMinMaxFinalProjectedAngle(p, c, f0, f1)
    each = [oracle_lib.calcEdgeCenterEdgeAngle(p[a], cc, p[b]) for a, b, cc in zip(f0, f1, c)]
    assert lo == min(each) and hi == max(each)


def test_mesh_stats(ref, oracle_lib):
    """getMeshStats (SM.C:1478-1541): minimum and maximum edge length bit-equal to the oracle's"""
    from smoothmesh_amd.polymesh import cavity_mesh
    for m in (_block(), cavity_mesh(8, jitter=0.2, seed=4), rp.fan_mesh(7)):
        lo, hi, per = ref.mesh_stats(m)
        assert (lo, hi) == oracle_lib.Oracle(m).mesh_stats()


# ---- whole runs: constraints ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constraints", ["-edgeAngleConstraint false -faceAngleConstraint false", "-faceAngleConstraint false",
                                         "-edgeAngleConstraint false", ""])
@pytest.mark.parametrize("jitter", [0.1, 0.3, 0.45])
def test_constraint_switches(ref, oracle_lib, constraints, jitter):
    _pin(ref, oracle_lib, _block(jitter, seed=int(jitter * 100)), "-centroidalIters 10 -relTol 0 " + constraints,
         freezes=(jitter == 0.45 and "-faceAngleConstraint false" not in constraints))


def test_edge_angle_constraint_alone_freezes(ref, oracle_lib):
    """the edge-angle rule (SM.C:900-930) on its own, with a limit high enough that it freezes points"""
    _pin(ref, oracle_lib, _block(0.45, seed=45), "-centroidalIters 10 -relTol 0 -faceAngleConstraint false -minAngle 75", freezes=True)


@pytest.mark.parametrize("minAngle", [15, 35, 50])
@pytest.mark.parametrize("maxAngle", [140, 160, 175])
def test_angle_limits(ref, oracle_lib, minAngle, maxAngle):
    _pin(ref, oracle_lib, _block(0.45, seed=minAngle + maxAngle), f"-centroidalIters 8 -relTol 0 -minAngle {minAngle} -maxAngle {maxAngle}",
         freezes=True)


@pytest.mark.parametrize("text", [
    "-totalMinFreeze true -minEdgeLength 0.06",
    "-totalMinFreeze false -minEdgeLength 0.06",
    "-minEdgeLength 0.09 -maxStepLength 0.004 -relStepFrac 0.3",
    "-minEdgeLength 0.02 -maxStepLength 0.03 -relStepFrac 0.9",          # more than half of minEdgeLength: the WARNING branch
    "-maxStepLength 0.01 -relStepFrac 1.0 -edgeAngleConstraint false",
])
def test_lengths_and_steps(ref, oracle_lib, text):
    m = _block(0.4, seed=9)
    r, *_ = _pin(ref, oracle_lib, m, "-centroidalIters 10 -relTol 0 " + text, freezes=True)
    prm = rp.configure(m, rp.args(text), oracle_lib.Oracle(m).mesh_stats()[0])[0]
    assert ("WARNING: The maximum allowed step length is more than half" in r.log) == (prm.maxStepLength > 0.5 * prm.minEdgeLength)


# ---- stopping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,line", [("-centroidalIters 100", "Residual reached relTol, stopping."),
                                       ("-centroidalIters 100 -relTol 0.5", "Residual reached relTol, stopping."),
                                       ("-centroidalIters 6 -relTol 1e-9", "Maximum centroidalIters reached, stopping.")])
def test_relTol_stopping(ref, oracle_lib, text, line):
    r, pts, frz, res = _pin(ref, oracle_lib, _block(0.2, seed=1, dims=(8, 8, 8)), text)
    other = ({"Residual reached relTol, stopping.", "Maximum centroidalIters reached, stopping."} - {line}).pop()
    assert line in r.log and other not in r.log
    assert 1 < len(pts) <= 100
    # the mesh is written once, at the end, under the time of the last iteration, and it is the last iteration's points
    assert [n for n, _ in r.written] == [str(len(pts))] and np.array_equal(r.written[0][1], pts[-1])


def test_write_interval(ref, oracle_lib):
    """SM.C:2416: a write every writeInterval iterations, but never after the first iteration unless it is the last"""
    r, pts, *_ = _pin(ref, oracle_lib, _block(0.3, seed=2, dims=(6, 6, 6)), "-centroidalIters 7 -relTol 0 -writeInterval 2")
    assert [n for n, _ in r.written] == ["2", "4", "6", "7"]
    for n, p in r.written:
        assert np.array_equal(p, pts[int(n) - 1])


# ---- defaults -----------------------------------------------------------------------------------------------------------------
def test_defaults(ref, oracle_lib):
    """a run without a numeric option: default_params / LayerParams against what the reference derives (SM.C:1857-1918), seen
    through its log AND through its results (1000 iterations allowed, relTol 0.02 stops it)"""
    from smoothmesh_amd import LayerParams, default_params
    m = _block(0.45, seed=3)
    r, pts, frz, res = _pin(ref, oracle_lib, m, "", freezes=True)
    lo, hi = oracle_lib.Oracle(m).mesh_stats()
    prm, L = default_params(lo), LayerParams()
    said = dict(l.split() for l in r.log.splitlines() if l.startswith("    ") and len(l.split()) == 2)
    want = {"centroidalIters": "1000", "relTol": "0.02", "minEdgeLength": rp.printed(prm.minEdgeLength), "maxStepLength": rp.printed(prm.maxStepLength),
            "relStepFrac": rp.printed(prm.relStepFrac), "totalMinFreeze": str(int(prm.totalMinFreeze)), "edgeAngleConstraint": "true",
            "faceAngleConstraint": "true", "minAngle": rp.printed(prm.minAngle), "maxAngle": rp.printed(prm.maxAngle),
            "layerMaxBlendingFraction": rp.printed(L.layerMaxBlendingFraction), "layerEdgeLength": rp.printed(prm.minEdgeLength),
            "layerExpansionRatio": rp.printed(L.layerExpansionRatio), "minLayers": str(L.minLayers), "maxLayers": str(L.maxLayers)}
    assert said == want
    assert prm.edgeAngleConstraint and prm.faceAngleConstraint and prm.minEdgeLength == 0.5 * lo and prm.maxStepLength == 0.3 * (0.5 * lo)
    assert f"Mesh minimum edge length = {rp.printed(lo)}" in r.log and f"Mesh maximum edge length = {rp.printed(hi)}" in r.log
    assert "Residual reached relTol, stopping." in r.log and len(pts) < 1000


# ---- boundary layer treatment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [
    "-layerPatches xmin",
    "-layerPatches '(xmin ymax)' -layerExpansionRatio 1.2 -layerEdgeLength 0.05",
    "-layerPatches '(\"x.*\" zmin)' -minLayers 0 -maxLayers 3 -layerMaxBlendingFraction 0.6",
    "-layerPatches '(\".*\")' -minLayers 2 -maxLayers 5 -layerExpansionRatio 1.0 -layerEdgeLength 0.02",
    "-layerPatches '(\"[yz]m(in|ax)\")' -layerMaxBlendingFraction 0.2 -maxLayers 10",
])
def test_layers(ref, oracle_lib, text):
    _pin(ref, oracle_lib, _block(0.3, seed=8), "-centroidalIters 10 -relTol 0 " + text, layers=True)


@pytest.mark.parametrize("text", ["-layerPatches nosuchpatch", "-layerPatches '(\"w.*\")'", "-layerPatches xmin -layerMaxBlendingFraction 0"])
def test_layers_not_enabled(ref, oracle_lib, text):
    """no patch selected, or a zero blending fraction: SM.C:2024-2033"""
    r, *_ = _pin(ref, oracle_lib, _block(0.3, seed=8, dims=(6, 5, 4)), "-centroidalIters 5 -relTol 0 " + text, layers=False)
    assert "Boundary layer treatment is disabled." in r.log


def test_layers_on_curved_wall_and_baffles(ref, oracle_lib):
    from smoothmesh_amd.polymesh import cavity_mesh
    _pin(ref, oracle_lib, cavity_mesh(10, jitter=0.3, seed=2), "-centroidalIters 8 -relTol 0 -layerPatches cavity -maxLayers 3", layers=True)
    for split in (False, True):
        _pin(ref, oracle_lib, rp.baffle_mesh(split=split), "-centroidalIters 8 -relTol 0 -layerPatches '(xmin \"baffle.*\")'", layers=True)
        _pin(ref, oracle_lib, rp.baffle_mesh(split=split), "-centroidalIters 8 -relTol 0")


# ---- mesh kinds, OpenFOAM lines, ties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["com", "org"])
def test_foam_variants(ref, oracle_lib, variant):
    """the -DOPENFOAM_ORG build with the .org geometry against set_foam_variant("org"), and the same for .com"""
    from smoothmesh_amd.polymesh import cavity_mesh
    assert ref._load(variant).ref_is_org() == (variant == "org")
    _pin(ref, oracle_lib, _block(0.45, seed=3), "-centroidalIters 8 -relTol 0", variant, freezes=True)
    _pin(ref, oracle_lib, cavity_mesh(9, jitter=0.3, seed=5), "-centroidalIters 8 -relTol 0 -layerPatches '(cavity)'", variant, layers=True)
    _pin(ref, oracle_lib, rp.fan_mesh(9), "-centroidalIters 8 -relTol 0", variant)


@pytest.mark.parametrize("nSpokes", [5, 12, 20])
def test_valence_fan(ref, oracle_lib, nSpokes):
    _pin(ref, oracle_lib, rp.fan_mesh(nSpokes), "-centroidalIters 8 -relTol 0")
    _pin(ref, oracle_lib, rp.fan_mesh(nSpokes), "-centroidalIters 8 -relTol 0 -edgeAngleConstraint false -faceAngleConstraint false "
         "-minEdgeLength 0.3 -totalMinFreeze true")


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (3, 2, 1), (2, 2, 2), (16, 16, 16)])
def test_block_sizes(ref, oracle_lib, dims):
    _pin(ref, oracle_lib, _block(0.3, seed=3, dims=dims), "-centroidalIters 5 -relTol 0")


@pytest.mark.parametrize("shape", [(5, 6, 4, True, 3), (4, 4, 4, False, 1), (8, 5, 7, True, 9), (6, 6, 6, False, 4)])
def test_exact_ties(ref, oracle_lib, shape):
    """points on binary fractions: equal edge lengths are bit-equal, so the stable sortedOrder (SM.C:345-346), the strict
    comparisons of the freeze rules and isCloserPoint see exact ties"""
    m = rp.tied_mesh(*shape)
    _pin(ref, oracle_lib, m, "-centroidalIters 8 -relTol 0")
    _pin(ref, oracle_lib, m, "-centroidalIters 8 -relTol 0 -minEdgeLength 0.0625 -totalMinFreeze true -maxStepLength 0.015625")
    from smoothmesh_amd.meshgen import hex_block
    _pin(ref, oracle_lib, hex_block(6, 5, 4, jitter=0.0), "-centroidalIters 4 -relTol 0 -layerPatches '(\".*\")'", layers=True)


# ---- the reference's own command lines ---------------------------------------------------------------------------------------
def _reference_commands():
    """(case, options verbatim from testcaseN/run_serial, stand-in mesh as in test_gpu_reference_commands.py but smaller, iterations cap)"""
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    walls = lambda n, seed: rp.one_patch(hex_block(n, jitter=0.3, seed=seed), "walls")
    cav = cavity_mesh(12, jitter=0.2, seed=2)
    for p in cav.patches:
        p.name = {"cavity": "wall_sphere"}.get(p.name, p.name)
    top = hex_block(12, jitter=0.3, seed=5)
    for p in top.patches:
        p.name = {"ymax": "top"}.get(p.name, p.name)
    deff = hex_block(12, jitter=0.3, seed=1)
    for p in deff.patches:
        p.name = {"xmin": "defaultFaces", "xmax": "default2"}.get(p.name, p.name)
    return [
        ("testcase", "-centroidalIters 100 -minEdgeLength 0.01 -maxStepLength 0.002 -minAngle 15 -maxAngle 160 -layerPatches '(\"def.*\")'", deff),
        ("testcase2", "-centroidalIters 100 -minEdgeLength 0.05 -maxStepLength 0.05 -layerExpansionRatio 1.2 -maxLayers 10 -layerPatches '(wall_sphere)'", cav),
        ("testcase3", "-relTol 1e-8 -centroidalIters 200 -minAngle 15", hex_block(12, jitter=0.25, seed=3)),
        ("testcase4", "-centroidalIters 200 -layerExpansionRatio 1.2 -layerEdgeLength 0.05 -maxLayers 3 -layerPatches '(walls)' -smoothingPatches '(\".*\")'", walls(12, 4)),
        ("testcase5", "-centroidalIters 500 -minAngle 15 -layerExpansionRatio 1.2 -layerEdgeLength 0.05 -maxLayers 3 -layerPatches '(\"top\")' -smoothingPatches '(\".*\")'", top),
        ("testcase6", "-centroidalIters 300 -layerExpansionRatio 1.2 -layerEdgeLength 0.05 -maxLayers 3 -layerPatches '(walls \"baffle.*\")' -smoothingPatches '(\".*\")'",
         rp.baffle_mesh(split=True)),
        ("testcase7", "-centroidalIters 100 -layerPatches '(walls)'", walls(14, 7)),
        ("testcase8", "-centroidalIters 50", hex_block(12, jitter=0.3, seed=8)),
    ]


@pytest.mark.parametrize("k", range(8))
def test_reference_command_lines(ref, oracle_lib, k):
    """testcase*/run_serial, options verbatim, on stand-in meshes WITHOUT constant/geometry (so testcase3/4/5/6/8 run without
    their boundary point smoothing: that stage is not part of the stand-in)"""
    case, text, mesh = _reference_commands()[k]
    r, pts, *_ = _pin(ref, oracle_lib, mesh, text, layers=("-layerPatches" in text))
    assert len(pts) > 1
    assert f"Patches for boundary point smoothing: (\".*\")" in r.log


# ---- a seeded sweep, in the style of scripts/fuzz_parity.py (serial kinds) ---------------------------------------------------
def _sweep_case(k):
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    rng = np.random.default_rng(1000 + k)
    kind = rng.choice(["hex", "hex", "cavity", "tied", "baffle", "fan"])
    jitter = float(rng.choice([0.1, 0.3, 0.45]))
    seed = int(rng.integers(1 << 30))
    if kind == "hex":
        m = hex_block(*(int(x) for x in rng.integers(2, 12, size=3)), jitter=jitter, seed=seed)
    elif kind == "cavity":
        m = cavity_mesh(int(rng.integers(8, 12)), jitter=min(jitter, 0.3), seed=seed)
    elif kind == "tied":
        m = rp.tied_mesh(*(int(x) for x in rng.integers(4, 8, size=3)), bool(rng.integers(2)), seed)
    elif kind == "baffle":
        m = rp.baffle_mesh(jitter=jitter, seed=seed, split=bool(rng.integers(2)))
    else:
        m = rp.fan_mesh(int(rng.integers(4, 22)), seed=seed)
    lo = min(np.linalg.norm(m.points[a] - m.points[b]) for a, b in [(0, 1)]) if False else None
    text = f"-centroidalIters {int(rng.integers(2, 9))} -relTol 0"
    for name in ("edgeAngleConstraint", "faceAngleConstraint", "totalMinFreeze"):
        text += f" -{name} {'true' if rng.integers(2) else 'false'}"
    text += f" -minAngle {rng.choice([15, 35, 50])} -maxAngle {rng.choice([140, 160, 175])} -relStepFrac {rng.choice([0.3, 0.5, 0.9])}"
    if rng.random() < 0.5:
        names = [p.name for p in m.patches]
        pick = list(rng.choice(names, size=min(len(names), int(rng.integers(1, 4))), replace=False))
        if rng.random() < 0.3:
            pick.append('"x.*"')
        text += " -layerPatches '(" + " ".join(pick) + ")'"
        text += f" -layerMaxBlendingFraction {rng.choice([0.2, 0.3, 0.6])} -layerExpansionRatio {rng.choice([1.0, 1.2, 1.5])}"
        text += f" -minLayers {int(rng.integers(0, 3))} -maxLayers {int(rng.integers(3, 6))}"
    return m, text, str(rng.choice(["com", "org"])), (float(rng.choice([0.3, 0.5, 0.9])), float(rng.choice([0.1, 0.3, 0.6])))


@pytest.mark.parametrize("k", range(30))
def test_seeded_sweep(ref, oracle_lib, k):
    m, text, variant, (fe, fs) = _sweep_case(k)
    lo = oracle_lib.Oracle(m).mesh_stats()[0]
    text += f" -minEdgeLength {fe * lo!r} -maxStepLength {fs * fe * lo!r}"
    _pin(ref, oracle_lib, m, text, variant)


# ---- the log ---------------------------------------------------------------------------------------------------------------------
def test_fatal_error_is_returned(ref):
    """an error comes back as an exception with its text; the process goes on"""
    with pytest.raises(ref.ReferenceError_, match="Invalid option"):
        ref.run(_block(0.2, dims=(3, 3, 3)), ["-noSuchOption", "2"])
