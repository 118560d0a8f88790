"""Shared by test_reference_pin.py (oracle against the reference) and test_gpu_reference_pin.py (HIP against the reference):
turning a reference command line into the oracle's / the engine's configuration, and the comparison itself.

The option list is read HERE, by the test's own reading of the reference's documented options (its -help texts), not by
anything of the oracle or the engine: numeric options that are absent get what smoothmesh_amd.default_params and
LayerParams supply, and the comparison with the reference then shows whether those defaults are the reference's."""
import re
import shlex

import numpy as np

NUMERIC = {"minEdgeLength": float, "maxStepLength": float, "relStepFrac": float, "minAngle": float, "maxAngle": float}
BOOL = ("totalMinFreeze", "edgeAngleConstraint", "faceAngleConstraint")


def parse(argv):
    """['-minAngle', '15', ...] -> {'minAngle': '15', ...}"""
    argv = [str(a) for a in argv]
    assert len(argv) % 2 == 0 and all(a.startswith("-") for a in argv[::2]), argv
    return {a[1:]: b for a, b in zip(argv[::2], argv[1::2])}


def patch_words(text):
    """'(walls "baffle.*")' or 'walls' -> ('walls', '"baffle.*"'): the words as smoothmesh_amd.patch_arrays takes them"""
    t = text.strip()
    if t.startswith("("):
        assert t.endswith(")")
        t = t[1:-1]
    return tuple(re.findall(r'"[^"]*"|[^\s"()]+', t))


def configure(mesh, argv, meshMinEdgeLength):
    """-> (SmoothParams, LayerParams or None, layerEdgeLength, iterations, relTol)"""
    from smoothmesh_amd import LayerParams, default_params
    opt = parse(argv)
    over = {k: f(opt[k]) for k, f in NUMERIC.items() if k in opt}
    over.update({k: {"true": True, "false": False}[opt[k]] for k in BOOL if k in opt})
    prm = default_params(meshMinEdgeLength, **over)
    lay = None
    if "layerPatches" in opt:
        lay = LayerParams(layerPatches=patch_words(opt["layerPatches"]))
        for k, f in (("layerMaxBlendingFraction", float), ("layerExpansionRatio", float), ("minLayers", int), ("maxLayers", int)):
            if k in opt:
                setattr(lay, k, f(opt[k]))
    layerEdgeLength = float(opt.get("layerEdgeLength", prm.minEdgeLength))
    return prm, lay, layerEdgeLength, int(opt.get("centroidalIters", 1000)), float(opt.get("relTol", 0.02))


def oracle_for(oracle_lib, mesh, argv, variant="com"):
    """an Oracle configured as the command line says; -> (oracle, iterations, relTol, layers enabled)"""
    from smoothmesh_amd import patch_arrays
    o = oracle_lib.Oracle(mesh)
    o.set_foam_variant(variant)
    prm, lay, layerEdgeLength, iters, relTol = configure(mesh, argv, o.mesh_stats()[0])
    o.set_params(prm)
    on = False
    if lay is not None:
        st, sz, kd, sel = patch_arrays(mesh, lay.layerPatches)
        on = o.setup_layers(st, sz, kd, sel, lay.layerMaxBlendingFraction, layerEdgeLength, lay.layerExpansionRatio, lay.minLayers, lay.maxLayers)
    return o, iters, relTol, on


def oracle_series(oracle_lib, mesh, argv, variant="com"):
    """the oracle, one iteration at a time: (points per iteration, nFrozenPoints, residuals as floats, layers enabled)"""
    o, iters, relTol, on = oracle_for(oracle_lib, mesh, argv, variant)
    pts, frz, res = [], [], []
    for _ in range(iters):
        n, r, f = o.iterate(1, relTol)
        assert n == 1
        pts.append(o.points().copy()); frz.append(int(f[0])); res.append(float(r[0]))
        if r[0] < relTol:
            break
    return pts, np.array(frz, np.int64), res, on


def printed(x):
    """a double as the reference's Info stream prints it: six significant digits, general format"""
    return "%g" % x


def first_difference(a, b):
    d = np.flatnonzero((np.asarray(a) != np.asarray(b)).any(axis=1))
    return None if len(d) == 0 else (int(d[0]), np.asarray(a)[d[0]].tolist(), np.asarray(b)[d[0]].tolist(), len(d))


def assert_same_run(ref, pts, frz, res, what=""):
    """bit-equal points at every iteration, equal nFrozenPoints series, residuals equal as the reference prints them"""
    assert len(ref.points) == len(pts), (what, "iterations", len(ref.points), len(pts))
    assert ref.nFrozenPoints.tolist() == list(frz), (what, "nFrozenPoints", ref.nFrozenPoints.tolist(), list(frz))
    for i, (a, b) in enumerate(zip(pts, ref.points)):
        assert np.array_equal(a, b), (what, "points differ after iteration", i + 1, first_difference(a, b))
    assert ref.residuals == [printed(r) for r in res], (what, "residuals", ref.residuals, [printed(r) for r in res])


def args(text):
    return shlex.split(text)


# ---- meshes ---------------------------------------------------------------------------------------------------------
def fan_mesh(nSpokes, nLayers=3, jitter=0.05, seed=1):
    """prisms around an axis: the axis points have valence nSpokes + 2"""
    from smoothmesh_amd.meshgen import extrude_surface
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, nSpokes, endpoint=False)
    ring1 = np.stack([np.cos(ang), np.zeros(nSpokes), np.sin(ang)], axis=1)
    ring2 = 2.0 * np.stack([np.cos(ang + 0.1), np.zeros(nSpokes), np.sin(ang + 0.1)], axis=1)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], ring1, ring2])
    verts[1:1 + nSpokes] += jitter * rng.standard_normal((nSpokes, 3)) * [1, 0, 1]
    faces = []
    for i in range(nSpokes):
        j = (i + 1) % nSpokes
        faces.append([0, 1 + i, 1 + j])
        faces.append([1 + i, 1 + nSpokes + i, 1 + nSpokes + j, 1 + j])
    return extrude_surface(verts, faces, nLayers=nLayers, thickness=1.0, direction=(0, 1, 0))


def baffle_mesh(dims=(8, 7, 6), jitter=0.3, seed=4, split=False):
    """a wall inside a jittered block (createBaffles), optionally split into twins (splitBaffles)"""
    from smoothmesh_amd.meshgen import add_baffle, baffle_in_plane, hex_block, split_baffles
    m = add_baffle(hex_block(*dims, jitter=jitter, seed=seed), baffle_in_plane(hex_block(*dims), 0, 4.0 / dims[0], lambda c: c[:, 1] < 0.7))
    return split_baffles(m) if split else m


def tied_mesh(nx, ny, nz, graded, seed):
    """points on binary fractions (scripts/fuzz_parity.py, kind "tied"): spacing 2^-4 (x 2^-5 if graded), a tenth of the interior
    points moved by multiples of 2^-10 -- equal lengths stay bit-equal, so sortedOrder and the closest-point choice see exact ties"""
    from smoothmesh_amd.meshgen import hex_block
    rng = np.random.default_rng(seed)
    if graded:
        nx *= 2
    m = hex_block(nx, ny, nz, lengths=(nx / (32.0 if graded else 16.0), ny / 16.0, nz / 16.0), jitter=0.0)
    P = m.points.reshape(-1, 3)
    inner = np.flatnonzero(m.find_internal_points())
    mv = rng.choice(inner, size=max(1, len(inner) // 10), replace=False)
    P[mv] += rng.integers(-6, 7, size=(len(mv), 3)) / 1024.0
    return m


def one_patch(mesh, name, ptype="wall"):
    from smoothmesh_amd.mesh import Patch
    first = min(p.startFace for p in mesh.patches)
    mesh.patches = [Patch(name, ptype, sum(p.nFaces for p in mesh.patches), first)]
    return mesh
