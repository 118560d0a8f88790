"""The graded blocks A and B of tests/quality_fold_reference.py, checked on the numpy references alone (no GPU): the ties and exact
values that tests/test_gpu_quality_reductions.py places under the engine's reductions are really there.  Plane positions are binary
fractions, so every measure is a function of exact coordinate differences and cells / faces of one shape carry the same bits.

Measured record (reference, both variants; the tests below print it again):
    A: minVolume 2^-15 on 4 cells, workgroups 0-1, lowest 749; maxAspectRatio 6 on 31 cells, workgroups 0-1, lowest 178; minFaceWeight
       0.25 and minVolRatio 1/3 on 216 faces each, workgroups 0-3, lowest 27; minTetQuality on 8 faces, workgroups 0, 1, 3, 4, lowest
       1357; minDeterminant on 10 cells, lowest 5
    B: minVolume on 2 cells, workgroup 1, lowest 2477; maxAspectRatio on 20 cells; weight and ratio as A; minTetQuality on 4 faces,
       workgroups 3-4, lowest 6325; minDeterminant on 6 cells, lowest 5"""
import functools

import numpy as np
import pytest

from quality_fold_reference import block_a, block_b, groups_of, internal_faces, tied
from test_quality_geometry_reference import geometry_reference_of
from test_quality_motion_reference import motion_reference_of
from test_quality_reference import reference_of

H = 2.0 ** -5
BLOCKS = {"A": block_a, "B": block_b}


@functools.lru_cache(maxsize=None)
def graded_case(name, variant):
    """(mesh, {kind: (reference report, reference fields)}), computed once and left unchanged"""
    from oracle import oracle_ffi
    oracle_ffi.build()
    m = BLOCKS[name]()
    out = {"quality": reference_of(oracle_ffi, m, variant), "geometry": geometry_reference_of(oracle_ffi, m, variant),
           "motion": motion_reference_of(oracle_ffi, m, variant)}
    for _, f in out.values():
        for v in f.values():
            v.setflags(write=False)
    return m, out


def test_shape_of_the_blocks():
    for name in BLOCKS:
        m = BLOCKS[name]()
        assert (m.nCells, m.nFaces, m.nInternalFaces) == (2592, 8388, 7164)          # 1 full + 1 ragged cell workgroup, 4 + 1 of faces
        assert np.array_equal(np.rint(m.points / H) * H, m.points)
        assert m.points.max(axis=0).tolist() == [H * 50, H * 25, H * (16 if name == "A" else 17)]


@pytest.mark.parametrize("variant", ["com", "org"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ties_and_exact_values(name, variant):
    m, ref = graded_case(name, variant)
    (rep, f), (grep, gf), (mrep, mf) = ref["quality"], ref["geometry"], ref["motion"]
    inner = internal_faces(m)
    rows = {"minVolume": (f["cellVolume"], None, "min"), "maxAspectRatio": (f["cellAspectRatio"], None, "max"),
            "minFaceWeight": (gf["faceWeight"], inner, "min"), "minVolRatio": (gf["faceVolumeRatio"], inner, "min"),
            "minTetQuality": (mf["faceTetQuality"], None, "min"), "minDeterminant": (gf["cellDeterminant"], None, "min")}
    t = {}
    for k, (x, dom, kind) in rows.items():
        t[k] = tied(x, dom, kind)
        print(f"    block {name} {variant} {k}: {x[t[k][0]]!r} tied on {t[k].size}, workgroups {groups_of(t[k])}, lowest id {int(t[k][0])}")
        assert t[k].size > 1, k                                                  # the extreme is tied
    # the tie spans the stated workgroups
    assert groups_of(t["minVolume"]) == ([0, 1] if name == "A" else [1])
    if name == "A":
        assert groups_of(t["maxAspectRatio"]) == [0, 1]
    assert groups_of(t["minFaceWeight"]) == [0, 1, 2, 3] and groups_of(t["minVolRatio"]) == [0, 1, 2, 3]
    assert groups_of(t["minTetQuality"]) == ([0, 1, 3, 4] if name == "A" else [3, 4])
    # the lowest tied id is not element 0: a reduction that kept its first element would be wrong
    for k in ("minVolume", "maxAspectRatio", "minFaceWeight", "minVolRatio", "minTetQuality"):
        assert t[k][0] != 0, k
    # the references report the lowest tied id
    assert rep["minVolumeCell"] == t["minVolume"][0] and grep["minFaceWeightFace"] == t["minFaceWeight"][0]
    assert grep["minVolRatioFace"] == t["minVolRatio"][0] and grep["minDeterminantCell"] == t["minDeterminant"][0]
    assert mrep["minTetFace"] == t["minTetQuality"][0]
    # exact values
    assert rep["minVolume"] == 2.0 ** -15 and rep["maxAspectRatio"] == 6.0
    assert grep["minFaceWeight"] == 0.25 and grep["minVolRatio"] == 1.0 / 3.0
    assert np.all(f["faceNonOrthogonality"] == 0.0) and np.all(f["faceSkewness"] == 0.0)
    assert np.all(gf["faceConcavity"] == 0.0) and np.all(f["cellOpenness"] == 0.0)
    assert np.all(gf["faceFlatness"] == 1.0) and np.all(mf["faceTwist"] == 1.0) and np.all(mf["faceTriangleTwist"] == 1.0)
    X, Y, Z = m.points.max(axis=0)
    assert rep["totalVolume"] == X * Y * Z and float(np.sum(f["cellVolume"][::-1])) == X * Y * Z
