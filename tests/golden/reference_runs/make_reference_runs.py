"""Writes tests/golden/reference_runs/*.npz: a handful of runs of THE REFERENCE ITSELF (oracle/_ref/libsmref.so, the reference's
own source on the stand-in OpenFOAM of oracle/foam_shim/), recorded as data -- the mesh and the option list that went in, the
points after every iteration, nFrozenPoints and the residuals as printed that came out.  tests/test_reference_runs_golden.py
holds the ORACLE to them where the reference is not present.  Run from the repository root after __graft_entry__.build():
    python tests/golden/reference_runs/make_reference_runs.py
The addressing and the geometry that the stand-in mesh used are the oracle's (they are inputs of the stand-in), so a change of
the oracle's addressing order or geometry formulas needs these files written again."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cases():
    import ref_pin_cases as rp
    from smoothmesh_amd.meshgen import hex_block
    from smoothmesh_amd.polymesh import cavity_mesh
    return [
        ("block_constraints", hex_block(6, 5, 4, jitter=0.45, seed=3), "-centroidalIters 8 -relTol 0 -minAngle 50 -maxAngle 140", "com"),
        ("block_defaults", hex_block(6, 5, 5, jitter=0.4, seed=11), "", "com"),
        ("block_layers", hex_block(6, 5, 4, jitter=0.3, seed=8),
         "-centroidalIters 8 -relTol 0 -layerPatches '(\"x.*\" zmin)' -minLayers 0 -maxLayers 3 -layerMaxBlendingFraction 0.6 -layerExpansionRatio 1.2 "
         "-layerEdgeLength 0.05", "com"),
        ("cavity_layers_org", cavity_mesh(6, jitter=0.3, seed=2), "-centroidalIters 3 -relTol 0 -layerPatches cavity -maxLayers 3", "org"),
        ("fan_total_freeze", rp.fan_mesh(9), "-centroidalIters 8 -relTol 0 -minEdgeLength 0.3 -totalMinFreeze true -faceAngleConstraint false", "com"),
        ("tied_block", rp.tied_mesh(5, 6, 4, True, 3), "-centroidalIters 6 -relTol 0", "com"),
    ]


def main():
    import ref_pin_cases as rp
    from oracle import ref_ffi
    for name, m, text, variant in cases():
        r = ref_ffi.run(m, rp.args(text), variant)
        np.savez_compressed(
            os.path.join(HERE, name + ".npz"), options=text, variant=variant, points=m.points, faceOffsets=m.faceOffsets, facePoints=m.facePoints,
            owner=m.owner, neighbour=m.neighbour, nCells=m.nCells, patchName=np.array([p.name for p in m.patches]),
            patchType=np.array([p.type for p in m.patches]), patchStart=np.array([p.startFace for p in m.patches], np.int32),
            patchSize=np.array([p.nFaces for p in m.patches], np.int32), ref_points=np.stack(r.points), ref_nFrozenPoints=r.nFrozenPoints,
            ref_residuals=np.array(r.residuals))
        print(name, len(r.points), "iterations,", os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
