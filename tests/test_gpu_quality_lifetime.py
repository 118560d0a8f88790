"""Lifetimes of the mesh-quality features' state (include/smgpu.h smgpu_set_quality_trace / smgpu_set_quality_guard /
smgpu_set_tangle_constraint, the three reports and their coupled forms; DESIGN.md "Mesh quality" 10): a feature that was on, used
and switched off, then switched on and used again, is a fresh engine's feature from the same points, in every order of enabling;
record slabs that grow and are reused between calls give the records of one call; and an engine destroyed with every feature's
memory live leaves a second engine in the same process the same results.  The arithmetic is the neighbouring tests'."""
import dataclasses
import functools
import itertools
import struct

import numpy as np
import pytest

from test_gpu_quality_guard import TANGLE, dented_block_tiles
from test_gpu_quality_trace import _engine
from test_gpu_tangle import dented_cavity

pytestmark = pytest.mark.gpu

# name -> (mesh, engine settings): the loop with the reference's constraints on a mesh no feature fires on; two meshes that
# unconstrained smoothing tangles (the guard trips, the tangle constraint reverts)
MESHES = {
    "hex12": (lambda: _hex_block(12, 9, 7, jitter=0.3), {}),
    "dented_tiles": (dented_block_tiles, TANGLE),
    "cavity_band": (lambda: dented_cavity((0.5, 0.5), (0.1875, 0.2, 0.2125, 0.225)), dict(constraints=False, maxStepLength=0.05, minEdgeLength=1e-4)),
}
# the guard judges the trace's records: the trace comes before it
ORDERS = [o for o in itertools.permutations(("trace", "guard", "tangle")) if o.index("trace") < o.index("guard")] + [("trace", "guard")]
INTERVAL = 2


def _hex_block(*a, **k):
    from smoothmesh_amd.meshgen import hex_block
    return hex_block(*a, **k)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name][0]()


def _new(name):
    return _engine(_mesh(name), **MESHES[name][1])


def _key(v):
    """a value with every float and array replaced by its bytes: equality of keys is equality bit for bit"""
    if dataclasses.is_dataclass(v):
        return (type(v).__name__,) + tuple((f.name, _key(getattr(v, f.name))) for f in dataclasses.fields(v))
    if isinstance(v, dict):
        return tuple((k, _key(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return tuple(_key(x) for x in v)
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (float, np.floating)):
        return struct.pack("<d", float(v))
    return v


def _switch_on(e, order):
    for what in order:
        if what == "trace":
            e.set_quality_trace(INTERVAL)
        elif what == "guard":
            e.set_quality_guard()
        else:
            e.set_tangle_constraint()


def _switch_off(e):
    e.set_quality_guard(None)
    e.clear_tangle_constraint()
    e.set_quality_trace(0)


def _use(e, calls):
    """iterate(n) for n in calls -> everything the features and the loop show of it"""
    out = []
    for n in calls:
        done, res, frz = e.iterate(n, 0.0)
        out.append((done, res, frz, e.last_near_ties))
    return _key(dict(calls=out, trace=e.quality_trace(), tangle=e.tangle_records(), tangleState=e.tangle_state(), guard=e.quality_guard(),
                     points=e.get_points()))


# ---- 1. on, used, off, on again, used ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids="-".join)
@pytest.mark.parametrize("name", ["hex12", "dented_tiles"])
def test_on_used_off_on_again_used(name, order):
    e = _new(name)
    _switch_on(e, order)
    assert e.iterate(10, 0.0)[0] >= 1                          # (a guard that trips returns fewer, and rolls back)
    g = e.quality_guard()
    if name == "dented_tiles":                                 # the case tests something: a trip with its rollback, or reverted points
        assert g.tripped if "tangle" not in order else any(r.nBadCells > 0 for r in e.tangle_records())
    _switch_off(e)
    assert not e.quality_guard().armed and not e.tangle_state().on and e.tangle_records() == [] and e.quality_trace() == []
    pts = e.get_points()
    assert not np.array_equal(pts, _mesh(name).points)
    _switch_on(e, order)
    again = _use(e, (3, 8))
    fresh = _new(name)
    fresh.set_points(pts)
    _switch_on(fresh, order)
    assert again == _use(fresh, (3, 8))


# ---- 2. slab growth and reuse ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dented_tiles", "cavity_band"])
def test_slab_growth_and_reuse(name):
    def run(calls):
        e = _new(name)
        e.set_quality_trace(1)
        e.set_tangle_constraint()
        stats = [e.iterate(n, 0.0) for n in calls]
        assert [s[0] for s in stats] == list(calls)
        return (np.concatenate([s[1] for s in stats]), np.concatenate([s[2] for s in stats]), e.quality_trace(), e.tangle_records(),
                e.tangle_state(), e.get_points())

    a, b = run((2, 9, 3)), run((14,))
    assert [r.iteration for r in a[2]] == list(range(1, 15)) and [r.iteration for r in a[3]] == list(range(1, 15))
    assert a[4].iteration == 14
    assert any(r.nBadCells > 0 for r in a[3]), "the mesh does not tangle: the case tests nothing"
    assert _key(a) == _key(b)


# ---- 3. all three report kinds, then destroy ---------------------------------------------------------------------------
def _everything():
    """every quality feature's device memory brought to life on one serial engine and on the two engines of a split, then all
    three engines closed with it live -> what they answered"""
    import torch
    from smoothmesh_amd import SmoothEngine
    from smoothmesh_amd import quality as Q
    from smoothmesh_amd.decompose import decompose, grid_partition
    m = _mesh("hex12")
    e = _new("hex12")
    out = dict(quality=e.mesh_quality(), geometry=e.mesh_quality_geometry(), motion=e.mesh_quality_motion(),
               fields=[e.quality_field("cellVolume"), e.quality_field("faceSkewness"), e.quality_geometry_field("faceWeight"),
                       e.quality_geometry_field("cellDeterminant"), e.quality_motion_field("faceTwist")],
               sets=[e.quality_sets(skewThreshold=0.3), e.quality_geometry_sets(weightThreshold=0.45), e.quality_motion_sets(twistThreshold=0.95)])
    assert sum(len(v) for s in out["sets"] for v in s.values()) > 0
    _switch_on(e, ("trace", "guard", "tangle"))
    out["loop"] = e.iterate(5, 0.0)                            # the records stay unread: pending at the destroy
    out["after"] = (e.mesh_quality(), e.mesh_quality_geometry(), e.mesh_quality_motion())
    subs = decompose(m, grid_partition(m, (2, 1, 1)), 2)
    assert sum(p.nFaces for p in subs[0].mesh.patches if p.type == "processor") > 0
    engines = [SmoothEngine(s.mesh) for s in subs]
    dev = torch.device("cuda", 0)
    out["coupled"] = [Q.local_quality(engines, subs, dev, {}), Q.local_quality_geometry(engines, subs, dev, {}),
                      Q.local_quality_motion(engines, subs, dev, {}),
                      Q.local_quality_field(engines, "faceNonOrthogonality", dev), Q.local_quality_geometry_field(engines, "faceVolumeRatio", dev),
                      Q.local_quality_motion_field(engines, "faceTetQuality", dev),
                      Q.local_quality_sets(engines, dev, dict(skewThreshold=0.3)), Q.local_quality_geometry_sets(engines, dev, dict(weightThreshold=0.45)),
                      Q.local_quality_motion_sets(engines, dev, dict(twistThreshold=0.95))]
    for x in [e] + engines:
        x.close()
    return _key(out)


def test_all_report_kinds_then_destroy_then_again():
    first = _everything()
    assert first == _everything()
