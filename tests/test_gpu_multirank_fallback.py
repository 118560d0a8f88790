"""The multi-rank (halo) path off its default kernels, on ONE GPU (LocalMultiSmoother, as tests/test_gpu_multirank.py): every rank
on the direct-gather kernels (SMGPU_TILES=0, or a tile builder that refuses the mesh), one rank of a world falling back alone, and
the per-point pack kernel beside the tiled kernels (SMGPU_PACK_TILES=0).  These are the `!useTiles` / `!packTiles` branches of
smgpu_iter_begin / mid / end: k_halo_packA + k_halo_packL in place of k_pack_tile, runProposalAndConstraints behind the combine
kernels, k_halo_orF + k_apply in place of k_shared_fix, the point-block partials of the residual reduction, and the refusal of the
peer-store transport.  Expected = the oracle's MultiDomain at the project's tolerances, and the default-knob GPU run of the same
case bit for bit.  Every case reads the launch counters, so that a silent return to the tiled path cannot pass as a pass."""
import os

import numpy as np
import pytest

from test_gpu_multirank import _check_against_multi_oracle, _hex_case, _poly_case

pytestmark = pytest.mark.gpu

_DEFAULT = {}      # default-knob GPU runs, once per case


def _launches(eng):
    return {c["name"]: c["launches"] for c in eng.counters()}


def _is_direct(eng):
    c = _launches(eng)
    return c["k_face_geom"] > 0 and c["k_geom_tile"] == 0


def _is_tiled(eng):
    c = _launches(eng)
    return c["k_geom_tile"] > 0 and c["k_face_geom"] == 0


def _run(subs, prm, iters, overlap, env, monkeypatch, set_up=None, engine_factory=None):
    """one LocalMultiSmoother created and run under `env` -> results, per-rank launch counters' verdicts and the halo mode"""
    from smoothmesh_amd.halo import LocalMultiSmoother
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        ms = LocalMultiSmoother(subs, device=0, overlap=overlap, engine_factory=engine_factory)
        if set_up is None:
            ms.set_params(prm)
        else:
            set_up(ms)
        for st in ms.states:
            st.eng.enable_timing(True)
        run = ms.iterate(iters, 0.0)
        r = dict(run=run, pts=ms.get_points(), direct=[_is_direct(st.eng) for st in ms.states], tiled=[_is_tiled(st.eng) for st in ms.states],
                 mode=ms.states[0].eng.debug_halo_mode())
        for st in ms.states:
            st.eng.close()
    return r


def _default(key, subs, prm, iters, overlap, monkeypatch, set_up=None):
    if key not in _DEFAULT:
        r = _run(subs, prm, iters, overlap, {}, monkeypatch, set_up)
        assert not any(r["direct"]), r["direct"]      # the default is the tiled path
        _DEFAULT[key] = r
    return _DEFAULT[key]


def _same_bits(a, b):
    assert a["run"][0] == b["run"][0] and np.array_equal(a["run"][1], b["run"][1]) and np.array_equal(a["run"][2], b["run"][2])
    for p, q in zip(a["pts"], b["pts"]):
        assert np.array_equal(p, q)


# ---- 1a: every rank on the direct-gather kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("constraints,overlap", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_hex_world_of_eight_on_direct_gather_kernels(oracle_lib, monkeypatch, constraints, overlap):
    """SMGPU_TILES=0 with a halo: face, edge and corner sharers (2 x 2 x 2), k_halo_packA, the combine kernels in front of
    runProposalAndConstraints, k_halo_orF + k_apply, in order and with an exchange stream"""
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 2), (5, 4, 4), constraints)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, bool(overlap), {"SMGPU_TILES": "0"}, monkeypatch)
    assert all(r["direct"]), r["direct"]
    assert not r["mode"]["multi_role"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("hex8", constraints, overlap), subs, prm, 8, bool(overlap), monkeypatch))


def test_polyhedral_world_of_four_on_direct_gather_kernels(oracle_lib, monkeypatch):
    """the castellated cavity mesh cut 2 x 2 x 1 (hanging-node faces on processor patches, points with four sharers), constraints on"""
    subs, orcs, prm, table, mo = _poly_case(oracle_lib, 12, (2, 2, 1), True)
    oracle_run = mo.iterate(7, 0.0)
    r = _run(subs, prm, 7, False, {"SMGPU_TILES": "0"}, monkeypatch)
    assert all(r["direct"]), r["direct"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    assert r["run"][2][-1] > sum(int((~s.mesh.find_internal_points().astype(bool)).sum()) for s in subs)   # the constraints did freeze points
    _same_bits(r, _default(("poly4",), subs, prm, 7, False, monkeypatch))


def _layers_case(oracle_lib):
    from test_gpu_layers import _layers_parallel_case, _set_layers_and_check_setup
    subs, orcs, prm, mo, lp, fields = _layers_parallel_case(oracle_lib, (2, 2, 1), ["xmin", "zmax"], False, (5, 4, 4))
    return subs, orcs, prm, mo, (lambda ms: _set_layers_and_check_setup(ms, fields, prm, lp))


def test_layers_on_direct_gather_kernels(oracle_lib, monkeypatch):
    """exchange L beside exchange A behind the non-tiled kernels: k_halo_packL, k_halo_combineAL / k_halo_combineL"""
    subs, orcs, prm, mo, set_up = _layers_case(oracle_lib)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, True, {"SMGPU_TILES": "0"}, monkeypatch, set_up)
    assert all(r["direct"]), r["direct"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("layers4",), subs, prm, 8, True, monkeypatch, set_up))


def test_boundary_smoothing_with_layers_on_direct_gather_kernels(oracle_lib, monkeypatch):
    """decomposed boundary point smoothing with layers (the 14-double L records, k_bnd_normals_shared) behind the non-tiled kernels"""
    from test_gpu_boundary import _decomposed_boundary_case
    mo, orcs, subs, prm, set_up = _decomposed_boundary_case(oracle_lib, (2, 2, 2), False, True)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, True, {"SMGPU_TILES": "0"}, monkeypatch, set_up)
    assert all(r["direct"]), r["direct"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("boundary8",), subs, prm, 8, True, monkeypatch, set_up))


# ---- 1b: a tile builder refuses the sub-domains ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,what", [("SMGPU_GEOM_CAPP", "gp"), ("SMGPU_SMOOTH_CAPC", "sc")])
def test_automatic_fallback_under_a_halo(oracle_lib, monkeypatch, key, what):
    """a hard cap one below the largest element of the sub-domains (tests/test_gpu_tile_shapes.py): the builder refuses, smgpu_create
    turns the tiles off by itself, and the halo is configured on an engine that did not ask for the direct-gather kernels"""
    from test_gpu_tile_shapes import _needs
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 2), (5, 4, 4), True)
    need = max(_needs(s.mesh)[what] for s in subs)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, False, {key: need - 1}, monkeypatch)
    assert all(r["direct"]), (key, need, r["direct"])
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("hex8", True, 0), subs, prm, 8, False, monkeypatch))


# ---- 1c: one rank falls back alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_one_rank_of_a_world_on_direct_gather_kernels(oracle_lib, monkeypatch, grid, constraints):
    """a rank whose sub-domain a tile builder refuses falls back alone while its peers stay tiled: the records the per-point
    pack kernel sends meet those of k_pack_tile in the peers' combines, and the other way round"""
    import torch
    from smoothmesh_amd import SmoothEngine
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, grid, (5, 4, 4), constraints)
    made = []

    def factory(mesh):
        cur = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
        before = os.environ.get("SMGPU_TILES")
        if len(made) == 1:
            os.environ["SMGPU_TILES"] = "0"
        try:
            made.append(SmoothEngine(mesh, device=0, stream=cur))
        finally:
            if before is None:
                os.environ.pop("SMGPU_TILES", None)
            else:
                os.environ["SMGPU_TILES"] = before
        return made[-1]

    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, False, {}, monkeypatch, engine_factory=factory)
    assert r["direct"] == [i == 1 for i in range(len(subs))], r["direct"]
    assert r["tiled"] == [i != 1 for i in range(len(subs))], r["tiled"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("hex8" if grid == (2, 2, 2) else "hex2", constraints, 0), subs, prm, 8, False, monkeypatch))


# ---- 1d: the per-point pack kernel beside the tiled kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 1])
def test_per_point_pack_kernel_with_tiles_on(oracle_lib, monkeypatch, overlap):
    """SMGPU_PACK_TILES=0: exchange A through k_halo_packA while geometry and smoothing stay tiled, and no multi-role launches
    (debug_halo_mode is the evidence that the knob was read: the default in-order run of this case takes them)"""
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 1), (16, 12, 12), False)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, bool(overlap), {"SMGPU_PACK_TILES": "0"}, monkeypatch)
    assert all(r["tiled"]), r["tiled"]
    assert not r["mode"]["multi_role"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    base = _default(("hex4big", overlap), subs, prm, 8, bool(overlap), monkeypatch)
    if not overlap:
        assert base["mode"]["multi_role"]
    _same_bits(r, base)


def test_per_point_pack_kernel_with_layers(oracle_lib, monkeypatch):
    """SMGPU_PACK_TILES=0 with the layer treatment: k_halo_packA + k_halo_packL in front of the tiled smoothing"""
    subs, orcs, prm, mo, set_up = _layers_case(oracle_lib)
    oracle_run = mo.iterate(8, 0.0)
    r = _run(subs, prm, 8, True, {"SMGPU_PACK_TILES": "0"}, monkeypatch, set_up)
    assert not any(r["direct"]) and not r["mode"]["multi_role"]
    _check_against_multi_oracle(subs, orcs, oracle_run, r["run"], r["pts"])
    _same_bits(r, _default(("layers4",), subs, prm, 8, True, monkeypatch, set_up))


# ---- the shared points' own tiles, their tables built on either side ---------------------------------------------------------------------
@pytest.mark.parametrize("constraints", [False, True])
@pytest.mark.parametrize("knob,where", [("1", "device"), ("0", "host"), ("2", "host")])
def test_shared_point_tiles_on_the_device_and_on_the_host(oracle_lib, monkeypatch, capfd, knob, where, constraints):
    """SMGPU_DEVICE_TILES=0 / 2: the tables of the tiles over the shared points (smgpu_halo_configure) come from the host's builder and
    are uploaded, instead of being adopted from the device build -- same coordinates, bit for bit; the SMGPU_VERBOSE=2 line of every
    rank says where they were built, so that a silent return to the other side cannot pass"""
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 2, 2), (5, 4, 4), constraints)
    base = _default(("hex8", constraints, 0), subs, prm, 8, False, monkeypatch)
    capfd.readouterr()
    r = _run(subs, prm, 8, False, {"SMGPU_DEVICE_TILES": knob, "SMGPU_VERBOSE": "2"}, monkeypatch)
    said = [line for line in capfd.readouterr().err.splitlines() if "shared-point tiles:" in line and "tables on the" in line]
    assert len(said) == len(subs) and all(line.endswith("tiles, tables on the " + where) for line in said), (knob, said)
    assert all(r["tiled"]), r["tiled"]
    _same_bits(r, base)


# ---- 1e: the peer-store transport refuses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SMGPU_TILES": "0"}, {"SMGPU_PACK_TILES": "0"}])
def test_peer_store_transport_refuses_without_the_tiled_pack_kernel(oracle_lib, monkeypatch, env):
    """smgpu_halo_set_push on an engine with shared points: the peer stores are k_pack_tile's, so without it the call fails with
    its own text instead of running; with the default knobs the same description (the engine's own receive slots standing in
    for the peers', as scripts/check_arrangements.py does) is accepted -- nothing is launched either way"""
    from smoothmesh_amd import SmgpuError
    from smoothmesh_amd.halo import LocalMultiSmoother, PushBuffers
    subs, orcs, prm, table, mo = _hex_case(oracle_lib, (2, 1, 1), (5, 4, 4), False)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ms = LocalMultiSmoother(subs, device=0, overlap=False)
        ms.set_params(prm)
        st = ms.states[0]
        assert st.t.nSend > 0
        pb = PushBuffers(0, st.t.nRecv)
        try:
            peers = [o for o in range(len(st.t.counts)) if st.t.counts[o] > 0]
            cnt = [int(st.t.counts[o]) for o in peers]
            base = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
            args = (cnt, base, list(range(len(peers))), [pb.ptr["recvA"]] * len(peers), [pb.ptr["recvL"]] * len(peers),
                    [pb.ptr["recvF"]] * len(peers), [pb.ptr["flags"]] * len(peers), pb.ptr["flags"])
            if env:
                with pytest.raises(SmgpuError, match="needs the tiled pack kernel"):
                    st.eng.set_push(*args)
            else:
                st.eng.set_push(*args)
                st.eng.clear_push()
        finally:
            for s in ms.states:
                s.eng.close()
            pb.close()
