#!/usr/bin/env python3
"""bench.py -- headline benchmark: mesh points smoothed per second over the smoothing iteration loop
(src/smoothMesh.C:2257-2437) on MI355X, plus achieved bandwidth vs the HBM roofline.

A "step" is one smoothing iteration over the whole (per-rank) mesh.  Default workload = BASELINE.json
configs[1]: 1M-cell uniform hex block (100^3, interior jitter 0.2 h, seed 12345), constraints off,
relTol 0 (exactly K iterations run).  Inputs are device-resident when the timed region starts.

  python bench.py --gpus N --steps K --warmup W [--workload hex100|hex100c|hexN[c]] [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: set-up, the W + K steps timed cold (ms_per_step_cold), the clock
pre-run, the W warm-up and K timed steps (the reported value), --dump-outputs, and the result line.  Everything below
that takes runs of its own -- the configs[] sub-runs, parity_check, cpu_baseline, the per-kernel hipEvent pass
(roofline, kernels, chains), the 100-step at_100_iters leg, on N > 1 halo_cost -- is measured with --full only.

N > 1, one rank per GPU (started by torch.distributed.run, or by this script itself when WORLD_SIZE is unset): weak
scaling -- hexN: every rank owns an N^3 sub-block of a (Px*N, Py*N, Pz*N) block; cavityN: the castellated polyhedral
cavity mesh on a round(N * world^(1/3))^3 base grid cut into Px x Py x Pz boxes (BASELINE configs[4]: cavity215 on 8
GPUs = the 430^3-base, ~80 M-cell mesh), every rank generating ITS box only (polymesh.cavity_subdomain).  Shared-point
values are exchanged per iteration with RCCL all_to_all (smoothmesh_amd/halo.py); value = all ranks' points * K /
max-over-ranks time.

With --full the default N = 1 run also measures BASELINE.json's other single-GPU configurations (configs[2] hex100c, configs[3]
cavity215c and its constraints-off twin) with BASELINE's iteration counts (100 / 200) and reports them under "configs" in the
same JSON line (--no-configs skips that, --configs a,b,c selects).  With --full the headline and every configs[] entry carry
  ms_per_step_cold  the same W + K steps timed before the clock pre-run,
  parity_check      the engine against the CPU oracle on THIS workload's own mesh (same start, same n iterations),
  cpu_baseline      the serial oracle's rate on that mesh (bounded number of iterations),
none of which touches a timed region (--no-parity skips the oracle legs of the sub-runs: the 10 M-cell oracle costs a few
minutes of host time).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_VALU_PEAK_TOPS = 256 * 64 * 2.4e9 / 1e12   # FP64 vector instructions per second (x2 = 78.6 TFLOP/s with FMA)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level table); ~6290 achievable


def workload_layers(w):
    """trailing L = boundary layer treatment on (hex: all six sides, cavity: the cavity wall), one GPU only"""
    return w.rstrip("B").endswith("L")


def workload_boundary(w):
    """trailing B = boundary point smoothing on (hex: every side onto the block's own surface + its twelve feature
    edges; cavity: the cavity wall onto the sphere it was carved from)"""
    return w.endswith("B")


def boundary_params(kind, n, hi=(1.0, 1.0, 1.0)):
    from smoothmesh_amd import BoundaryParams
    from smoothmesh_amd.surfgen import box_feature_edges, box_surface, sphere_surface
    if kind == "hex":
        return BoundaryParams(initEdges=box_feature_edges(n, hi=hi), targetSurfaces=box_surface(max(n // 2, 1), hi=hi))
    return BoundaryParams(initEdges=box_feature_edges(n), targetSurfaces=sphere_surface(levels=6), smoothingPatches=("cavity",))


def parse_workload(w):
    """hexN[c][L] = N^3 hex block; cavityN[c][L] = castellated polyhedral cube-with-sphere-cavity on an N^3 base
    grid; c = edgeAngle + faceAngle constraints on; L = boundary layer treatment on (see workload_layers)."""
    w = w.rstrip("B")
    if w.endswith("L"):
        w = w[:-1]
    constraints = w.endswith("c")
    base = w[:-1] if constraints else w
    for kind in ("hex", "cavity"):
        if base.startswith(kind):
            return kind, int(base[len(kind):]), constraints
    raise SystemExit(f"unknown workload {w}")


def make_mesh(kind, n):
    if kind == "hex":
        from smoothmesh_amd.meshgen import hex_block
        return hex_block(n, jitter=0.2, seed=12345)
    from smoothmesh_amd.polymesh import cavity_mesh
    return cavity_mesh(n, jitter=0.2, seed=12345)


def proc_grid(n):
    return {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1), 8: (2, 2, 2)}.get(n) or (n, 1, 1)


def layer_params(kind):
    from smoothmesh_amd import LayerParams
    return LayerParams(layerPatches=('".*"',) if kind == "hex" else ("cavity",))


_MESHES = {}    # (kind, n) -> mesh: a workload and its constraints-on twin share one mesh ...
_ORACLES = {}   # ... and one oracle (its set-up is minutes of host time on the 10 M-cell mesh)


def get_mesh(kind, n):
    key = (kind, n)
    if key not in _MESHES:
        for k in [k for k in _MESHES if k != key]:      # one large mesh (and its oracle) at a time
            _MESHES.pop(k)
            o = _ORACLES.pop(k, None)
            if o is not None:
                o.close()
        _MESHES[key] = make_mesh(kind, n)
    return _MESHES[key]


def oracle_leg(kind, n_side, constraints, eng, prm, budget_s=12.0, layers=False, boundary=False, max_iters=40):
    """The checker and the reported CPU baseline in one pass: the serial oracle (CPU restatement of the reference loop;
    kind = "port": the reference itself needs OpenFOAM and cannot be built here) runs n iterations of THIS workload's own
    mesh from the initial coordinates -- n bounded by budget_s of CPU time -- and the engine `eng` runs the same n iterations
    from the same start; returns (cpu_baseline, parity_check).  Neither is part of any timed region."""
    import numpy as np
    from oracle import oracle_ffi
    mesh = get_mesh(kind, n_side)
    key = (kind, n_side)
    plain = not (layers or boundary)
    t0 = time.perf_counter()
    o = _ORACLES.get(key) if plain else None
    if o is None:
        o = oracle_ffi.Oracle(mesh)
        if plain:
            _ORACLES[key] = o
    setup_s = time.perf_counter() - t0
    o.set_points(mesh.points)
    o.set_params(prm)
    if layers or boundary:
        from smoothmesh_amd import LayerParams, patch_arrays
        lp = layer_params(kind) if layers else LayerParams()
        st, sz, kd, sel = patch_arrays(mesh, lp.layerPatches)
        lopt = (lp.layerMaxBlendingFraction, prm.minEdgeLength, lp.layerExpansionRatio, lp.minLayers, lp.maxLayers)
        if boundary:
            bp = boundary_params(kind, n_side)
            o.setup_boundary(st, sz, kd, sel, patch_arrays(mesh, bp.smoothingPatches)[3], lopt, bp.initEdges, bp.targetEdges, bp.targetSurfaces)
        else:
            o.setup_layers(st, sz, kd, sel, *lopt)
    # census of the oracle's threshold comparisons of angles (SM.C:923, 1367, 1391-1394, 1421-1424) over these iterations: the engine
    # takes acos with another algorithm than glibc (csrc/smacos.hpp, at most the last bit apart) -- how many comparisons had their
    # two sides within 8 ulp, i.e. could have been decided by that bit?  (a counter increment per comparison: not measurable in the rate)
    oracle_ffi.acos_census(True)
    t0 = time.perf_counter()
    _, res1, frz1 = o.iterate(1, 0.0)            # first iteration untimed: it also first-touches the oracle's work arrays
    t1 = time.perf_counter() - t0
    iters = max(1, min(max_iters - 1, int(budget_s / max(t1, 1e-3))))
    t0 = time.perf_counter()
    _, res2, frz2 = o.iterate(iters, 0.0)
    dt = time.perf_counter() - t0
    n = 1 + iters
    census = oracle_ffi.acos_census(False)
    res_o, frz_o = np.concatenate([res1, res2]), np.concatenate([frz1, frz2])
    pts_o = o.points()
    if not plain:
        o.close()
    base = {
        "value": mesh.nPoints * iters / dt, "unit": "points/s", "cores": 1, "kind": "port",
        "sample": f"{iters} iterations (after one untimed) of this workload's own mesh ({mesh.nPoints} points, {mesh.nCells} cells), "
                  f"serial oracle (g++ -O3 -ffp-contract=off), {dt:.1f} s; omits OpenFOAM overheads (movePoints, field rebuilds), "
                  f"so it is faster than the real reference"
                  + ("; with boundary point smoothing the oracle tests every target triangle per ray where OpenFOAM walks an "
                     "octree, so THIS number is slower than the real reference and no fair baseline" if boundary else ""),
        "host_cpus": os.cpu_count(), "oracle_setup_s": setup_s,
    }
    # the engine: the same n iterations from the same coordinates
    eng.set_points(mesh.points)
    n_g, res_g, frz_g = eng.iterate(n, 0.0)
    near_g = int(eng.last_near_ties.sum()) if hasattr(eng, "last_near_ties") else None
    pts_g = eng.get_points()
    denom = float(np.max(np.abs(pts_o)))
    par = {
        "iters": int(n), "against": "CPU oracle (oracle/), same mesh, same initial coordinates, same parameters",
        "rel_linf": float(np.max(np.abs(pts_g - pts_o)) / (denom if denom > 0 else 1.0)),
        "bitwise_equal": bool(np.array_equal(pts_g, pts_o)),
        "nFrozen_equal": bool(n_g == n and np.array_equal(frz_g, frz_o)),
        "residual_max_rel_diff": float(np.max(np.abs(res_g - res_o) / np.maximum(np.abs(res_o), 1e-300))) if n_g == n else None,
        "nFrozenPoints": [int(x) for x in frz_g[:4]],
        "tolerance": 1e-10,
        # the engine's own near-tie census over these n iterations (include/smgpu.h): angle comparisons with sides within 4 ulp
        "near_ties": near_g,
        "acos_census": {**census, "what": "the oracle's comparisons of an angle with a threshold / another angle in these iterations (oracle: "
                        "glibc acos, engine: csrc/smacos.hpp, at most the last bit apart); within_8ulp = sides 1..8 ulp apart, i.e. comparisons "
                        "the last bit could decide; equal = both sides the same function of the same inputs"},
    }
    par["ok"] = bool(par["rel_linf"] <= par["tolerance"] and par["nFrozen_equal"])
    return base, par


def workload_text(kind, n_side, constraints, layers, boundary, world=1, n_global=None):
    if kind == "hex":
        w = f"{n_side}^3-cell uniform hex block per GPU (blockMesh numbering)"
    elif world == 1:
        w = (f"castellated polyhedral cube-with-sphere-cavity, {n_side}^3 base grid + one 2:1 refinement shell "
             f"(own generator standing in for snappyHexMesh)")
    else:
        w = (f"castellated polyhedral cube-with-sphere-cavity, {n_global}^3 base grid + one 2:1 refinement shell (own generator "
             f"standing in for snappyHexMesh + decomposePar), cut into {world} boxes, one per GPU, each rank generating its own")
    cfg = (2 if constraints else 1) if kind == "hex" else (3 if world == 1 else 4)
    return (w + f", interior jitter 0.2h seed 12345, "
            f"{'edgeAngle+faceAngle constraints on (minAngle 35 / maxAngle 160)' if constraints else 'constraints off'}, "
            + ("boundary layer treatment on (" + ("all six sides" if kind == "hex" else "the cavity wall") + ", default layer options), "
               if layers else "") +
            f"relTol 0, defaults otherwise (BASELINE.json configs[{cfg}]"
            + (" + -layerPatches" if layers else "") + (" + constant/geometry/*.obj" if boundary else "") + ")"
            + (", boundary point smoothing on (" + ("all sides onto the block's own surface and feature edges" if kind == "hex"
                                                     else "the cavity wall onto the triangulated sphere") + ")" if boundary else ""))


# The constraint evaluators run as a conservative f32 filter followed by the exact kernels on what the filter left open.
# One pass of the evaluator over the mesh is the unit: its algorithmic bytes (every array element the exact algorithm touches
# once) against the summed time of its kernels.  (Charging the post-filter exact kernels the full-array bytes -- as round 2's
# table did -- printed bandwidths above the HBM peak for kernels that touch 2 % of the elements.)
KERNEL_UNITS = [
    ("edge_angle (filter + exact)", ["k_edge_angle_filter", "k_edge_angle"], ["k_edge_angle"]),
    ("face_angles_current (filter + list compaction + exact edges + points)", ["k_fa_edges_filter", "k_fa_edges", "k_fa_points"],
     ["k_fa_edges", "k_fa_points"]),
]


def kernel_report(workload, ctr, K, dt, dt_ev, sizes=None):
    """roofline objects + per-kernel table from the hipEvent counters of the second pass"""
    # HBM traffic per launch, measured separately under rocprofv3 --pmc (scripts/measure_traffic.sh) and
    # committed under profiles/; None when no measurement of this workload exists
    traffic = None
    tdoc = None
    for rnd in ("r6", "r5", "r4", "r3", "r2", "r1"):
        tpath = os.path.join(ROOT, "profiles", rnd, f"traffic_{workload}.json")
        if os.path.exists(tpath):
            tdoc = json.load(open(tpath))
            tdoc["_round"] = rnd
            break
    by_name = {c["name"]: c for c in ctr}
    ctr = sorted(ctr, key=lambda c: -c["ms"])

    def us(c):
        return c["ms"] / c["launches"] * 1e3

    def roof(c):
        """roofline object of one counter: HBM bytes when the kernel has an algorithmic byte count, else FP64 instructions"""
        avg_s = us(c) * 1e-6
        r = {"kernel": c["name"], "avg_launch_us": us(c)}
        if c["algoBytesPerLaunch"] > 1024:
            ach = c["algoBytesPerLaunch"] / avg_s / 1e9
            r.update({"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                      "algorithmic_bytes_per_launch": int(c["algoBytesPerLaunch"])})
        if c.get("algoF64OpsPerLaunch"):
            v = {"algorithmic_ops_per_launch": int(c["algoF64OpsPerLaunch"]),
                 "achieved_Tops": c["algoF64OpsPerLaunch"] / avg_s / 1e12, "peak_Tops": FP64_VALU_PEAK_TOPS,
                 "frac": c["algoF64OpsPerLaunch"] / avg_s / 1e12 / FP64_VALU_PEAK_TOPS}
            if "bound" in r:
                r["valu_f64"] = v
            else:   # no streaming byte count: priced against the FP64 vector instruction rate only
                r.update({"bound": "valu_f64", "achieved": v["achieved_Tops"], "peak": FP64_VALU_PEAK_TOPS, "unit": "T FP64 instr/s",
                          "frac": v["frac"], "algorithmic_ops_per_launch": v["algorithmic_ops_per_launch"]})
        return r

    # dominant device kernel = the largest total time among the kernels that carry an algorithmic count (no name is excluded)
    cand = [c for c in ctr if c["algoBytesPerLaunch"] > 1024 or c.get("algoF64OpsPerLaunch")]
    roofline = None
    if cand:
        dom = cand[0]
        roofline = roof(dom)
        if tdoc:
            for kname, kv in tdoc["kernels"].items():
                if kname.split("<")[0] == dom["name"].split("<")[0].replace("k_smooth", "k_smooth_tile"):
                    traffic = int(2 * kv["FETCH_SIZE_KB"] * 1024 + kv["WRITE_SIZE_KB"] * 1024)
                    roofline["traffic_source"] = f"profiles/{tdoc['_round']}/traffic_{workload}.json"
                    # NOT measured by this run: a committed measurement of the same kernel on the same workload
                    roofline["traffic_measured_by"] = ("builder, round " + tdoc["_round"][1:] + ", rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes "
                                                       "(scripts/measure_traffic.sh; FETCH_SIZE x 2 on gfx950), read from the committed file -- "
                                                       "not re-measured in this run")
        roofline["traffic"] = traffic
        roofline["note"] = ("per-kernel durations from hipEvents on the engine's stream in a second pass over the same K steps, every kernel "
                            "ALONE on the chip (the side streams are off in that pass); "
                            "meshes whose working set is < 256 MiB (e.g. 100^3) are Infinity-Cache resident: read their fraction as "
                            "cache-level throughput, not as an HBM-roofline test; valu_f64 = the rate of ALGORITHMIC FP64 instructions "
                            "(sqrt = 22, division = 11 as expanded, no FMA contraction) against 256 CUs x 64 lanes x 2.4 GHz")
    gather = next((c for c in ctr if c["name"].startswith("k_smooth")), None)
    rows = []
    grouped = set()
    for label, members, byte_src in KERNEL_UNITS:
        mem = [by_name[m] for m in members if m in by_name]
        if not mem:
            continue
        grouped.update(c["name"] for c in mem)
        t_us = sum(us(c) for c in mem)
        nbytes = sum(by_name[m]["algoBytesPerLaunch"] for m in byte_src if m in by_name)
        rows.append({"name": label, "kernels": {c["name"]: us(c) for c in mem}, "launches": int(max(c["launches"] for c in mem)),
                     "avg_us": t_us, "algo_GBps": nbytes / (t_us * 1e-6) / 1e9 if nbytes else None, "_ms": sum(c["ms"] for c in mem)})
    for c in ctr:
        if c["name"] in grouped:
            continue
        rows.append({"name": c["name"], "launches": int(c["launches"]), "avg_us": us(c),
                     "algo_GBps": c["algoBytesPerLaunch"] / (us(c) * 1e-6) / 1e9 if c["algoBytesPerLaunch"] > 1024 else None,
                     **({"algo_f64_Tops": c["algoF64OpsPerLaunch"] / (us(c) * 1e-6) / 1e12} if c.get("algoF64OpsPerLaunch") else {}),
                     "_ms": c["ms"]})
    rows.sort(key=lambda r: -r.pop("_ms"))
    # The centroid-gather kernel (BASELINE.json's 40 % target) with BOTH byte accountings: the fused kernel's own algorithmic bytes
    # (centroid gather + closest points + clamp + edge-length freeze: K_cg + K_prop's lists) and SURVEY 8(d)'s K_cg bytes alone
    # (4(P+1) + 4 nnz_pc + 24 C + 24 P + P + 24 P) -- the fused kernel does all of K_cg's traffic and more in that time, so the
    # K_cg-only figure is a lower bound of what a kernel doing only K_cg would reach.
    gather_obj = None
    if gather is not None:
        gather_obj = {**roof(gather), "note": "the fused centroid-gather + proposal kernel (the kernel BASELINE.json's 40 % target names), timed alone"}
        if sizes:
            P_, C_, npc = int(sizes["nPoints"]), int(sizes["nCells"]), int(sizes["nnzPointCells"])
            kcg = 4 * (P_ + 1) + 4 * npc + 24 * C_ + 24 * P_ + P_ + 24 * P_
            ach = kcg / (us(gather) * 1e-6) / 1e9
            gather_obj["accountings"] = {
                "fused (this kernel's algorithmic bytes)": {"bytes_per_launch": int(gather["algoBytesPerLaunch"]), "achieved_GBps": gather_obj.get("achieved"),
                                                           "frac": gather_obj.get("frac")},
                "K_cg only (SURVEY 8d)": {"bytes_per_launch": int(kcg), "achieved_GBps": ach, "frac": ach / HBM_PEAK_GBS}}
    # Constraints on: the iteration is two chains that run side by side between the geometry kernel and the freeze walk -- the
    # main stream (proposal, edge-angle evaluator) and the side stream (face-angle filter, list compaction, exact pass of the
    # current coordinates).  Their kernels were timed alone; an iteration costs at least the longer chain plus the serial part.
    by = {c["name"]: us(c) for c in ctr}
    side_names = ["k_fa_edges_filter", "k_fa_edges", "k_fa_points"]
    main_par = ["k_smooth<proposal>", "k_edge_angle_filter", "k_edge_angle"]
    chains = None
    if any(n in by for n in side_names):
        side = sum(by.get(n, 0.0) for n in side_names)
        mainp = sum(by.get(n, 0.0) for n in main_par)
        serial = sum(v for n, v in by.items() if n not in side_names and n not in main_par)
        chains = {"unit": "us per iteration, every kernel timed alone",
                  "serial_part": {n: by[n] for n in by if n not in side_names and n not in main_par}, "serial_part_us": serial,
                  "main_stream_chain": {n: by[n] for n in main_par if n in by}, "main_stream_chain_us": mainp,
                  "side_stream_chain": {n: by[n] for n in side_names if n in by}, "side_stream_chain_us": side,
                  "sum_all_alone_us": serial + mainp + side, "critical_path_us": serial + max(mainp, side),
                  "ms_per_step_measured": dt / K * 1e3,
                  "note": "ms_per_step (both chains side by side) lies between critical_path_us and sum_all_alone_us: kernels that share "
                          "the chip slow each other down (both chains are FP64-issue bound)"}
    return {
        "roofline": roofline,
        "roofline_centroid_gather": gather_obj,
        **({"chains": chains} if chains else {}),
        "kernels": rows,
        "ms_per_step_with_events": dt_ev / K * 1e3,
    }


PRE_SECONDS = float(os.environ.get("SMOOTHMESH_BENCH_PRE_S", "0.3"))


def clock_warm(iterate, engine, sync, fixed=0):
    """Before the W warm-up and K timed steps the contract asks for: run the workload itself for PRE_SECONDS so that the GPU
    is at its sustained clocks (a 20-step run of a 0.1 ms step is over before the power management has left the idle state),
    then put the initial coordinates back (from a pinned host copy: a sub-millisecond gap).  Returns the iterations spent."""
    import torch
    if PRE_SECONDS <= 0:
        return 0
    p0 = engine.get_points()
    pinned = torch.empty(p0.shape, dtype=torch.float64).pin_memory().numpy()
    pinned[...] = p0
    done, chunk = 0, 20
    sync()
    if fixed:      # several ranks: the same number of iterations on every rank (the exchanges are collective)
        iterate(fixed)
        sync()
        engine.set_points(pinned)
        return fixed
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < PRE_SECONDS:
        iterate(chunk)
        sync()
        done += chunk
        chunk = min(2 * chunk, 400)
    engine.set_points(pinned)
    return done


DUMP_LIMIT_BYTES = 64 * 2**20     # --dump-outputs: all arrays together


def dump_outputs(path, points, res, frz):
    """--dump-outputs DIR: what the timed iterate() call handed its caller after the last timed step -- the coordinates
    (smgpu_get_points), the per-iteration residual and nFrozenPoints -- as DIR/<name>.npy in float64.  Coordinates larger than
    DUMP_LIMIT_BYTES are written as a fixed sample of points (seed 0, ascending rows) with the row numbers beside them."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name in ("points", "points_sample", "points_sample_index", "residual", "nFrozenPoints"):     # nothing stale from an earlier run
        if os.path.exists(os.path.join(path, name + ".npy")):
            os.remove(os.path.join(path, name + ".npy"))
    pts = np.ascontiguousarray(points, dtype=np.float64)
    out = {"residual": np.asarray(res, dtype=np.float64), "nFrozenPoints": np.asarray(frz, dtype=np.float64)}
    room = DUMP_LIMIT_BYTES - sum(a.nbytes for a in out.values()) - 4096
    if pts.nbytes <= room:
        out["points"] = pts
    else:
        idx = np.sort(np.random.default_rng(0).choice(len(pts), size=room // (pts.itemsize * 4), replace=False))
        out["points_sample"] = pts[idx]
        out["points_sample_index"] = idx.astype(np.float64)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def run_single(workload, K, W, device, oracle=True, oracle_budget_s=12.0, nominal100=False, keep_points=False, full=True):
    """one GPU, one workload: W warm-up + K timed steps on a cold GPU (ms_per_step_cold), the clock pre-run, W + K again (the
    reported value; inputs resident), and with `full` -- outside every timed region -- the same K steps with per-kernel
    hipEvents, the near-tie census and the oracle leg (parity_check + cpu_baseline on this workload's own mesh; only if
    `oracle` too).  keep_points: also return the coordinates the timed steps left (read after the clock has stopped)"""
    import torch
    from smoothmesh_amd import SmoothEngine, default_params
    kind, n_side, constraints = parse_workload(workload)
    layers, boundary = workload_layers(workload), workload_boundary(workload)
    t_setup = time.perf_counter()
    mesh = get_mesh(kind, n_side)
    t_mesh = time.perf_counter() - t_setup
    t0 = time.perf_counter()
    eng = SmoothEngine(mesh, device=device)
    prm = default_params(eng.mesh_stats()[0], edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
    eng.set_params(prm)
    if layers and not eng.set_layers(layer_params(kind), prm.minEdgeLength):
        raise SystemExit("boundary layer treatment could not be enabled")
    if boundary and not eng.set_boundary_smoothing(boundary_params(kind, n_side), prm.minEdgeLength)["enabled"]:
        raise SystemExit("boundary point smoothing could not be enabled")
    t_create = time.perf_counter() - t0

    def timed():
        if W:
            eng.iterate(W, 0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, res, frz = eng.iterate(K, 0.0)          # returns after the stream has drained
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert n == K
        return dt, res, frz

    dt_cold, _, _ = timed()                        # exactly the contract's W + K on a GPU that has just left its idle clocks
    eng.set_points(mesh.points)
    pre = clock_warm(lambda k: eng.iterate(k, 0.0), eng, torch.cuda.synchronize)
    dt, res, frz = timed()
    points = eng.get_points() if keep_points else None
    near_timed = eng.last_near_ties.sum() if full and hasattr(eng, "last_near_ties") else 0
    # the metric says "(100 iters)": when the contract's K is shorter (the driver runs 20 steps = 1.7 ms on the hex block), the same
    # loop once more over 100 steps from the initial coordinates, reported beside the K-step value
    dt100 = None
    if K < 100 and nominal100 and full:
        eng.set_points(mesh.points)
        if W:
            eng.iterate(W, 0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.iterate(100, 0.0)
        torch.cuda.synchronize()
        dt100 = time.perf_counter() - t0
    dt_ev = ctr = None
    if full:
        # second pass over the same K steps with per-kernel hipEvent brackets (on the engine's stream)
        eng.reset_counters()
        eng.enable_timing(True)
        t0 = time.perf_counter()
        eng.iterate(K, 0.0)
        dt_ev = time.perf_counter() - t0
        eng.enable_timing(False)
        ctr = [c for c in eng.counters() if c["launches"] > 0 and c["ms"] > 0]
    sizes = eng.sizes()
    nPoints = mesh.nPoints
    base = par = None
    t0 = time.perf_counter()
    if oracle and full:
        base, par = oracle_leg(kind, n_side, constraints, eng, prm, budget_s=oracle_budget_s, layers=layers, boundary=boundary)
    t_oracle = time.perf_counter() - t0
    # near-tie census of everything this engine ran (include/smgpu.h): angle comparisons with sides within 4 ulp -- the decisions
    # the reference's acos could take the other way; zero = none
    # (since_create includes the clock pre-run: hundreds of iterations that drive a SMALL mesh to convergence, where steps of an ulp
    # make near ties of their own; the summary quotes the iterations that were compared with the oracle, else the timed ones)
    near = {**eng.near_ties(), "timed_steps": int(near_timed)} if full and hasattr(eng, "near_ties") else None
    eng.close()
    del eng
    return dict(kind=kind, n_side=n_side, constraints=constraints, layers=layers, boundary=boundary, dt=dt, dt_cold=dt_cold, dt_ev=dt_ev,
                ctr=ctr, sizes=sizes, total_points=nPoints, res=res, frz=frz, points=points, pre=pre, cpu_baseline=base, parity_check=par, near_ties=near,
                dt100=dt100, phases={"mesh_generation_s": t_mesh, "engine_setup_s": t_create, "oracle_leg_s": t_oracle})


def make_subdomain(kind, n_side, grid, rank, world):
    """this rank's sub-domain of the weak-scaling workload: hexN = an N^3 block per rank of the (Px N, Py N, Pz N) block; cavityN =
    box `rank` of the castellated polyhedral mesh on a round(N world^(1/3))^3 base grid (every rank generates ITS box only)"""
    if kind == "hex":
        from smoothmesh_amd.meshgen import hex_subdomain
        return hex_subdomain((n_side, n_side, n_side), grid, rank, jitter=0.2, seed=12345), None
    from smoothmesh_amd.polymesh import cavity_subdomain
    n_global = int(round(n_side * world ** (1.0 / 3.0)))
    return cavity_subdomain(n_global, grid, rank, jitter=0.2, seed=12345), n_global


def small_case_parity(kind, constraints, grid, rank, world, device, iters=6, overlap=False):
    """parity_check (b) of an N > 1 line: a down-scaled case of the same family on the SAME processor grid, run through the SAME
    transport in this very job (DistributedSmoother picks it exactly as for the timed workload), against the oracle's MultiDomain
    (the reference under mpirun with the same decomposition).  Every rank builds the small expected result itself (a few
    thousand cells) and compares its own sub-domain; the verdict is reduced over the ranks."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from oracle import oracle_ffi
    from smoothmesh_amd import default_params
    from smoothmesh_amd.decompose import shared_point_table
    from smoothmesh_amd.halo import DistributedSmoother
    n_small = 12 if kind == "hex" else 24
    if kind == "hex":
        from smoothmesh_amd.meshgen import hex_subdomain
        subs = [hex_subdomain((n_small,) * 3, grid, r, jitter=0.2, seed=12345) for r in range(world)]
        what = f"{n_small}^3-cell hex block per rank"
    else:
        from smoothmesh_amd.polymesh import cavity_subdomain
        subs = [cavity_subdomain(n_small, grid, r, jitter=0.2, seed=12345) for r in range(world)]
        what = f"castellated polyhedral cavity mesh on a {n_small}^3 base grid"
    orcs = [oracle_ffi.Oracle(sd.mesh) for sd in subs]
    prm = default_params(min(o.mesh_stats()[0] for o in orcs), edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
    for o in orcs:
        o.set_params(prm)
    mo = oracle_ffi.MultiOracle(orcs, *shared_point_table(subs))
    n_o, res_o, frz_o = mo.iterate(iters, 0.0)
    ds = DistributedSmoother(subs[rank], device=device, overlap=overlap)
    ds.set_params(prm)
    n_g, res_g, frz_g = ds.iterate(iters, 0.0)
    mine, want = ds.get_points(), orcs[rank].points()
    info = ds.transport_info()
    hm = ds.engine.debug_halo_mode() if hasattr(ds.engine, "debug_halo_mode") else {}
    info["form"] = ("multi-role launches" + (", flagged" if hm.get("flagged") else "")) if hm.get("multi_role") else "one kernel per step"
    ds.close()
    for o in orcs:
        o.close()
    denom = float(np.max(np.abs(want)))
    rel = float(np.max(np.abs(mine - want)) / (denom if denom > 0 else 1.0))
    ok = bool(n_g == n_o and np.array_equal(np.asarray(frz_g), np.asarray(frz_o)) and rel <= 1e-10)
    rdev = "cpu" if dist.get_backend() == "gloo" else torch.device("cuda", device)
    t = torch.tensor([1.0 if ok else 0.0, -rel, 1.0 if np.array_equal(mine, want) else 0.0], dtype=torch.float64, device=rdev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return {"case": f"{what}, cut {grid[0]}x{grid[1]}x{grid[2]}, {'constraints on' if constraints else 'constraints off'}, {iters} iterations",
            "against": "oracle MultiDomain (the reference under mpirun, same decomposition), every rank its own sub-domain",
            "transport": info["transport"], "form": info["form"], "exchange_stream": bool(overlap),
            "ok": bool(t[0].item() == 1.0), "rel_linf_max_over_ranks": float(-t[1].item()),
            "bitwise_equal_on_every_rank": bool(t[2].item() == 1.0), "nFrozenPoints": [int(x) for x in np.asarray(frz_g)[:4]], "tolerance": 1e-10}


def shared_copies_check(ds, sub):
    """parity_check (a) of an N > 1 line: after the timed steps, are the copies of every shared point bit-identical on all the
    ranks that hold it?  One gather of (global point id, 64-bit hash of the three coordinates, internal-point flag) per shared
    point to rank 0.  Points on which the sharers disagree about internal / boundary are set aside and counted: findInternalMeshPoints
    is rank-local in the reference (SM.C:40-91), such a point is restored on one rank and moved on another there too."""
    import numpy as np
    dist = ds.dist
    t = ds.tables
    loc = np.asarray(t.sharedLocal, np.int64)
    pts = np.ascontiguousarray(ds.get_points().reshape(-1, 3)[loc])
    bits = pts.view(np.uint64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        h = (bits[:, 0] * np.uint64(0x9E3779B97F4A7C15)) ^ (bits[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9)) \
            ^ ((bits[:, 2] << np.uint64(17)) | (bits[:, 2] >> np.uint64(47)))
    # a shared point is named by (global id, group): the id alone is not enough once a baffle lies between ranks (one mesh point,
    # two shared points, HaloTables.sharedComp); the groups' labels are the same on every rank
    gid = np.asarray(sub.pointProcAddressing, np.int64)[loc] * np.int64(1 << 20) + (np.asarray(t.sharedComp, np.int64) % np.int64(1 << 20))
    internal = np.asarray(sub.mesh.find_internal_points(), np.uint8)[loc]
    box = [None] * ds.world if ds.rank == 0 else None
    dist.gather_object((gid, h, internal), box, dst=0)
    if ds.rank != 0:
        return None
    g = np.concatenate([b[0] for b in box]); hh = np.concatenate([b[1] for b in box]); ii = np.concatenate([b[2] for b in box])
    order = np.argsort(g, kind="stable")
    g, hh, ii = g[order], hh[order], ii[order]
    first = np.concatenate([[True], g[1:] != g[:-1]]) if len(g) else np.zeros(0, bool)
    run = np.cumsum(first) - 1
    nrun = int(run[-1]) + 1 if len(g) else 0
    hmin = np.full(nrun, np.iinfo(np.uint64).max, np.uint64); hmax = np.zeros(nrun, np.uint64)
    imin = np.full(nrun, 255, np.uint8); imax = np.zeros(nrun, np.uint8)
    np.minimum.at(hmin, run, hh); np.maximum.at(hmax, run, hh)
    np.minimum.at(imin, run, ii); np.maximum.at(imax, run, ii)
    rogue = imin != imax
    bad = (hmin != hmax) & ~rogue
    return {"shared_points": nrun, "copies": int(len(g)), "mismatching_points": int(bad.sum()),
            "decomposition_dependent_points_set_aside": int(rogue.sum()), "ok": bool(not bad.any()),
            "what": "after the timed steps: every copy of a shared point carries the same 64-bit coordinate hash on all ranks that hold it"}


def rank0_cpu_baseline(sub, prm, budget_s, rank, world):
    """cpu_baseline of an N > 1 line: rank 0's serial oracle on ITS OWN sub-domain (as a serial mesh: processor-patch points are
    internal points there, nothing is combined), one core; the job's CPU rate with one core per rank would be ~ world x this"""
    from oracle import oracle_ffi
    if rank != 0:
        return None
    t0 = time.perf_counter()
    o = oracle_ffi.Oracle(sub.mesh)
    setup_s = time.perf_counter() - t0
    o.set_params(prm)
    t0 = time.perf_counter()
    o.iterate(1, 0.0)
    t1 = time.perf_counter() - t0
    iters = max(1, min(39, int(budget_s / max(t1, 1e-3))))
    t0 = time.perf_counter()
    o.iterate(iters, 0.0)
    dtc = time.perf_counter() - t0
    o.close()
    return {"value": sub.mesh.nPoints * iters / dtc, "unit": "points/s", "cores": 1, "kind": "port",
            "sample": f"{iters} iterations (after one untimed) of RANK 0's sub-domain as a serial mesh ({sub.mesh.nPoints} points, "
                      f"{sub.mesh.nCells} cells; its processor-patch points are internal points, nothing is exchanged), serial oracle "
                      f"(g++ -O3 -ffp-contract=off), {dtc:.1f} s; omits OpenFOAM overheads, so it is faster than the real reference; "
                      f"the reference under mpirun -np {world} with one core per rank would run at about {world} x this",
            "host_cpus": os.cpu_count(), "oracle_setup_s": setup_s}


def run_distributed(workload, K, W, rank, world, local_rank, backend, oracle=True, force_dist=False, oracle_budget_s=12.0,
                    keep_points=False, full=True):
    """N ranks, one workload: per-rank sub-domain, exchange arrangement autotuned (with `oracle`: the exchange-stream arrangement
    only a candidate after its check), clock pre-run, W warm-up + K timed steps between barriers (max over ranks); transport = how
    the records travelled (communicator size included); with `full`, outside the timed region: the same K steps with per-kernel
    hipEvents, halo_cost, and (with `oracle` too) parity_check (a) copies of shared points identical across ranks, (b) a
    down-scaled case through the same transport against the oracle's MultiDomain; cpu_baseline = rank 0's oracle on its own
    sub-domain.  keep_points: also return this rank's coordinates after the timed steps"""
    import torch
    import torch.distributed as dist
    from smoothmesh_amd import default_params
    from smoothmesh_amd.halo import DistributedSmoother
    kind, n_side, constraints = parse_workload(workload)
    layers, boundary = workload_layers(workload), workload_boundary(workload)
    grid = proc_grid(world)
    rdev = "cuda" if backend == "nccl" else "cpu"
    small = None
    if oracle and full and world > 1:
        try:
            small = small_case_parity(kind, constraints, grid, rank, world, local_rank)
        except Exception as ex:   # noqa: BLE001 -- reported in the line, the measurement goes on (on every rank alike)
            small = {"ok": False, "error": f"{type(ex).__name__}: {ex}"}
        # a failure on SOME ranks only (an oracle mismatch that raised, a device error) must become every rank's verdict before the
        # next collective; a rank that died inside a collective cannot be helped from here
        bad = torch.tensor([0 if (small or {}).get("ok") or "error" not in (small or {}) else 1], dtype=torch.int32, device=rdev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if int(bad.item()) and "error" not in small:
            small = {"ok": False, "error": "small case raised on another rank"}
    t0 = time.perf_counter()
    sub, n_global = make_subdomain(kind, n_side, grid, rank, world)
    t_mesh = time.perf_counter() - t0
    t0 = time.perf_counter()
    ds = DistributedSmoother(sub, device=local_rank, probe_slots=60000 if force_dist else 0)
    prm = default_params(ds.global_min_edge(), edgeAngleConstraint=constraints, faceAngleConstraint=constraints)
    ds.set_params(prm)
    if layers and not ds.set_layers(layer_params(kind), prm.minEdgeLength):
        raise SystemExit("boundary layer treatment could not be enabled")
    if boundary:   # hex: every rank is a unit cube of the global block [0, grid]; cavity: the global unit cube
        hi = tuple(float(g) for g in grid) if kind == "hex" else (1.0, 1.0, 1.0)
        if not ds.set_boundary_smoothing(boundary_params(kind, n_side, hi), prm.minEdgeLength)["enabled"]:
            raise SystemExit("boundary point smoothing could not be enabled")
    t_create = time.perf_counter() - t0
    # The exchange-stream arrangement (with the constraints off: the two multi-role launches with the exchanges NEXT TO them, ordered
    # by flag words -- never run between two devices before the first multi-GPU node) is only a candidate of the autotune below if
    # the down-scaled case gives the oracle's MultiDomain result through it on every rank of THIS job; waits are bounded (10 s here)
    flagged_check = None
    allow_overlap = world == 1
    if oracle and world > 1 and backend == "nccl" and os.environ.get("SMOOTHMESH_EXCHANGE", "") != "push" and os.environ.get("SMOOTHMESH_OVERLAP") is None:
        prev_to = os.environ.get("SMGPU_PUSH_TIMEOUT_S")
        os.environ["SMGPU_PUSH_TIMEOUT_S"] = "10"
        try:
            flagged_check = small_case_parity(kind, constraints, grid, rank, world, local_rank, overlap=True)
        except Exception as ex:   # noqa: BLE001
            flagged_check = {"ok": False, "error": f"{type(ex).__name__}: {ex}"}
        finally:
            if prev_to is None:
                os.environ.pop("SMGPU_PUSH_TIMEOUT_S", None)
            else:
                os.environ["SMGPU_PUSH_TIMEOUT_S"] = prev_to
        okf = torch.tensor([1 if flagged_check.get("ok") else 0], dtype=torch.int32, device=rdev)
        dist.all_reduce(okf, op=dist.ReduceOp.MIN)
        allow_overlap = bool(int(okf.item()))
        if not allow_overlap:
            flagged_check["ok"] = False
    # ... and only if the REAL workload (far more shared tiles than the down-scaled case: spinning shared-point workgroups, the
    # RCCL kernel and the relay compete for resident slots) gives the in-order result bit for bit over a few iterations
    if allow_overlap and world > 1 and flagged_check is not None and getattr(ds, "xstream", None) is not None:
        import numpy as np
        real = {"iters": 3}
        prev_to = os.environ.get("SMGPU_PUSH_TIMEOUT_S")
        os.environ["SMGPU_PUSH_TIMEOUT_S"] = "10"
        try:
            p0 = ds.engine.get_points()
            ds.set_overlap(False)
            ds.iterate(3, 0.0)
            a = ds.engine.get_points()
            ds.engine.set_points(p0)
            ds.set_overlap(True)
            ds.iterate(3, 0.0)
            b = ds.engine.get_points()
            real["bitwise_equal_to_inorder"] = bool(np.array_equal(a, b))
            real["ok"] = real["bitwise_equal_to_inorder"]
        except Exception as ex:   # noqa: BLE001
            real.update({"ok": False, "error": f"{type(ex).__name__}: {ex}"})
        finally:
            if prev_to is None:
                os.environ.pop("SMGPU_PUSH_TIMEOUT_S", None)
            else:
                os.environ["SMGPU_PUSH_TIMEOUT_S"] = prev_to
        okf = torch.tensor([1 if real.get("ok") else 0], dtype=torch.int32, device=rdev)
        dist.all_reduce(okf, op=dist.ReduceOp.MIN)
        allow_overlap = bool(int(okf.item()))
        ds.set_overlap(False)
        try:
            ds.engine.set_points(p0)
        except Exception:   # noqa: BLE001 -- (p0 unset: get_points itself failed; the run below will say so)
            pass
        flagged_check["real_workload"] = real
        if not allow_overlap:
            flagged_check["ok"] = False
    # exchange arrangement (in order on the engine's stream / on a communication stream next to the
    # exchange-independent kernels): timed on this machine before the warm-up, same choice on every rank
    tune = ds.autotune(20, allow_overlap=allow_overlap) if os.environ.get("SMOOTHMESH_OVERLAP") is None else None
    if tune is None:
        ds.set_overlap(os.environ["SMOOTHMESH_OVERLAP"] == "1")
    pre = clock_warm(lambda k: ds.iterate(k, 0.0), ds.engine, lambda: (torch.cuda.synchronize(), dist.barrier()), fixed=200 if K >= 20 else 5)
    if W:
        ds.iterate(W, 0.0)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, res, frz = ds.iterate(K, 0.0)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0
    tt = torch.tensor([dt_local], dtype=torch.float64, device=rdev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    npts = torch.tensor([sub.mesh.nPoints], dtype=torch.float64, device=rdev)
    dist.all_reduce(npts, op=dist.ReduceOp.SUM)
    total_points = int(npts.item())      # points of all sub-domains (shared points counted per rank,
    eng = ds.engine                      # as the reference's per-rank loops process them)
    points = eng.get_points() if keep_points else None
    copies = shared_copies_check(ds, sub) if world > 1 and full else None      # parity_check (a): the state the timed steps left
    dt_ev = ctr = None
    if full:
        eng.reset_counters()
        eng.enable_timing(True)
        t0 = time.perf_counter()
        ds.iterate(K, 0.0)
        torch.cuda.synchronize()
        dt_ev = time.perf_counter() - t0
        eng.enable_timing(False)
        ctr = [c for c in eng.counters() if c["launches"] > 0 and c["ms"] > 0]
    sizes = dict(eng.sizes())
    info = ds.transport_info()
    hm = eng.debug_halo_mode() if hasattr(eng, "debug_halo_mode") else {}
    info["iteration_form"] = (("multi-role launches (k_geom_halo / k_smooth_halo on tiles of the shared points)" + (", flagged" if hm.get("flagged") else "")
                               + (", fix role inside" if hm.get("fix_inside") else "")) if hm.get("multi_role") else "one kernel per step")
    if flagged_check is not None:
        info["exchange_stream_check"] = flagged_check
    parallelism = (f"domain decomposition {grid[0]}x{grid[1]}x{grid[2]}, "
                   + {"direct": "RCCL send/recv groups on the engine's stream, ", "push": "peer stores (the pack kernels write the peers' receive slots), ",
                      "torch": f"{'RCCL' if backend == 'nccl' else backend + ' (debug)'} all_to_all halo, "}[info["transport"]] +
                   f"exchange {'overlapped on a communication stream' if getattr(ds, 'overlap', False) else 'in order'}"
                   + (f" (autotuned: {tune['us_per_iter']})" if tune and tune['us_per_iter'] else ""))
    ds.close()               # streams drained, second communicator destroyed -- on every rank, before the group goes
    # what the multi-rank code path costs per iteration BEFORE any byte crosses a link: every rank's own sub-domain as a serial mesh
    # (its processor-patch points are plain internal points, nothing is packed, combined or exchanged) through the single-rank loop,
    # same W + K steps, max over the ranks
    halo_cost = None
    if full and not (layers or boundary) and (world > 1 or force_dist):
        from smoothmesh_amd import SmoothEngine
        se = SmoothEngine(sub.mesh, device=local_rank)
        se.set_params(prm)
        se.iterate(max(W, 5), 0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        se.iterate(K, 0.0)
        torch.cuda.synchronize()
        ts = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=rdev)
        se.close()
        dist.all_reduce(ts, op=dist.ReduceOp.MAX)
        dt_s = float(ts.item())
        halo_cost = {"serial_ms_per_step": dt_s / K * 1e3, "ms_per_step": dt / K * 1e3, "halo_overhead_us": (dt - dt_s) / K * 1e6,
                     "weak_efficiency_bound": dt_s / dt,
                     "note": "serial = every rank's own sub-domain as a serial mesh through the single-rank loop (nothing packed, combined or "
                             "exchanged), same steps, max over ranks; the difference is the multi-rank code path (halo roles, exchanges, "
                             "k_shared_fix) plus link time; bound = serial / multi-rank"}
    t0 = time.perf_counter()
    base = rank0_cpu_baseline(sub, prm, oracle_budget_s, rank, world) if oracle and full else None
    t_oracle = time.perf_counter() - t0
    dist.barrier()           # (the other ranks wait for rank 0's oracle here)
    par = None
    if world > 1 and oracle and full:
        par = {"shared_point_copies": copies, "small_case": small,
               "ok": bool((copies or {}).get("ok", rank != 0) and (small or {}).get("ok", False))}
    return dict(kind=kind, n_side=n_side, constraints=constraints, layers=layers, boundary=boundary, dt=dt, dt_ev=dt_ev, ctr=ctr, sizes=sizes,
                total_points=total_points, res=res, frz=frz, points=points, pre=pre, cpu_baseline=base, parity_check=par, transport=info,
                parallelism=parallelism, n_global=n_global, halo_cost=halo_cost,
                phases={"mesh_generation_s": t_mesh, "engine_setup_s": t_create, "oracle_leg_s": t_oracle})


def self_launch(args):
    """--gpus N > 1 without a launcher: start the N ranks ourselves (one process per GPU, torch.distributed.run) BEFORE
    anything in this process touches the GPU, relay rank 0's JSON line and exit with the launcher's code"""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            print(line, flush=True)
    raise SystemExit(r.returncode)


def _parity_ok(par):
    return par is None or bool(par.get("ok", False))


def finalize_line(out):
    """Last step before printing: (1) append `configs_summary` as the LAST key -- one short object per measured configuration
    (headline first), so that a reader who only keeps the tail of the ~15 KB line still sees every configuration's rate, parity
    verdict and CPU ratio; (2) the process exit code: non-zero when any parity_check is not ok or any configs[] entry carries an
    error (the line is printed either way; a wrong or missing result must not look like a pass).  Returns (out, exit_code)."""
    def brief(wl, e):
        par = e.get("parity_check")
        b = {"workload": wl, "steps": e.get("steps"), "ms_per_step": e.get("ms_per_step"), "points_per_s": e.get("value"),
             "parity_ok": None if par is None else bool(par.get("ok", False)),
             "bitwise_equal": None if par is None else par.get("bitwise_equal", (par.get("small_case") or {}).get("bitwise_equal_on_every_rank")),
             "cpu_ratio": e.get("speedup_vs_cpu_baseline")}
        rf = _roof_brief(e.get("roofline"))
        if rf:      # the dominant kernel of THIS configuration: name, launch time, HBM fraction, and the ceiling that binds it
            b.update({"dominant_kernel": rf["kernel"], "avg_launch_us": rf["avg_launch_us"], "roofline_bound": rf["bound"],
                      "roofline_frac": rf["frac"], "binding": rf["binding"]})
            if "valu_f64_frac" in rf:
                b["valu_f64_frac"] = rf["valu_f64_frac"]
            if rf.get("traffic") is not None and rf.get("algorithmic_bytes_per_launch"):
                b["traffic_over_algorithmic"] = rf["traffic"] / rf["algorithmic_bytes_per_launch"]
        g = _gather_brief(e.get("roofline_centroid_gather"))
        if g and g.get("frac_K_cg") is not None:
            b["gather_frac_K_cg"] = g["frac_K_cg"]
        if e.get("near_ties") is not None:      # angle comparisons within 4 ulp (the reference's acos could decide them the other way)
            pn = (par or {}).get("near_ties")
            b["near_ties"] = pn if pn is not None else e["near_ties"].get("timed_steps", e["near_ties"]["total"])
        if "error" in e:
            b["error"] = e["error"][:200]
        return b
    out.pop("configs_summary", None)
    entries = [(out.get("workload_name", "headline"), out)] + [(c.get("workload", "?"), c) for c in out.get("configs", [])]
    failures = []
    for wl, e in entries:
        if "error" in e:
            failures.append(f"{wl}: {e['error']}")
        elif not _parity_ok(e.get("parity_check")):
            failures.append(f"{wl}: parity_check not ok")
    out["exit_code"] = 1 if failures else 0
    if failures:
        out["failures"] = failures
    out["configs_summary"] = [brief(wl, e) for wl, e in entries]       # LAST key: survives a tail of the line
    return out, out["exit_code"]


COMPACT_LIMIT = 4096     # bytes: the driver's reader keeps a bounded tail of stdout; round 5's 20 KB line came back unparsed


def _sig(x, n=6):
    """floats to n significant digits (the compact line is a record, not a checkpoint); everything else as it is"""
    if isinstance(x, float):
        return float(f"{x:.{n}g}") if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    return x


def _roof_brief(r):
    """the contract's roofline object (bound / achieved / peak / unit / frac / traffic) + which ceiling really binds the kernel:
    `bound` names the roofline the bytes are priced against (the metric is HBM GB/s); `binding` = the ceiling with the larger
    fraction (k_geom_tile: the FP64 vector issue rate, valu_f64), with both fractions side by side"""
    if not r:
        return None
    b = {k: r.get(k) for k in ("kernel", "avg_launch_us", "bound", "achieved", "peak", "unit", "frac", "algorithmic_bytes_per_launch", "traffic")}
    v = r.get("valu_f64")
    if v:
        b["valu_f64_frac"] = v["frac"]
        b["binding"] = "valu_f64" if v["frac"] > (r.get("frac") or 0.0) else r.get("bound")
    else:
        b["binding"] = r.get("bound")
    if r.get("bound") == "hbm":
        b["hbm_frac"] = r.get("frac")
    return b


def _gather_brief(g):
    if not g:
        return None
    acc = g.get("accountings") or {}
    kcg = acc.get("K_cg only (SURVEY 8d)") or {}
    fus = acc.get("fused (this kernel's algorithmic bytes)") or {}
    return {"kernel": g.get("kernel"), "avg_launch_us": g.get("avg_launch_us"), "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac_K_cg": kcg.get("frac"), "achieved_K_cg": kcg.get("achieved_GBps"),
            "frac_fused": fus.get("frac", g.get("frac")), "achieved_fused": fus.get("achieved_GBps", g.get("achieved"))}


def compact_line(out, detail_path=None):
    """The ONE line stdout carries: <= COMPACT_LIMIT bytes, strict JSON (no NaN / Infinity), the contract's keys + roofline +
    cpu_baseline + parity + one short object per measured configuration.  Everything else (per-kernel tables, chains, halo cost,
    phases, the acos census ...) is in the detail document (bench_detail.json; also printed to stderr)."""
    def short(sv, n):
        return sv if sv is None or len(sv) <= n else sv[:n - 3] + "..."
    cfg = out.get("config") or {}
    par = out.get("parity_check")
    cb = out.get("cpu_baseline")
    c = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_cold", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data")}
    c["config"] = {"workload": short(cfg.get("workload"), 330), "name": out.get("workload_name"), "points_per_gpu": cfg.get("points_per_gpu"),
                   "cells_per_gpu": cfg.get("cells_per_gpu"), "parallelism": short(cfg.get("parallelism"), 120)}
    c["roofline"] = _roof_brief(out.get("roofline"))
    c["roofline_centroid_gather"] = _gather_brief(out.get("roofline_centroid_gather"))
    if cb:
        c["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                             "sample": short(cb.get("sample"), 200), "host_cpus": cb.get("host_cpus")}
        c["speedup_vs_cpu_baseline"] = out.get("speedup_vs_cpu_baseline")
    if par:
        sc = par.get("small_case") or {}
        c["parity_check"] = {"ok": bool(par.get("ok", False)), "bitwise_equal": par.get("bitwise_equal", sc.get("bitwise_equal_on_every_rank")),
                             "iters": par.get("iters", sc.get("iters")), "rel_linf": par.get("rel_linf", sc.get("rel_linf_max_over_ranks")),
                             "tolerance": par.get("tolerance", 1e-10), "against": "CPU oracle (unpinned restatement of the reference)"}
    if out.get("rccl"):
        rc = out["rccl"]
        c["rccl"] = {"transport": rc.get("transport"), "backend": short(str(rc.get("backend")), 60), "ranks_seen": rc.get("ranks_seen")}
    for k in ("halo_overhead_us", "weak_efficiency_bound"):
        if k in out:
            c[k] = out[k]
    if out.get("at_100_iters"):
        c["at_100_iters"] = {k: out["at_100_iters"][k] for k in ("steps", "ms_per_step", "value")}
    c["exit_code"] = out.get("exit_code", 0)
    if out.get("failures"):
        c["failures"] = [short(f, 160) for f in out["failures"]][:4]
    c["detail"] = detail_path
    c["configs_summary"] = out.get("configs_summary")
    c = _sig(c)
    line = json.dumps(c, allow_nan=False, separators=(",", ":"))
    # never longer than the limit: drop the optional parts in this order until it fits
    for drop in (("cpu_baseline", "sample"), ("config", "workload"), ("roofline_centroid_gather", None), ("failures", None), ("rccl", None)):
        if len(line.encode()) <= COMPACT_LIMIT:
            break
        if drop[1] is None:
            c.pop(drop[0], None)
        elif isinstance(c.get(drop[0]), dict):
            c[drop[0]][drop[1]] = short(c[drop[0]].get(drop[1]), 60)
        line = json.dumps(c, allow_nan=False, separators=(",", ":"))
    while len(line.encode()) > COMPACT_LIMIT and c.get("configs_summary"):
        c["configs_summary"] = c["configs_summary"][:-1]
        c["configs_summary_truncated"] = True
        line = json.dumps(c, allow_nan=False, separators=(",", ":"))
    return line


def emit(out):
    """the exit path: finalize, write the full document to the detail file (SMOOTHMESH_BENCH_DETAIL, default bench_detail.json
    beside this script; "" = no file) and to stderr, print the ONE compact JSON line on stdout, return the process exit code
    (main() raises SystemExit with it after the process group is gone).  SMOOTHMESH_BENCH_FALSIFY=<workload> flips that entry's
    parity verdict -- the test hook that shows a failed comparison reaches the exit code."""
    fals = os.environ.get("SMOOTHMESH_BENCH_FALSIFY")
    if fals:
        for e in [out] + list(out.get("configs", [])):
            if e.get("workload_name", e.get("workload")) == fals and e.get("parity_check"):
                e["parity_check"]["ok"] = False
                e["parity_check"]["falsified_by_test_hook"] = True
    out, code = finalize_line(out)
    detail = os.environ.get("SMOOTHMESH_BENCH_DETAIL", os.path.join(ROOT, "bench_detail.json"))
    full = json.dumps(_sig(out, 12), allow_nan=False)
    written = None
    if detail:
        try:
            with open(detail, "w") as f:
                f.write(full + "\n")
            written = os.path.relpath(detail, ROOT) if os.path.abspath(detail).startswith(ROOT) else detail
        except OSError as ex:
            print(f"bench.py: could not write {detail}: {ex}", file=sys.stderr)
    if os.environ.get("SMOOTHMESH_BENCH_FULL"):      # the builder's own scripts (scripts/*.sh) read the full document from stdout
        print(full, flush=True)
        return code
    print("BENCH_DETAIL " + full, file=sys.stderr, flush=True)
    print(compact_line(out, written), flush=True)
    return code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="hex100")
    ap.add_argument("--full", action="store_true", help="besides the headline, everything that takes runs of its own: configs[], "
                    "parity_check, cpu_baseline, the per-kernel hipEvent pass (roofline, kernels), at_100_iters, halo_cost")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--configs", default=None, help="with --full: comma-separated workloads reported under \"configs\"; "
                    "default with the default workload: hex100c,cavity215,cavity215c (N = 1), cavity215c (N > 1)")
    ap.add_argument("--no-configs", action="store_true")
    ap.add_argument("--config-steps", type=int, default=0, help="steps of the configs[] sub-runs; 0 = BASELINE.json's counts "
                    "(100 on the hex block, 200 on the polyhedral mesh)")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle legs of the configs[] sub-runs (the 10 M-cell "
                    "oracle costs minutes of host time)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write what the headline's last timed "
                    "step computed to DIR/<name>.npy (float64): points (rank 0's sub-domain when N > 1; a fixed sample past 64 MB), "
                    "residual, nFrozenPoints")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.configs and not args.full:
        ap.error("--configs measures sub-runs of their own: it needs --full")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)            # does not return
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} != WORLD_SIZE {world}")

    import numpy as np
    import torch

    kind, n_side, constraints = parse_workload(args.workload)
    layers = workload_layers(args.workload)
    boundary = workload_boundary(args.workload)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no GPU visible); there is no CPU fallback")
    if os.environ.get("SMOOTHMESH_SHARE_GPU"):      # debugging aid: several ranks on one GPU
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    K, W = args.steps, args.warmup
    n_global = None
    single = multi = None
    multi_subs = []

    # SMOOTHMESH_FORCE_DIST=1: run the N=1 case through the multi-rank code path (host-overhead measurements)
    force_dist = world == 1 and bool(os.environ.get("SMOOTHMESH_FORCE_DIST"))
    if force_dist:
        for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29577")):
            os.environ.setdefault(k, v)
    if world == 1 and not force_dist:
        r = run_single(args.workload, K, W, local_rank, oracle=not args.no_cpu_baseline, nominal100=True,
                       keep_points=args.dump_outputs is not None, full=args.full)
        dt, dt_ev, ctr, sizes, total_points, res, frz = r["dt"], r["dt_ev"], r["ctr"], r["sizes"], r["total_points"], r["res"], r["frz"]
        if args.dump_outputs is not None and rank == 0:
            dump_outputs(args.dump_outputs, r.pop("points"), res, frz)
        pre = r["pre"]
        single = r
        parallelism = "1 GPU"
    else:
        import torch.distributed as dist
        backend = os.environ.get("SMOOTHMESH_BACKEND", "nccl")   # "nccl" is RCCL on ROCm; "gloo" = debug only
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
        r = run_distributed(args.workload, K, W, rank, world, local_rank, backend, oracle=not args.no_cpu_baseline, force_dist=force_dist,
                            keep_points=args.dump_outputs is not None and rank == 0, full=args.full)
        dt, dt_ev, ctr, sizes, total_points, res, frz = r["dt"], r["dt_ev"], r["ctr"], r["sizes"], r["total_points"], r["res"], r["frz"]
        if args.dump_outputs is not None and rank == 0:
            dump_outputs(args.dump_outputs, r.pop("points"), res, frz)
        pre, parallelism, n_global = r["pre"], r["parallelism"], r["n_global"]
        multi = r
        # BASELINE configs[4] beside the weak-scaling headline: the polyhedral mesh, cavity215c per GPU (the 430^3-base, ~80 M-cell
        # mesh on 8 GPUs), constraints on, BASELINE's 200 iterations -- in the same job, every rank taking part
        names = [] if (args.no_configs or force_dist or not args.full) else (args.configs.split(",") if args.configs is not None else
                                                            (["cavity215c"] if args.workload == "hex100" else []))
        multi_subs = []
        for wl in [w for w in names if w]:
            t0 = time.perf_counter()
            k_, _, _ = parse_workload(wl)
            Kc = args.config_steps or (100 if k_ == "hex" else 200)
            rc = run_distributed(wl, Kc, min(W, 5), rank, world, local_rank, backend, oracle=not (args.no_parity or args.no_cpu_baseline),
                                 oracle_budget_s=10.0 if k_ == "hex" else 30.0)
            if rank == 0:
                sub_ = {
                    "workload": wl, "config": workload_text(rc["kind"], rc["n_side"], rc["constraints"], rc["layers"], rc["boundary"], world, rc["n_global"]),
                    "n_gpus": world, "points": int(rc["total_points"]), "points_per_gpu": int(rc["sizes"]["nPoints"]), "cells_per_gpu": int(rc["sizes"]["nCells"]),
                    "steps": Kc, "ms_per_step": rc["dt"] / Kc * 1e3, "value": rc["total_points"] * Kc / rc["dt"], "unit": "points/s",
                    "parallelism": rc["parallelism"], "rccl": rc["transport"],
                    **({"halo_overhead_us": rc["halo_cost"]["halo_overhead_us"], "weak_efficiency_bound": rc["halo_cost"]["weak_efficiency_bound"],
                        "halo_cost": rc["halo_cost"]} if rc["halo_cost"] else {}),
                    **kernel_report(wl, rc["ctr"], Kc, rc["dt"], rc["dt_ev"], rc["sizes"]),
                    "residual_last": float(rc["res"][-1]), "nFrozenPoints_last": int(rc["frz"][-1]), "phases": rc["phases"],
                }
                if rc["parity_check"]:
                    sub_["parity_check"] = rc["parity_check"]
                if rc["cpu_baseline"]:
                    sub_["cpu_baseline"] = rc["cpu_baseline"]
                    sub_["speedup_vs_cpu_baseline"] = sub_["value"] / rc["cpu_baseline"]["value"]
                sub_["wall_s_including_setup"] = time.perf_counter() - t0
                multi_subs.append(sub_)

    if rank != 0:
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return

    out = {
        "metric": "mesh-points smoothed/sec/node (100 iters) + achieved HBM GB/s vs roofline",
        "workload_name": args.workload,
        "value": total_points * K / dt,
        "unit": "points/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": dt / K * 1e3,
        **({"ms_per_step_cold": single["dt_cold"] / K * 1e3} if single else {}),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "pre_run": {"iterations": int(pre), "note": "the workload itself, untimed, before the W warm-up steps (GPU clocks up); "
                    "coordinates reset to the initial ones afterwards; ms_per_step_cold = the same W + K steps timed BEFORE it "
                    "(first launches after set-up, GPU leaving its idle clocks)"},
        "config": {
            "workload": workload_text(kind, n_side, constraints, layers, boundary, world, n_global),
            "points_per_gpu": int(sizes["nPoints"]), "cells_per_gpu": int(sizes["nCells"]),
            "device_bytes_per_gpu": int(sizes["deviceBytes"]),
            "parallelism": parallelism,
        },
        **(kernel_report(args.workload, ctr, K, dt, dt_ev, sizes) if args.full else {}),
        "residual_last": float(res[-1]), "nFrozenPoints_last": int(frz[-1]),
        "parity": "HIP == CPU oracle (tests/); the oracle restates the reference and is unpinned against a real OpenFOAM build",
    }
    if force_dist:
        out["config"]["parallelism"] += " [N=1 forced through the multi-rank path]"
    if multi:
        # how the shared-point records travelled in THIS job: transport (direct = grouped ncclSend / ncclRecv on the engine's stream,
        # torch = all_to_all_single, push = peer stores), the size the communicator itself reports, the start-up self-check
        out["rccl"] = multi["transport"]
        out["phases"] = multi["phases"]
        if multi["halo_cost"]:
            out["halo_overhead_us"] = multi["halo_cost"]["halo_overhead_us"]
            out["weak_efficiency_bound"] = multi["halo_cost"]["weak_efficiency_bound"]
            out["halo_cost"] = multi["halo_cost"]
        if multi["parity_check"]:
            out["parity_check"] = multi["parity_check"]
            out["parity"] = ("parity_check (this job): copies of shared points identical on all ranks after the timed steps + a down-scaled "
                             "case through the same transport against the oracle's MultiDomain; tests/ for the rest; the oracle restates the "
                             "reference and is unpinned against a real OpenFOAM build")
        if multi["cpu_baseline"]:
            out["cpu_baseline"] = multi["cpu_baseline"]
            out["speedup_vs_cpu_baseline"] = out["value"] / multi["cpu_baseline"]["value"]
        if multi_subs:
            out["configs"] = multi_subs
    if world == 1 and not force_dist:
        # BASELINE.json's other single-GPU configurations, measured by this same run (bounded steps)
        names = [] if (args.no_configs or not args.full) else (args.configs.split(",") if args.configs is not None else
                                            (["hex100c", "cavity215", "cavity215c"] if args.workload == "hex100" else []))
        subs = []
        for wl in [w for w in names if w]:
            t0 = time.perf_counter()
            try:
                k_, _, _ = parse_workload(wl)
                Kc = args.config_steps or (100 if k_ == "hex" else 200)
                r = run_single(wl, Kc, min(W, 5), local_rank, oracle=not (args.no_parity or args.no_cpu_baseline),
                               oracle_budget_s=10.0 if k_ == "hex" else 30.0)
                sub = {
                    "workload": wl, "config": workload_text(r["kind"], r["n_side"], r["constraints"], r["layers"], r["boundary"]),
                    "points": int(r["total_points"]), "cells": int(r["sizes"]["nCells"]), "steps": Kc,
                    "ms_per_step": r["dt"] / Kc * 1e3, "ms_per_step_cold": r["dt_cold"] / Kc * 1e3,
                    "value": r["total_points"] * Kc / r["dt"], "unit": "points/s",
                    **kernel_report(wl, r["ctr"], Kc, r["dt"], r["dt_ev"], r["sizes"]),
                    "residual_last": float(r["res"][-1]), "nFrozenPoints_last": int(r["frz"][-1]),
                    "near_ties": r["near_ties"],
                    "phases": r["phases"],
                }
                if r["cpu_baseline"]:
                    sub["cpu_baseline"] = r["cpu_baseline"]
                    sub["speedup_vs_cpu_baseline"] = sub["value"] / r["cpu_baseline"]["value"]
                    sub["parity_check"] = r["parity_check"]
            except Exception as ex:          # a failing sub-run must not take the headline line with it
                sub = {"workload": wl, "error": f"{type(ex).__name__}: {ex}"}
            sub["wall_s_including_setup"] = time.perf_counter() - t0
            subs.append(sub)
        if subs:
            out["configs"] = subs
        if single and single["cpu_baseline"]:
            out["cpu_baseline"] = single["cpu_baseline"]
            out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
            out["parity_check"] = single["parity_check"]
            out["parity"] = ("HIP == CPU oracle: parity_check (this run, this mesh) + tests/; the oracle restates the reference and is "
                             "unpinned against a real OpenFOAM build")
        if single and single.get("dt100"):
            out["at_100_iters"] = {"steps": 100, "ms_per_step": single["dt100"] / 100 * 1e3, "value": total_points * 100 / single["dt100"], "unit": "points/s",
                                   "note": "the metric's nominal iteration count, timed like the K steps, from the initial coordinates"}
        if single:
            out["phases"] = single["phases"]
            if single["near_ties"] is not None:
                out["near_ties"] = single["near_ties"]
    import resource
    out["host_max_rss_gib"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20   # rank 0's process
    code = emit(out)
    if world > 1 or force_dist:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if code:
        raise SystemExit(code)


if __name__ == "__main__":
    main()
