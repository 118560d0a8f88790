// quality_loop.hpp -- the mesh quality features that follow smgpu_iterate (DESIGN.md "Mesh quality", 10.10 - 10.19): the quality
// history, the guard on it, the tangle constraint, the quality constraint (its six setters: qualityConstraintSet; its eight
// getters: qualityConstraintRecords / qualityConstraintState).  Host code; included by smgpu.hip once, inside its extern "C", in front of
// iterateBody, which calls into it.  State: smgpu_handle::qt, qg, tg, qc (quality_state.hpp), numbered by smgpu_handle::iterCount.
// ---- the quality history (kernels_quality_trace.hpp, 10.10) ----
// the running number of the points the engine holds, and how many of the next n iterations are due a record
static int64_t qualityTraceNumber(const smgpu_handle* h) { return h->iterCount - h->qt.since; }
static int qualityTraceDue(const smgpu_handle* h, int n) {
    const int64_t at = qualityTraceNumber(h);
    return (int)((at + n) / h->qt.interval - at / h->qt.interval);
}
// start of a traced smgpu_iterate call: the trace's device memory (on the first one), and a zeroed slab with one record per due
// iteration of the call
static int qualityTraceBegin(smgpu_handle* h, int nIters) {
    if (qualityEnsure(h)) return 1;
    const MeshView& m = h->mv;
    QualityTraceHost& t = h->qt;
    if (!t.block.live()) {
        const size_t nFB = (size_t)std::max(1, qualityGrid(m.nFaces)), nCB = (size_t)std::max(1, qualityGrid(m.nCells));
        const size_t nT = h->useTiles ? (size_t)std::max(1, h->gt.nTiles) : 1;
        if (t.block.alloc(&t.cellCtr, 3 * (size_t)std::max(1, m.nCells)) || t.block.alloc(&t.facePart, nFB) ||
            t.block.alloc(&t.cellPart, std::max(nCB, nT)) || t.block.alloc(&t.cellFold, (size_t)std::max(1, qualityGrid((int)nT))) ||
            t.block.alloc(&t.acc, 1))
            return t.block.failed("the quality trace");
        HIP_OK(hipMemsetAsync(t.acc, 0, sizeof(Accum), h->stream));
    }
    return t.slab.begin(h->stream, qualityTraceDue(h, nIters));
}
// the trace of the points ptsCur now names into the record `out` on the device, behind everything queued on the engine's stream;
// outside the engine's launch counters and timing events, like the report's geometry launch.  The geometry writes the trace's own
// cell centres and tests the trace's own stop word, wantAvg is 0 and no deferred finish rides in it: the loop finds everything it
// reads as it left it.
static int qualityTraceQueue(smgpu_handle* h, int64_t number, const smgpu_iter_stats* gate, smgpu_quality_trace_record* out) {
    const MeshView& m = h->mv;
    State ts = h->st;
    ts.cellCtr = h->qt.cellCtr;
    ts.acc = h->qt.acc;
    ts.stats = nullptr;
    const bool fused = h->qt.fusedWanted && h->useTiles && h->gt.nTiles > 0;
    const int nFB = qualityGrid(m.nFaces);
    int nCB = qualityGrid(m.nCells);
    const QCell* cPart = h->qt.cellPart;
    if (h->useTiles) {
        const int nT = h->gt.nTiles;
        if (nT > 0)
            withGeomTile(h, [&](auto tile, auto org) {
                constexpr int T = decltype(tile)::value;
                constexpr bool ORG = decltype(org)::value;
                if (fused) {
                    ensureDynLds(k_quality_geom_tile<T, ORG>, h->device, h->geomLds);
                    hipLaunchKernelGGL((k_quality_geom_tile<T, ORG>), dim3(tileGrid(nT, h->xcdMap)), dim3(T), (uint32_t)h->geomLds, h->stream, h->mv, ts, h->gv, nT,
                                       h->xcdMap, h->qt.thr, h->qt.cellPart, gate);
                } else {   // the report's geometry launch: writeFaces, no face averages, and the engine's deferred finish is not this launch's to close
                    ensureDynLds(k_geom_tile<T, ORG>, h->device, h->geomLds);
                    hipLaunchKernelGGL((k_geom_tile<T, ORG>), dim3(tileGrid(nT, h->xcdMap)), dim3(T), (uint32_t)h->geomLds, h->stream,
                                       tileLaunch(h->gv.meta, ts, nullptr, nT, h->xcdMap), h->mv, ts, h->gv, 0, 1, 0, 0, (double*)nullptr, (double*)nullptr);
                }
            });
    } else {
        if (m.nFaces > 0) hipLaunchKernelGGL(k_face_geom, dim3(gridFor(m.nFaces)), dim3(kBlock), 0, h->stream, m, ts, 0, h->foamOrg ? 1 : 0);
        if (m.nCells > 0) hipLaunchKernelGGL(k_cell_centres, dim3(gridFor(m.nCells)), dim3(kBlock), 0, h->stream, m, ts, h->foamOrg ? 1 : 0);
    }
    if (nFB > 0)
        hipLaunchKernelGGL(k_quality_faces<false>, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, ts.ptsCur, ts.fCtr, ts.fArea, ts.cellCtr, h->q.own, h->q.nei,
                           QCoupling<false>{}, h->qt.thr, h->qt.facePart, (double*)nullptr, (double*)nullptr);
    if (fused) {
        nCB = qualityGrid(h->gt.nTiles);
        hipLaunchKernelGGL(k_quality_trace_fold, dim3(nCB), dim3(kQualityBlock), 0, h->stream, h->qt.cellPart, h->gt.nTiles, h->qt.cellFold, gate);
        cPart = h->qt.cellFold;
    } else if (nCB > 0) {
        hipLaunchKernelGGL(k_quality_cells, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, ts.fCtr, ts.fArea, h->qt.thr, h->qt.cellPart, (double*)nullptr,
                           (double*)nullptr, (double*)nullptr);
    }
    hipLaunchKernelGGL(k_quality_trace_final, dim3(1), dim3(kQualityBlock), 0, h->stream, h->qt.facePart, nFB, cPart, nCB, m.nCells, m.nFaces, m.nInternalFaces,
                       (long long)number, out, gate);
    HIP_OK(hipGetLastError());
    return 0;
}

static int qualityGuardDisarm(smgpu_handle* h, bool release);
int smgpu_set_quality_trace(smgpu_handle* h, int32_t interval, const smgpu_quality_params* p) {
    if (!h) return fail("null handle");
    if (interval < 0) return fail("smgpu_set_quality_trace: interval < 0");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    HIP_OK(hipSetDevice(h->device));
    if (qualityGuardDisarm(h, true)) return 1;   // the numbering restarts: the guard's iteration numbers would name other points
    h->qt.interval = interval;
    h->qt.since = h->iterCount;
    h->qt.slab.discard();
    h->qt.thr = qualityThresholds(p);
    if (interval == 0) {
        HIP_OK(hipStreamSynchronize(h->stream));
        h->qt.release();
    }
    return 0;
}
int smgpu_get_quality_trace(smgpu_handle* h, smgpu_quality_trace_record* out, int64_t cap, int64_t* n) {
    if (!h || !n) return fail("null argument");
    return h->qt.slab.drain(out, cap, n, "smgpu_get_quality_trace");
}

// ---- the boundary revert switch (DESIGN.md "Mesh quality", 10.21) ----
// The opt-in under which the serial tangle constraint, the serial quality constraint and the guard accept an engine with boundary
// point smoothing.  It is a decision about the contract, not a mode of the loop: the loop launches what it launches without it.
int smgpu_set_boundary_revert(smgpu_handle* h, int32_t on) {
    if (!h) return fail("null handle");
    if (h->haloOn) return fail("smgpu_set_boundary_revert: not available on an engine with a halo (the coupled constraints refuse boundary point smoothing)");
    if (!on && h->bndOn && (h->tg.on || h->qc.on || h->qg.armed))
        return fail(std::string("smgpu_set_boundary_revert: ") + (h->tg.on ? "the tangle constraint is on" : h->qc.on ? "the quality constraint is on" : "the quality guard is armed") +
                    " over boundary point smoothing, which only the switch allows; switch that off first");
    h->bndRevert = on != 0;
    return 0;
}
int smgpu_get_boundary_revert(smgpu_handle* h, int32_t* on) {
    if (!h || !on) return fail("null argument");
    *on = h->bndRevert ? 1 : 0;
    return 0;
}

// ---- the guard on the quality history (kernels_quality_guard.hpp, DESIGN.md "Mesh quality", 10.11) ----
static int qualityGuardDisarm(smgpu_handle* h, bool release) {
    h->qg.armed = false;
    h->qg.tripPending = false;
    h->qg.state.armed = 0;
    if (release && h->qg.block.live()) {
        HIP_OK(hipStreamSynchronize(h->stream));
        h->qg.release();
    }
    return 0;
}
// the per-point state an iteration carries to the next (State's non-const pointers that an iteration reads before it writes them:
// ptsCur, and layerNormal with layers or with boundary point smoothing, whose k_bnd_normals blends it once per iteration) between
// the engine and the snapshot, on the engine's stream.  Of BndView's non-const members flags (BF_SHARP), featSum and featCnt are
// written by every iteration before it reads them (10.21).
static bool guardCarriesNormals(const smgpu_handle* h) { return (h->layersOn || h->bndOn) && h->st.layerNormal; }
static int qualityGuardCopy(smgpu_handle* h, bool restore, int64_t number, bool needGood) {
    const long long n = 3 * (long long)h->mv.nPoints;
    const bool normals = guardCarriesNormals(h) && h->qg.normal;
    const double *s0 = restore ? h->qg.pts : h->st.ptsCur, *s1 = normals ? (restore ? h->qg.normal : h->st.layerNormal) : nullptr;
    double *d0 = restore ? h->st.ptsCur : h->qg.pts, *d1 = normals ? (restore ? h->st.layerNormal : h->qg.normal) : nullptr;
    const int grid = (int)std::max<long long>(1, ((n >> 1) + (long long)kGuardBlock * kGuardPer - 1) / ((long long)kGuardBlock * kGuardPer));
    if (normals) hipLaunchKernelGGL(k_quality_guard_snapshot<true>, dim3(grid), dim3(kGuardBlock), 0, h->stream, s0, d0, s1, d1, n, (long long)number, h->qg.dev, needGood ? 1 : 0);
    else hipLaunchKernelGGL(k_quality_guard_snapshot<false>, dim3(grid), dim3(kGuardBlock), 0, h->stream, s0, d0, s1, d1, n, (long long)number, h->qg.dev, needGood ? 1 : 0);
    HIP_OK(hipGetLastError());
    if (restore) { h->q.epoch++; h->geomAheadDone = false; }
    return 0;
}
// behind k_quality_trace_final of a traced iteration: the verdict on its record, then the snapshot if it passed
static int qualityGuardQueue(smgpu_handle* h, const smgpu_quality_trace_record* rec, int64_t number, const smgpu_iter_stats* gate) {
    hipLaunchKernelGGL(k_quality_guard_verdict, dim3(1), dim3(64), 0, h->stream, rec, h->qg.dev, (unsigned)h->qg.prm.criteria, &h->st.acc->stop, gate);
    HIP_OK(hipGetLastError());
    return qualityGuardCopy(h, false, number, true);
}
// After the read-back of a call that tripped: back to the snapshot; with `refine`, on from it one iteration at a time, a trace and
// a verdict behind each, until one fails or interval - 1 have passed (the loop is deterministic from the snapshot's state, so
// these are the iterations of the call over again).  The steps go through smgpu_iterate's body with the trace at interval 1;
// what they would leave behind -- launch counts, timing events, the near-tie census, trace records -- is put back or not kept.
// The engine's iteration count goes back to the restored iteration, and every running number with it.
static int qualityGuardAfterTrip(smgpu_handle* h) {
    h->qg.tripPending = false;
    if (qualityGuardCopy(h, true, -1, false)) return 1;
    int64_t good = h->qg.state.snapshotIteration;
    const int interval = h->qt.interval;
    int rc = 0;
    if (h->qg.prm.refine && interval > 1) {
        Uncounted scope(h);
        unsigned long long nearSaved[3] = {0, 0, 0};
        if (h->st.nearTotal) HIP_OK(hipMemcpyAsync(nearSaved, h->st.nearTotal, sizeof(nearSaved), hipMemcpyDeviceToHost, h->stream));
        HIP_OK(hipMemsetAsync(&h->qg.dev->tripped, 0, sizeof(int), h->stream));
        HIP_OK(hipStreamSynchronize(h->stream));
        h->qg.refining = true;
        h->qt.interval = 1;
        for (int step = 1; step < interval && !rc; ++step) {
            h->iterCount = h->qt.since + good;
            int32_t done = 0;
            rc = iterateBody(h, 1, 0.0, nullptr, &done);
            if (rc) break;
            if (done != 1 || h->qg.lastVerdict != kGuardGood) {   // the first bad step: the snapshot is the state before it
                rc = qualityGuardCopy(h, true, -1, false);
                break;
            }
            ++good;
        }
        h->qt.interval = interval;
        h->qg.refining = false;
        if (!rc && h->st.nearTotal) HIP_OK(hipMemcpyAsync(h->st.nearTotal, nearSaved, sizeof(nearSaved), hipMemcpyHostToDevice, h->stream));
        HIP_OK(hipStreamSynchronize(h->stream));
        if (rc) return 1;
    }
    h->qg.state.snapshotIteration = good;
    h->qg.state.restoredIteration = good;
    h->iterCount = h->qt.since + good;
    return qualityGuardDisarm(h, false);
}

int smgpu_set_quality_guard(smgpu_handle* h, const smgpu_quality_guard_params* p, int32_t on) {
    if (!h) return fail("null handle");
    HIP_OK(hipSetDevice(h->device));
    if (!on) return qualityGuardDisarm(h, true);
    const smgpu_quality_guard_params prm = p ? *p : smgpu_quality_guard_params{SMGPU_GUARD_NONPOSITIVE_VOLUME | SMGPU_GUARD_WRONG_ORIENTED, 1};
    const uint32_t all = SMGPU_GUARD_NONPOSITIVE_VOLUME | SMGPU_GUARD_WRONG_ORIENTED | SMGPU_GUARD_ERROR_NONORTH;
    if (prm.criteria == 0 || (prm.criteria & ~all)) return fail("smgpu_set_quality_guard: criteria must be a non-empty combination of SMGPU_GUARD_NONPOSITIVE_VOLUME, _WRONG_ORIENTED and _ERROR_NONORTH");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    if (h->bndOn && !h->bndRevert)
        return fail("smgpu_set_quality_guard: not available on an engine with boundary point smoothing (its point normals are a running blend across the "
                    "iterations and its corner lists are host state, neither of which the guard's snapshot holds)");
    if (h->qt.interval <= 0) return fail("smgpu_set_quality_guard: the guard judges the records of the quality trace; switch it on first (smgpu_set_quality_trace)");
    if (h->iterOpen) return fail("smgpu_set_quality_guard: between smgpu_iter_begin and smgpu_iter_end");
    if (qualityGuardDisarm(h, true)) return 1;
    if (flushDeferred(h)) return 1;
    if (qualityTraceBegin(h, 0)) return 1;
    QualityGuardHost& g = h->qg;
    const size_t n = 3 * (size_t)std::max(1, h->mv.nPoints);
    if (g.block.alloc(&g.dev, 1) || g.block.alloc(&g.rec, 1) || g.block.alloc(&g.pts, n) ||
        (guardCarriesNormals(h) && g.block.alloc(&g.normal, n)))
        return g.block.failed("the quality guard");
    HIP_OK(hipMemsetAsync(h->qg.dev, 0, sizeof(GuardDev), h->stream));
    HIP_OK(hipMemsetAsync(h->qg.rec, 0, sizeof(smgpu_quality_trace_record), h->stream));
    // the baseline: the trace's launches on the current points, number 0
    if (qualityTraceQueue(h, 0, nullptr, h->qg.rec)) { h->qg.release(); return 1; }
    HIP_OK(hipMemcpyAsync(&h->qg.dev->baseline, h->qg.rec, sizeof(smgpu_quality_trace_record), hipMemcpyDeviceToDevice, h->stream));
    h->qg.prm = prm;
    h->qg.state = smgpu_quality_guard_state{};
    if (qualityGuardCopy(h, false, qualityTraceNumber(h), false)) { h->qg.release(); return 1; }
    HIP_OK(hipMemcpyAsync(&h->qg.state.baseline, h->qg.rec, sizeof(smgpu_quality_trace_record), hipMemcpyDeviceToHost, h->stream));
    if (checkDeviceError(h)) { h->qg.release(); return 1; }
    h->qg.state.armed = 1;
    h->qg.state.snapshotIteration = qualityTraceNumber(h);
    h->qg.armed = true;
    return 0;
}
int smgpu_get_quality_guard(smgpu_handle* h, smgpu_quality_guard_state* out) {
    if (!h || !out) return fail("null argument");
    *out = h->qg.state;
    return 0;
}
int smgpu_quality_guard_restore(smgpu_handle* h) {
    if (!h) return fail("null handle");
    if (!h->qg.armed) return fail("smgpu_quality_guard_restore: the quality guard is not armed (smgpu_set_quality_guard)");
    HIP_OK(hipSetDevice(h->device));
    if (flushDeferred(h)) return 1;
    if (qualityGuardCopy(h, true, -1, false)) return 1;
    if (checkDeviceError(h)) return 1;
    h->qg.state.restoredIteration = h->qg.state.snapshotIteration;
    h->iterCount = h->qt.since + h->qg.state.snapshotIteration;   // every running number names the same points
    return 0;
}

// ---- the tangle constraint (kernels_quality_tangle.hpp, DESIGN.md "Mesh quality", 10.12, 10.13) ----
static int tangleOff(smgpu_handle* h) {
    h->tg.on = false;
    h->tg.slab.discard();
    if (h->tg.block.live()) {
        HIP_OK(hipStreamSynchronize(h->stream));
        h->tg.release();
    }
    return 0;
}
// one evaluation of the points ptsCur names, behind everything queued on the engine's stream; outside the launch counters and
// the timing events.  Tiles: nothing the loop reads is written.  Without tiles the direct geometry kernels write the loop's face
// values (the next geometry launch writes them again before anything reads them), cell centres of the constraint's own, and
// test a stop word of its own.
static int tangleEvaluate(smgpu_handle* h, uint8_t* exemptOut, int pass, const smgpu_iter_stats* gate) {
    const MeshView& m = h->mv;
    State ts = h->st;
    ts.stats = nullptr;
    if (h->useTiles) {
        const int nT = h->gt.nTiles;
        if (nT > 0)
            withGeomTile(h, [&](auto tile, auto org) {
                constexpr int T = decltype(tile)::value;
                constexpr bool ORG = decltype(org)::value;
                ensureDynLds(k_tangle_tile<T, ORG>, h->device, h->geomLds);
                hipLaunchKernelGGL((k_tangle_tile<T, ORG>), dim3(tileGrid(nT, h->xcdMap)), dim3(T), (uint32_t)h->geomLds, h->stream, h->mv, ts, h->gv, nT, h->xcdMap,
                                   exemptOut ? (const uint8_t*)nullptr : (const uint8_t*)h->tg.exempt, exemptOut, h->tg.marks, h->tg.dev, pass, gate);
            });
    } else {
        ts.cellCtr = h->tg.cellCtr;
        ts.acc = h->tg.acc;
        if (m.nFaces > 0) hipLaunchKernelGGL(k_face_geom, dim3(gridFor(m.nFaces)), dim3(kBlock), 0, h->stream, m, ts, 0, h->foamOrg ? 1 : 0);
        if (m.nCells > 0) {
            hipLaunchKernelGGL(k_cell_centres, dim3(gridFor(m.nCells)), dim3(kBlock), 0, h->stream, m, ts, h->foamOrg ? 1 : 0);
            hipLaunchKernelGGL(k_tangle_cells, dim3((m.nCells + kTangleBlock - 1) / kTangleBlock), dim3(kTangleBlock), 0, h->stream, m, ts.fCtr, ts.fArea,
                               ts.cellCtr, exemptOut ? (const uint8_t*)nullptr : (const uint8_t*)h->tg.exempt, exemptOut, h->tg.marks, h->tg.dev, pass, gate);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}
// behind the movePoints of an iteration: the passes on the points ptsCur now names; x: the points the iteration started from
static int tangleQueue(smgpu_handle* h, int slot, int64_t number, const smgpu_iter_stats* gate, const double* x) {
    smgpu_tangle_record* rec = nullptr;
    if (h->tg.slab.slot(slot, &rec)) return 1;
    const int nP = h->mv.nPoints;
    const int gApply = std::max(1, (int)(((int64_t)nP + kTanglePts - 1) / kTanglePts));
    for (int k = 0; k <= h->tg.passes; ++k) {
        if (tangleEvaluate(h, nullptr, k, gate)) return 1;
        hipLaunchKernelGGL(k_tangle_verdict, dim3(1), dim3(64), 0, h->stream, h->tg.dev, rec, (long long)number, k, h->tg.passes, gate);
        hipLaunchKernelGGL(k_tangle_apply, dim3(gApply), dim3(kTangleBlock), 0, h->stream, x, h->st.ptsCur, h->tg.marks, nP, (const TangleDev*)h->tg.dev, rec, gate);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int smgpu_set_tangle_constraint(smgpu_handle* h, const smgpu_tangle_params* p, int32_t on) {
    if (!h) return fail("null handle");
    HIP_OK(hipSetDevice(h->device));
    if (!on) return tangleOff(h);
    const smgpu_tangle_params prm = p ? *p : smgpu_tangle_params{2};
    if (prm.passes < 0) return fail("smgpu_set_tangle_constraint: passes < 0");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    if (h->bndOn && !h->bndRevert)
        return fail("smgpu_set_tangle_constraint: not available on an engine with boundary point smoothing (it rewrites the proposals of the boundary "
                    "points from state that a reverted iteration would leave ahead of the points)");
    if (h->qc.on) return fail("smgpu_set_tangle_constraint: the quality constraint is on (smgpu_set_quality_constraint), and it contains this one; switch it off first");
    if (h->iterOpen) return fail("smgpu_set_tangle_constraint: between smgpu_iter_begin and smgpu_iter_end");
    if (tangleOff(h)) return 1;
    if (flushDeferred(h)) return 1;
    const MeshView& m = h->mv;
    const size_t nMark = ((size_t)std::max(1, m.nPoints) + 3) & ~(size_t)3, nCell = (size_t)std::max(1, m.nCells);
    TangleHost& t = h->tg;
    if (t.block.alloc(&t.dev, 1) || t.block.alloc(&t.exempt, nCell) || t.block.alloc(&t.marks, nMark) ||
        (!h->useTiles && (t.block.alloc(&t.cellCtr, 3 * nCell) || t.block.alloc(&t.acc, 1))))
        return t.block.failed("the tangle constraint");
    HIP_OK(hipMemsetAsync(h->tg.dev, 0, sizeof(TangleDev), h->stream));
    HIP_OK(hipMemsetAsync(h->tg.exempt, 0, nCell, h->stream));
    HIP_OK(hipMemsetAsync(h->tg.marks, 0, nMark, h->stream));
    if (h->tg.acc) HIP_OK(hipMemsetAsync(h->tg.acc, 0, sizeof(Accum), h->stream));
    // the exempt cells: one evaluation of the current points
    h->tg.passes = prm.passes;
    if (tangleEvaluate(h, h->tg.exempt, 0, nullptr)) { h->tg.release(); return 1; }
    TangleDev td{};
    HIP_OK(hipMemcpyAsync(&td, h->tg.dev, sizeof(TangleDev), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemsetAsync(h->tg.dev, 0, sizeof(TangleDev), h->stream));
    if (checkDeviceError(h)) { h->tg.release(); return 1; }
    h->tg.nExempt = td.badNow;
    h->tg.since = h->iterCount;
    h->tg.on = true;
    return 0;
}
static int tangleCoupledFlush(smgpu_handle* h);
int smgpu_get_tangle_records(smgpu_handle* h, smgpu_tangle_record* out, int64_t cap, int64_t* n) {
    if (!h || !n) return fail("null argument");
    if (h->tg.coupled) {   // the records of the chunk in use are still on the device
        if (h->tg.k >= 0) return fail("smgpu_get_tangle_records: between the passes of an iteration (smgpu_tangle_pass_begin / _end)");
        HIP_OK(hipSetDevice(h->device));
        if (tangleCoupledFlush(h)) return 1;
    }
    return h->tg.slab.drain(out, cap, n, "smgpu_get_tangle_records");
}
int smgpu_get_tangle_state(smgpu_handle* h, smgpu_tangle_state* out) {
    if (!h || !out) return fail("null argument");
    const int64_t number = h->tg.coupled ? h->tg.count : h->iterCount - h->tg.since;
    *out = smgpu_tangle_state{h->tg.on ? 1 : 0, h->tg.passes, h->tg.on ? h->tg.nExempt : 0, h->tg.on ? number : 0};
    return 0;
}

// ---- the coupled form on an engine with a halo (DESIGN.md "Mesh quality", 10.13) ----
// The passes are the host's calls behind smgpu_iter_end: every kernel below goes onto the engine's stream, behind the
// iteration's own.  x, the points the iteration started from, is the buffer smgpu_iter_end swapped out; the next launch that
// writes it is the next iteration's smoothing kernel, queued on the same stream behind the passes.
static int computeAfterExch(smgpu_handle* h);
// the records written in the chunk in use become pending; the next iteration starts a zeroed chunk
static int tangleCoupledFlush(smgpu_handle* h) {
    TangleHost& t = h->tg;
    if (t.slabUsed > 0) {
        if (t.slab.readBack(h->stream, t.slabUsed)) return 1;
        HIP_OK(hipStreamSynchronize(h->stream));
        t.slab.keep(t.slabUsed);
    }
    t.slabUsed = 0;
    t.slabFresh = false;
    return 0;
}
int smgpu_set_tangle_constraint_coupled(smgpu_handle* h, const smgpu_tangle_params* p, const smgpu_tangle_halo_desc* d, int32_t on) {
    if (!h) return fail("null handle");
    HIP_OK(hipSetDevice(h->device));
    if (!on) return tangleOff(h);
    const smgpu_tangle_params prm = p ? *p : smgpu_tangle_params{2};
    if (prm.passes < 0) return fail("smgpu_set_tangle_constraint_coupled: passes < 0");
    if (!h->haloOn)
        return fail("smgpu_set_tangle_constraint_coupled: the engine has no halo (smgpu_halo_configure); a serial engine takes smgpu_set_tangle_constraint");
    if (h->bndOn)
        return fail("smgpu_set_tangle_constraint_coupled: not available on an engine with boundary point smoothing (it rewrites the proposals of the "
                    "boundary points from state that a reverted iteration would leave ahead of the points)");
    if (h->qc.on) return fail("smgpu_set_tangle_constraint_coupled: the quality constraint is on (smgpu_set_quality_constraint_coupled), and it contains this one; switch it off first");
    if (h->iterOpen) return fail("smgpu_set_tangle_constraint_coupled: between smgpu_iter_begin and smgpu_iter_end");
    if (!d || (h->nSend && !d->sendT) || (h->nRecv && !d->recvT)) return fail("smgpu_set_tangle_constraint_coupled: null exchange buffer");
    if (tangleOff(h)) return 1;
    if (flushDeferred(h)) return 1;
    const MeshView& m = h->mv;
    const size_t nMark = ((size_t)std::max(1, m.nPoints) + 3) & ~(size_t)3, nCell = (size_t)std::max(1, m.nCells);
    TangleHost& t = h->tg;
    if (t.block.alloc(&t.dev, 1) || t.block.alloc(&t.exempt, nCell) || t.block.alloc(&t.marks, nMark) ||
        t.block.alloc(&t.counted, (size_t)std::max(1, h->nShared)) ||
        (!h->useTiles && (t.block.alloc(&t.cellCtr, 3 * nCell) || t.block.alloc(&t.acc, 1))))
        return t.block.failed("the tangle constraint");
    HIP_OK(hipMemsetAsync(t.dev, 0, sizeof(TangleDev), h->stream));
    HIP_OK(hipMemsetAsync(t.exempt, 0, nCell, h->stream));
    HIP_OK(hipMemsetAsync(t.marks, 0, nMark, h->stream));
    if (t.acc) HIP_OK(hipMemsetAsync(t.acc, 0, sizeof(Accum), h->stream));
    if (h->nShared > 0) HIP_OK(hipMemcpyAsync(t.counted, h->sharedMasterHost.data(), (size_t)h->nShared, hipMemcpyHostToDevice, h->stream));
    // the exempt cells: one evaluation of the current points (copies of a shared point are identical: the global mesh's answer)
    t.passes = prm.passes;
    if (tangleEvaluate(h, t.exempt, 0, nullptr)) { t.release(); return 1; }
    TangleDev td{};
    HIP_OK(hipMemcpyAsync(&td, t.dev, sizeof(TangleDev), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemsetAsync(t.dev, 0, sizeof(TangleDev), h->stream));
    if (checkDeviceError(h)) { t.release(); return 1; }
    t.nExempt = td.badNow;
    t.sendT = (int*)d->sendT; t.recvT = (int*)d->recvT;
    t.count = 0;
    t.k = -1;
    t.coupled = true;
    t.on = true;
    return 0;
}
// behind smgpu_iter_end: the iteration waits for its passes
static void tangleCoupledIterEnd(smgpu_handle* h, const double* x) {
    h->tg.x = x;
    h->tg.k = 0;
    h->tg.reverting = 0;
    h->tg.passOpen = false;
}
int smgpu_tangle_pass_begin(smgpu_handle* h, int64_t* nBadLocal) {
    if (!h || !nBadLocal) return fail("null argument");
    TangleHost& t = h->tg;
    if (!t.coupled) return fail("smgpu_tangle_pass_begin: the coupled tangle constraint is not on (smgpu_set_tangle_constraint_coupled)");
    if (h->iterOpen) return fail("smgpu_tangle_pass_begin: between smgpu_iter_begin and smgpu_iter_end");
    if (t.k < 0) return fail("smgpu_tangle_pass_begin: no iteration waits for its passes (the passes follow smgpu_iter_end)");
    if (t.passOpen) return fail("smgpu_tangle_pass_begin: the pass in hand has not been closed (smgpu_tangle_pass_end)");
    HIP_OK(hipSetDevice(h->device));
    if (t.k == 0 && (!t.slabFresh || t.slabUsed >= TangleHost::kChunk)) {
        if (tangleCoupledFlush(h)) return 1;
        if (t.slab.begin(h->stream, TangleHost::kChunk)) return 1;
        t.slabFresh = true;
    }
    if (tangleEvaluate(h, nullptr, 0, nullptr)) return 1;
    if (h->nSend > 0)
        hipLaunchKernelGGL(k_tangle_pack, dim3((h->nSend + kTangleBlock - 1) / kTangleBlock), dim3(kTangleBlock), 0, h->stream, h->nSend, (const int*)h->dSendShared,
                           (const int*)h->dSharedLocal, (const uint8_t*)t.marks, t.sendT);
    HIP_OK(hipGetLastError());
    // the one host read of the pass; it also waits for sendT, so whichever stream the host moves T on is ordered behind the pack
    TangleDev td{};
    HIP_OK(hipMemcpyAsync(&td, t.dev, sizeof(TangleDev), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemsetAsync(t.dev, 0, sizeof(TangleDev), h->stream));
    if (checkDeviceError(h)) return 1;
    if (td.err) return fail("smgpu_tangle_pass_begin: the marks of a geometry tile do not fit the LDS of its points");
    if (t.k == 0) t.nBad0 = td.badNow;
    t.passOpen = true;
    *nBadLocal = td.badNow;
    return 0;
}
// The revert of a pass that found bad cells somewhere, for the two coupled constraints: unless the revert is the full one, the
// marks the other ranks sent for the shared points (recvT) join this rank's and the pass counts as a reverting one; then the marked
// points -- all of them when full -- go back to x.  rec: the iteration's record, whose head is the tangle constraint's.
static int coupledRevert(smgpu_handle* h, bool full, const int* recvT, uint8_t* marks, const double* x, const uint8_t* counted, smgpu_tangle_record* rec,
                         int& reverting) {
    const int nP = h->mv.nPoints;
    if (!full) {
        if (computeAfterExch(h)) return 1;      // exchange T has been enqueued by the host
        if (h->nShared > 0 && h->nRecv > 0)
            hipLaunchKernelGGL(k_tangle_combine, dim3((h->nShared + kTangleBlock - 1) / kTangleBlock), dim3(kTangleBlock), 0, h->stream, h->nShared,
                               (const int*)h->dSharedLocal, (const int*)h->dCombOff, (const int*)h->dCombSlots, recvT, marks);
        ++reverting;
    }
    const int grid = std::max(1, (int)(((int64_t)nP + kTangleCountedPts - 1) / kTangleCountedPts));
    hipLaunchKernelGGL(k_tangle_apply_counted, dim3(grid), dim3(kTangleBlock), 0, h->stream, x, h->st.ptsCur, marks, nP, full ? 1 : 0, (const int*)h->dSharedSlot,
                       counted, rec);
    // points went back: the geometry smgpu_iter_ahead left for the next iteration is that of other points
    h->geomAheadDone = false;
    h->q.epoch++;
    return 0;
}
int smgpu_tangle_pass_end(smgpu_handle* h, int64_t nBadGlobal, int32_t* done) {
    if (!h || !done) return fail("null argument");
    TangleHost& t = h->tg;
    if (!t.coupled) return fail("smgpu_tangle_pass_end: the coupled tangle constraint is not on (smgpu_set_tangle_constraint_coupled)");
    if (!t.passOpen || t.k < 0) return fail("smgpu_tangle_pass_end without smgpu_tangle_pass_begin");
    if (nBadGlobal < 0) return fail("smgpu_tangle_pass_end: nBadGlobal < 0");
    HIP_OK(hipSetDevice(h->device));
    smgpu_tangle_record* rec = nullptr;
    if (t.slab.slot(t.slabUsed, &rec)) return 1;
    const bool full = nBadGlobal > 0 && t.k == t.passes;
    if (nBadGlobal > 0 && coupledRevert(h, full, t.recvT, t.marks, t.x, t.counted, rec, t.reverting)) return 1;
    const bool close = nBadGlobal == 0 || full;
    if (close) {
        hipLaunchKernelGGL(k_tangle_close, dim3(1), dim3(64), 0, h->stream, rec, (long long)(t.count + 1), t.reverting, full ? 1 : 0, (long long)t.nBad0);
        ++t.count;
        ++t.slabUsed;
        t.k = -1;
    } else ++t.k;
    t.passOpen = false;
    *done = close ? 1 : 0;
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- the quality constraint (kernels_quality_constraint.hpp, DESIGN.md "Mesh quality", 10.14) ----
// NULL limits of every entry (the narrower entries' defaults are its heads), and the limits of 10.16 as the kernels take them:
// which criteria a set of limits switches on
static const smgpu_quality_constraint_limits_all kQcLimitsDefault{65.0, 4.0, 20.0, 2, -1e30, -1.0, -1.0, 0.0, 0.0, 0.0, 180.0, 0.0, 0.0, 0.0};
static QcMore qualityConstraintMore(const smgpu_quality_constraint_limits_all& l) {
    return QcMore{l.minTetQuality, l.minTwist, l.minTriangleTwist, l.minFaceWeight, l.minVolRatio, l.minDeterminant, motionThresholds(nullptr).k,
                  l.minTetQuality > -1e30 ? 1 : 0, l.minTwist > -1.0 ? 1 : 0, l.minTriangleTwist > -1.0 ? 1 : 0,
                  l.minFaceWeight > 0.0 ? 1 : 0, l.minVolRatio > 0.0 ? 1 : 0, l.minDeterminant > 0.0 ? 1 : 0};
}
// the limits of 10.18 as the kernels take them, and maxConcave as given (the state's); sinConcave exactly as
// qualityGeomThresholds() (quality_reports.hpp) forms the geometry report's sine
struct QcShapeLimits { QcShape k; double maxConcave; };
static QcShapeLimits qualityConstraintShape(const smgpu_quality_constraint_limits_all& l) {
    return QcShapeLimits{QcShape{std::sin(l.maxConcave * (SMGPU_PI / 180.0)), l.minFlatness, l.minArea, l.minVol, l.maxConcave < 180.0 ? 1 : 0, l.minFlatness > 0.0 ? 1 : 0,
                                 l.minArea > 0.0 ? 1 : 0, l.minVol > 0.0 ? 1 : 0},
                         l.maxConcave};
}
static const QcShapeLimits kQcShapeOff = qualityConstraintShape(kQcLimitsDefault);
static int qualityConstraintOff(smgpu_handle* h) {
    h->qc.on = false;
    h->qc.more = qualityConstraintMore(kQcLimitsDefault);
    h->qc.shape = kQcShapeOff.k;
    h->qc.maxConcave = kQcShapeOff.maxConcave;
    h->qc.faceMore = h->qc.cellMore = false;
    h->qc.nExemptDet = h->qc.nExemptVol = 0;
    h->qc.slab.discard();
    if (h->qc.block.live()) {
        HIP_OK(hipStreamSynchronize(h->stream));
        h->qc.release();
    }
    return 0;
}
// One evaluation of the points ptsCur names, behind everything queued on the engine's stream; outside the launch counters and the
// timing events.  It has two halves, which the serial form queues back to back (qualityConstraintEvaluate) and the coupled form
// on either side of the host's move of the cell centres (qualityConstraintCoupledGeometry / _Verdicts, ungated: pass = 0, gate =
// NULL).  enabling: the verdicts become the exempt bytes.  The kernels take the form as their coupling argument:
extern "C++" {
template <class Fn>
static void withQcCoupling(const QualityConstraintHost& q, Fn fn) {
    if (q.coupled) fn(std::true_type{}, QCoupling<true>{q.slot, q.recvCc, q.recvVc});
    else fn(std::false_type{}, QCoupling<false>{});
}
// the instantiations of kernels_quality_limits.hpp's two kernels a set of limits takes
template <bool C, bool Vol>
static auto qcCellsMoreOf(bool det) { return det ? k_qc_cells_more<true, C, Vol> : k_qc_cells_more<false, C, Vol>; }
template <bool C, int Shape>
static auto qcFacesMoreOf(bool walk, bool ratio) {
    return walk ? (ratio ? k_qc_faces_more<true, true, C, Shape> : k_qc_faces_more<true, false, C, Shape>)
                : (ratio ? k_qc_faces_more<false, true, C, Shape> : k_qc_faces_more<false, false, C, Shape>);
}
}
// The geometry half.  Tiles: k_qc_tile writes fCtr / fArea, which no kernel of the tiled loop reads, and cell centres of the
// constraint's own.  Without tiles the direct geometry kernels write the loop's face values (the next geometry launch writes them
// again before anything reads them), the same cell centres, and test a stop word of the constraint's own, which k_qc_open sets
// in front of pass 0 -- in the coupled form in front of every evaluation.  Then 10.16's cell pass (kernels_quality_limits.hpp), in
// front of the faces, which read its volumes: coupled, the volumes travel with the cell centres, and the byte the pass leaves in
// cellFlag and its count in QcDev wait for the second half.
static int qualityConstraintGeometry(smgpu_handle* h, bool enabling, int pass, const smgpu_iter_stats* gate) {
    const MeshView& m = h->mv;
    QualityConstraintHost& q = h->qc;
    State ts = h->st;
    ts.cellCtr = q.cellCtr;
    ts.acc = q.acc;
    ts.stats = nullptr;
    if (h->useTiles) {
        const int nT = h->gt.nTiles;
        if (nT > 0)
            withGeomTile(h, [&](auto tile, auto org) {
                constexpr int T = decltype(tile)::value;
                constexpr bool ORG = decltype(org)::value;
                ensureDynLds(k_qc_tile<T, ORG>, h->device, h->geomLds);
                hipLaunchKernelGGL((k_qc_tile<T, ORG>), dim3(tileGrid(nT, h->xcdMap)), dim3(T), (uint32_t)h->geomLds, h->stream, h->mv, ts, h->gv, nT, h->xcdMap,
                                   enabling ? (const uint8_t*)nullptr : (const uint8_t*)q.exemptCell, enabling ? q.exemptCell : (uint8_t*)nullptr, q.tangled, q.dev,
                                   pass, gate);
            });
    } else {
        if (pass == 0) hipLaunchKernelGGL(k_qc_open, dim3(1), dim3(64), 0, h->stream, q.acc, gate);
        if (m.nFaces > 0) hipLaunchKernelGGL(k_face_geom, dim3(gridFor(m.nFaces)), dim3(kBlock), 0, h->stream, m, ts, 0, h->foamOrg ? 1 : 0);
        if (m.nCells > 0) hipLaunchKernelGGL(k_cell_centres, dim3(gridFor(m.nCells)), dim3(kBlock), 0, h->stream, m, ts, h->foamOrg ? 1 : 0);
    }
    if (q.cellMore && m.nCells > 0)
        withQcCoupling(q, [&](auto coupled, auto cp) {
            constexpr bool C = decltype(coupled)::value;
            auto cells = q.shape.volOn ? qcCellsMoreOf<C, true>(q.more.detOn != 0) : qcCellsMoreOf<C, false>(q.more.detOn != 0);
            hipLaunchKernelGGL(cells, dim3((m.nCells + kQcBlock - 1) / kQcBlock), dim3(kQcBlock), 0, h->stream, m, (const double*)ts.fCtr, (const double*)ts.fArea, cp,
                               q.more, q.shape, q.vol, enabling ? (const uint8_t*)nullptr : (const uint8_t*)q.exemptDet, enabling ? q.exemptDet : (uint8_t*)nullptr, q.cellFlag,
                               q.dev, pass, gate);
        });
    HIP_OK(hipGetLastError());
    return 0;
}
// The verdict half: the faces -- 10.16's wider pass when one of its face criteria is on -- then the cells
static int qualityConstraintVerdicts(smgpu_handle* h, bool enabling, int pass, const smgpu_iter_stats* gate) {
    const MeshView& m = h->mv;
    QualityConstraintHost& q = h->qc;
    const double *fCtr = h->st.fCtr, *fArea = h->st.fArea, *pts = h->st.ptsCur, *cellCtr = q.cellCtr;
    const uint8_t* exemptFace = enabling ? nullptr : q.exemptFace;
    uint8_t* exemptFaceOut = enabling ? q.exemptFace : nullptr;
    if (m.nFaces > 0)
        withQcCoupling(q, [&](auto coupled, auto cp) {
            constexpr bool C = decltype(coupled)::value;
            const dim3 grid((m.nFaces + kQcBlock - 1) / kQcBlock);
            if (q.faceMore) {
                const bool walk = q.more.tetOn || q.more.twistOn || q.more.triOn, ratio = q.more.ratioOn != 0;
                // (10.18: the area verdict alone needs no walk; concavity and flatness share the one the kernel makes)
                auto faces = (q.shape.concaveOn || q.shape.flatOn) ? qcFacesMoreOf<C, 2>(walk, ratio)
                             : q.shape.areaOn                      ? qcFacesMoreOf<C, 1>(walk, ratio)
                                                                   : qcFacesMoreOf<C, 0>(walk, ratio);
                hipLaunchKernelGGL(faces, grid, dim3(kQcBlock), 0, h->stream, m, pts, fCtr, fArea, cellCtr, (const double*)q.vol, (const int*)h->q.own,
                                   (const int*)h->q.nei, cp, q.lim, q.more, q.shape, exemptFace, exemptFaceOut, q.cellFlag, q.dev, pass, gate);
            } else
                hipLaunchKernelGGL(k_qc_faces<C>, grid, dim3(kQcBlock), 0, h->stream, m, pts, fCtr, fArea, cellCtr, (const int*)h->q.own, (const int*)h->q.nei, cp,
                                   q.lim, exemptFace, exemptFaceOut, q.cellFlag, q.dev, pass, gate);
        });
    const int gCells = (m.nCells + kQcBlock - 1) / kQcBlock;
    if (m.nCells > 0 && !h->useTiles)
        hipLaunchKernelGGL(k_qc_cells<true>, dim3(gCells), dim3(kQcBlock), 0, h->stream, m, fCtr, fArea, cellCtr,
                           enabling ? (const uint8_t*)nullptr : (const uint8_t*)q.exemptCell, enabling ? q.exemptCell : (uint8_t*)nullptr, (const uint8_t*)nullptr,
                           q.cellFlag, q.marks, q.dev, pass, gate);
    else if (m.nCells > 0 && !enabling)   // (enabling with tiles: k_qc_tile has left the exempt bytes and their count)
        hipLaunchKernelGGL(k_qc_cells<false>, dim3(gCells), dim3(kQcBlock), 0, h->stream, m, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                           (const uint8_t*)nullptr, (uint8_t*)nullptr, (const uint8_t*)q.tangled, q.cellFlag, q.marks, q.dev, pass, gate);
    HIP_OK(hipGetLastError());
    return 0;
}
static int qualityConstraintEvaluate(smgpu_handle* h, bool enabling, int pass, const smgpu_iter_stats* gate) {
    return qualityConstraintGeometry(h, enabling, pass, gate) || qualityConstraintVerdicts(h, enabling, pass, gate);
}
// behind the movePoints of an iteration: the passes on the points ptsCur now names; x: the points the iteration started from
// (the slab's slots are the scaled records of 10.19, whose head is the widest record of 10.18: kernels_quality_scale.hpp)
static int qualityConstraintQueueScaled(smgpu_handle* h, smgpu_quality_constraint_record_scaled* rec, int64_t number, const smgpu_iter_stats* gate, const double* x);
static int qualityConstraintQueue(smgpu_handle* h, int slot, int64_t number, const smgpu_iter_stats* gate, const double* x) {
    QualityConstraintHost& q = h->qc;
    smgpu_quality_constraint_record_scaled* wide = nullptr;
    if (q.slab.slot(slot, &wide)) return 1;
    if (q.scaling.scalePasses > 0) return qualityConstraintQueueScaled(h, wide, number, gate, x);
    smgpu_quality_constraint_record_all* const rec = reinterpret_cast<smgpu_quality_constraint_record_all*>(wide);
    const int nP = h->mv.nPoints;
    const int gApply = std::max(1, (int)(((int64_t)nP + kTanglePts - 1) / kTanglePts));
    for (int k = 0; k <= q.prm.passes; ++k) {
        if (qualityConstraintEvaluate(h, false, k, gate)) return 1;
        hipLaunchKernelGGL(k_qc_verdict, dim3(1), dim3(64), 0, h->stream, q.dev, q.acc, rec, (long long)number, k, (int)q.prm.passes, gate);
        // the record and the device words begin with the tangle constraint's (kernels_quality_constraint.hpp)
        hipLaunchKernelGGL(k_tangle_apply, dim3(gApply), dim3(kTangleBlock), 0, h->stream, x, h->st.ptsCur, q.marks, nP, (const TangleDev*)&q.dev->t,
                           reinterpret_cast<smgpu_tangle_record*>(rec), gate);
    }
    HIP_OK(hipGetLastError());
    return 0;
}
// 10.19, scaling on: the evaluations are the ones above and run to S + P; what follows a verdict is kernels_quality_scale.hpp's.
// Which of the two scale fields is current behind a launch is the host's to know: every launch of an iteration runs, or from
// some verdict on none does.
static int qualityConstraintQueueScaled(smgpu_handle* h, smgpu_quality_constraint_record_scaled* rec, int64_t number, const smgpu_iter_stats* gate, const double* x) {
    QualityConstraintHost& q = h->qc;
    const int nP = h->mv.nPoints, S = q.scaling.scalePasses, total = S + q.prm.passes, nSweeps = q.scaling.nSmoothScale;
    const long long nL = 3 * (long long)nP;
    const int gKeep = (int)std::max<long long>(1, ((nL >> 1) + (long long)kGuardBlock * kGuardPer - 1) / ((long long)kGuardBlock * kGuardPer));
    const int gWord = std::max(1, (int)((((int64_t)nP + 3) / 4 + kQsBlock - 1) / kQsBlock)), gPoint = std::max(1, (int)std::min<int64_t>(q.maxGrid, ((int64_t)nP + kQsBlock - 1) / kQsBlock));
    double *sCur = q.scaleA, *sNext = q.scaleB;
    for (int k = 0; k <= total; ++k) {
        if (qualityConstraintEvaluate(h, false, k, gate)) return 1;
        hipLaunchKernelGGL(k_qs_verdict, dim3(1), dim3(64), 0, h->stream, q.dev, q.acc, rec, (long long)number, k, S, total, gate);
        if (k == 0)
            hipLaunchKernelGGL(k_qs_keep, dim3(gKeep), dim3(kGuardBlock), 0, h->stream, (const double*)h->st.ptsCur, q.L, nL, sCur, q.nScale, (const QcDev*)q.dev, gate);
        hipLaunchKernelGGL(k_qs_mark, dim3(gWord), dim3(kQsBlock), 0, h->stream, q.marks, sCur, nP, q.scaling.errorReduction,
                           k == total ? (int)kQsFull : (k < S ? (int)kQsScale : (int)kQsZero), (const QcDev*)q.dev, gate);
        for (int i = 0; i < nSweeps && k < total; ++i) {
            hipLaunchKernelGGL(k_qs_sweep, dim3(gPoint), dim3(kQsBlock), 0, h->stream, h->mv, (const double*)sCur, sNext, (const QcDev*)q.dev, gate);
            std::swap(sCur, sNext);
        }
        hipLaunchKernelGGL(k_qs_apply, dim3(gPoint), dim3(kQsBlock), 0, h->stream, x, (const double*)q.L, h->st.ptsCur, (const double*)sCur, nP, (const QcDev*)q.dev, rec,
                           gate);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// What enabling shares between the serial and the coupled form.  First the refusals both make first, in their order; api names
// the entry called; coupled: the form, which wants an engine with a halo, where `serial` names the entry a serial engine takes
static int qualityConstraintRefusals(smgpu_handle* h, const std::string& api, const smgpu_quality_constraint_params& prm, const QcMore& more,
                                     const QcShapeLimits& shape, bool coupled, const char* serial) {
    if (prm.passes < 0) return fail(api + ": passes < 0");
    if (std::isnan(prm.maxNonOrtho) || std::isnan(prm.maxInternalSkewness) || std::isnan(prm.maxBoundarySkewness) || std::isnan(more.minTet) ||
        std::isnan(more.minTwist) || std::isnan(more.minTri) || std::isnan(more.minWeight) || std::isnan(more.minRatio) || std::isnan(more.minDet) ||
        std::isnan(shape.maxConcave) || std::isnan(shape.k.minFlat) || std::isnan(shape.k.minVol) || std::isnan(shape.k.minArea))
        return fail(api + ": a limit is NaN");
    if (shape.maxConcave < 0.0) return fail(api + ": maxConcave < 0");
    if (!coupled && h->haloOn) return fail(kQualityHaloRefusal);
    if (coupled && !h->haloOn) return fail(api + ": the engine has no halo (smgpu_halo_configure); a serial engine takes " + serial);
    if (h->bndOn && (coupled || !h->bndRevert))
        return fail(api + ": not available on an engine with boundary point smoothing (it rewrites the proposals of the boundary "
                    "points from state that a reverted iteration would leave ahead of the points)");
    if (h->tg.on)
        return fail(api + ": the tangle constraint is on (" + (coupled ? "smgpu_set_tangle_constraint_coupled" : "smgpu_set_tangle_constraint") +
                    "), and this constraint contains it; switch it off first");
    return 0;
}
// ... then, every refusal made: the constraint that was on goes, and the buffers, limits and launch choices of the new one are set
static int qualityConstraintAllocate(smgpu_handle* h, const smgpu_quality_constraint_params& prm, const QcMore& more, const QcShapeLimits& shape) {
    if (qualityConstraintOff(h)) return 1;
    if (flushDeferred(h)) return 1;
    if (qualityEnsure(h)) return 1;                  // owner / neighbour by face
    const MeshView& m = h->mv;
    const size_t nMark = ((size_t)std::max(1, m.nPoints) + 3) & ~(size_t)3, nCell = (size_t)std::max(1, m.nCells), nFace = (size_t)std::max(1, m.nFaces);
    QualityConstraintHost& q = h->qc;
    if (q.block.alloc(&q.dev, 1) || q.block.alloc(&q.exemptCell, nCell) || q.block.alloc(&q.cellFlag, nCell) || q.block.alloc(&q.tangled, nCell) || q.block.alloc(&q.exemptFace, nFace) ||
        q.block.alloc(&q.marks, nMark) || q.block.alloc(&q.cellCtr, 3 * nCell) || q.block.alloc(&q.acc, 1))
        return q.block.failed("the quality constraint");
    q.more = more;
    q.shape = shape.k;
    q.maxConcave = shape.maxConcave;
    q.faceMore = more.tetOn || more.twistOn || more.triOn || more.weightOn || more.ratioOn || shape.k.concaveOn || shape.k.flatOn || shape.k.areaOn;
    q.cellMore = more.ratioOn || more.detOn || shape.k.volOn;
    if (q.cellMore && (q.block.alloc(&q.vol, nCell) || q.block.alloc(&q.exemptDet, nCell))) return q.block.failed("the quality constraint");
    HIP_OK(hipMemsetAsync(q.dev, 0, sizeof(QcDev), h->stream));
    HIP_OK(hipMemsetAsync(q.exemptCell, 0, nCell, h->stream));
    HIP_OK(hipMemsetAsync(q.cellFlag, 0, nCell, h->stream));
    HIP_OK(hipMemsetAsync(q.tangled, 0, nCell, h->stream));
    HIP_OK(hipMemsetAsync(q.exemptFace, 0, nFace, h->stream));
    HIP_OK(hipMemsetAsync(q.marks, 0, nMark, h->stream));
    HIP_OK(hipMemsetAsync(q.acc, 0, sizeof(Accum), h->stream));
    if (q.cellMore) HIP_OK(hipMemsetAsync(q.exemptDet, 0, nCell, h->stream));
    q.prm = prm;
    // cosT exactly as qualityThresholds() forms the report's cosine
    const smgpu_quality_params rp{prm.maxNonOrtho, prm.maxInternalSkewness, 1e-6, 1000.0};
    q.lim = QcLimits{qualityThresholds(&rp).cosNonOrth, prm.maxInternalSkewness, prm.maxBoundarySkewness, prm.maxNonOrtho < 180.0 ? 1 : 0,
                     prm.maxInternalSkewness > 0.0 ? 1 : 0, prm.maxBoundarySkewness > 0.0 ? 1 : 0};
    return 0;
}

// the serial form (qualityConstraintSet below dispatches the six entries): name names the entry called, in its refusals; more: the
// limits of 10.16 (all off under smgpu_set_quality_constraint); shape: those of 10.18 (all off under the two older entries)
static int qualityConstraintEnable(smgpu_handle* h, const char* name, const smgpu_quality_constraint_params& prm, const QcMore& more, const QcShapeLimits& shape) {
    const std::string api(name);
    if (qualityConstraintRefusals(h, api, prm, more, shape, false, nullptr)) return 1;
    if (h->iterOpen) return fail(api + ": between smgpu_iter_begin and smgpu_iter_end");
    if (qualityConstraintAllocate(h, prm, more, shape)) return 1;
    QualityConstraintHost& q = h->qc;
    // the exempt cells and faces: one evaluation of the current points
    if (qualityConstraintEvaluate(h, true, 0, nullptr)) { q.release(); return 1; }
    QcDev qd{};
    HIP_OK(hipMemcpyAsync(&qd, q.dev, sizeof(QcDev), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemsetAsync(q.dev, 0, sizeof(QcDev), h->stream));
    if (checkDeviceError(h)) { q.release(); return 1; }
    q.nExemptCells = qd.t.badNow;
    q.nExemptFaces = qd.facesNow;
    q.nExemptDet = qd.underDetNow;
    q.nExemptVol = qd.smallVolNow;
    q.since = h->iterCount;
    q.on = true;
    return 0;
}
// The getters.  Every record in the slab and the one state are the widest (10.19's); a narrower getter answers with their head
// (quality_state.hpp, QC_HEAD_OF).  api names the entry called, in its refusals.
static int qualityConstraintCoupledFlush(smgpu_handle* h);
extern "C++" {
template <class Rec>
static int qualityConstraintRecords(smgpu_handle* h, Rec* out, int64_t cap, int64_t* n, const char* api) {
    if (!h || !n) return fail("null argument");
    if (h->qc.coupled) {   // the records of the chunk in use are still on the device
        if (h->qc.k >= 0) return fail(std::string(api) + ": between the passes of an iteration (smgpu_quality_constraint_pass_begin / _end)");
        HIP_OK(hipSetDevice(h->device));
        if (qualityConstraintCoupledFlush(h)) return 1;
    }
    return h->qc.slab.drainHeads(out, cap, n, api);
}
// while the constraint is off, or enabled with its exempt faces not taken yet, the counts and the running number read 0
template <class State>
static int qualityConstraintState(smgpu_handle* h, State* out) {
    if (!h || !out) return fail("null argument");
    const QualityConstraintHost& q = h->qc;
    const bool on = q.on && !q.pending;
    const int64_t number = q.coupled ? q.count : h->iterCount - q.since;
    *out = qcHead<State>(smgpu_quality_constraint_state_scaled{
        on ? 1 : 0, q.prm.passes, q.prm.maxNonOrtho, q.prm.maxInternalSkewness, q.prm.maxBoundarySkewness, on ? q.nExemptCells : 0, on ? q.nExemptFaces : 0, on ? number : 0,
        q.more.minTet, q.more.minTwist, q.more.minTri, q.more.minWeight, q.more.minRatio, q.more.minDet, on ? q.nExemptDet : 0,
        q.maxConcave, q.shape.minFlat, q.shape.minVol, q.shape.minArea, on ? q.nExemptVol : 0, q.scaling.scalePasses, q.scaling.nSmoothScale, q.scaling.errorReduction});
    return 0;
}
}
int smgpu_get_quality_constraint_records(smgpu_handle* h, smgpu_quality_constraint_record* out, int64_t cap, int64_t* n) {
    return qualityConstraintRecords(h, out, cap, n, "smgpu_get_quality_constraint_records");
}
int smgpu_get_quality_constraint_records_full(smgpu_handle* h, smgpu_quality_constraint_record_full* out, int64_t cap, int64_t* n) {
    return qualityConstraintRecords(h, out, cap, n, "smgpu_get_quality_constraint_records_full");
}
int smgpu_get_quality_constraint_records_all(smgpu_handle* h, smgpu_quality_constraint_record_all* out, int64_t cap, int64_t* n) {
    return qualityConstraintRecords(h, out, cap, n, "smgpu_get_quality_constraint_records_all");
}
int smgpu_get_quality_constraint_records_scaled(smgpu_handle* h, smgpu_quality_constraint_record_scaled* out, int64_t cap, int64_t* n) {
    return qualityConstraintRecords(h, out, cap, n, "smgpu_get_quality_constraint_records_scaled");
}
int smgpu_get_quality_constraint_state(smgpu_handle* h, smgpu_quality_constraint_state* out) { return qualityConstraintState(h, out); }
int smgpu_get_quality_constraint_state_full(smgpu_handle* h, smgpu_quality_constraint_state_full* out) { return qualityConstraintState(h, out); }
int smgpu_get_quality_constraint_state_all(smgpu_handle* h, smgpu_quality_constraint_state_all* out) { return qualityConstraintState(h, out); }
int smgpu_get_quality_constraint_state_scaled(smgpu_handle* h, smgpu_quality_constraint_state_scaled* out) { return qualityConstraintState(h, out); }
// 10.19: the scaling passes of the serial constraint.  Their memory is the constraint's own second block: allocated here, freed
// here with scalePasses = 0 and by everything that switches the constraint off (QualityConstraintHost::release)
int smgpu_set_quality_constraint_scaling(smgpu_handle* h, const smgpu_quality_constraint_scaling* p) {
    if (!h) return fail("null handle");
    const std::string api("smgpu_set_quality_constraint_scaling");
    const smgpu_quality_constraint_scaling prm = p ? *p : smgpu_quality_constraint_scaling{0, 4, 0.75};
    if (prm.scalePasses < 0) return fail(api + ": scalePasses < 0");
    if (!(prm.errorReduction >= 0.0 && prm.errorReduction < 1.0)) return fail(api + ": errorReduction is outside 0 <= errorReduction < 1");
    if (prm.nSmoothScale < 0) return fail(api + ": nSmoothScale < 0");
    if (h->haloOn) return fail(api + ": not available on an engine with a halo (the coupled form of the quality constraint has no scaling passes)");
    if (h->bndOn && h->bndRevert)
        return fail(api + ": not available on an engine with boundary point smoothing: scaling passes with boundary point smoothing are not available (a scaled "
                    "boundary point leaves the target surface)");
    if (h->bndOn) return fail(api + ": not available on an engine with boundary point smoothing (nor is the quality constraint)");
    if (h->tg.on)
        return fail(api + ": the tangle constraint is on (smgpu_set_tangle_constraint), and it has no scaling passes; the quality constraint with its "
                    "three criteria off is the tangle constraint");
    if (!h->qc.on) return fail(api + ": the quality constraint is off (smgpu_set_quality_constraint); switch it on first");
    if (h->iterOpen) return fail(api + ": between smgpu_iter_begin and smgpu_iter_end");
    if ((int64_t)prm.scalePasses + (int64_t)h->qc.prm.passes > 0x7fffffffLL) return fail(api + ": scalePasses + passes is above 2147483647");
    HIP_OK(hipSetDevice(h->device));
    QualityConstraintHost& q = h->qc;
    if (q.scaleBlock.live()) {
        HIP_OK(hipStreamSynchronize(h->stream));
        q.releaseScaling();
    }
    if (prm.scalePasses == 0) return 0;
    const size_t nP = (size_t)std::max(1, h->mv.nPoints), nScale = (nP + 1) & ~(size_t)1;
    if (q.scaleBlock.alloc(&q.L, 3 * nP) || q.scaleBlock.alloc(&q.scaleA, nScale) || q.scaleBlock.alloc(&q.scaleB, nScale)) {
        const int rc = q.scaleBlock.failed("the quality constraint's scaling passes");
        q.releaseScaling();
        return rc;
    }
    q.nScale = (long long)nScale;
    q.maxGrid = std::max(1, envInt("SMGPU_QS_MAX_GRID", kQsMaxGrid));   // (tests: several trips per lane on a small mesh)
    q.scaling = prm;
    return 0;
}

// ---- the coupled form on an engine with a halo (DESIGN.md "Mesh quality", 10.15) ----
// 10.13's protocol with one more exchange per pass: a processor face is an internal face of the global mesh, and its verdict needs
// the neighbour rank's cell centre at the points being judged.  Every kernel goes onto the engine's stream, behind the iteration's
// own; x is the buffer smgpu_iter_end swapped out, as in 10.13.
static int qualityConstraintCoupledFlush(smgpu_handle* h) {
    QualityConstraintHost& q = h->qc;
    if (q.slabUsed > 0) {
        if (q.slab.readBack(h->stream, q.slabUsed)) return 1;
        HIP_OK(hipStreamSynchronize(h->stream));
        q.slab.keep(q.slabUsed);
    }
    q.slabUsed = 0;
    q.slabFresh = false;
    return 0;
}
// the first half of an evaluation of the points ptsCur names: the geometry half, ungated, then the pack of the constraint's own
// cell centres -- never the loop's, which are those of other points -- and with minVolRatio on of its volumes (10.17), and the
// wait: sendCc and sendVc are the host's to move
static int qualityConstraintCoupledGeometry(smgpu_handle* h, bool enabling) {
    QualityConstraintHost& q = h->qc;
    if (qualityConstraintGeometry(h, enabling, 0, nullptr)) return 1;
    if (q.nProc > 0)
        hipLaunchKernelGGL(k_quality_pack, dim3((q.nProc + kQualityBlock - 1) / kQualityBlock), dim3(kQualityBlock), 0, h->stream, (const int*)h->q.own,
                           (const double*)q.cellCtr, (const int*)q.procFace, q.nProc, q.sendCc);
    if (q.nProc > 0 && q.more.ratioOn)
        hipLaunchKernelGGL(k_quality_pack_volumes, dim3((q.nProc + kQualityBlock - 1) / kQualityBlock), dim3(kQualityBlock), 0, h->stream, (const int*)h->q.own,
                           (const double*)q.vol, (const int*)q.procFace, q.nProc, q.sendVc);
    HIP_OK(hipGetLastError());
    return checkDeviceError(h);
}
// the second half, recvCc (and recvVc) moved by the host: the verdict half, ungated, and in a pass the pack of the shared points'
// marks; *qd: the counts, read with the loop's error word -- sendT is complete when this returns
static int qualityConstraintCoupledVerdicts(smgpu_handle* h, bool enabling, QcDev* qd) {
    QualityConstraintHost& q = h->qc;
    if (computeAfterExch(h)) return 1;          // exchange Cc has been enqueued by the host
    if (qualityConstraintVerdicts(h, enabling, 0, nullptr)) return 1;
    if (!enabling && h->nSend > 0)
        hipLaunchKernelGGL(k_tangle_pack, dim3((h->nSend + kTangleBlock - 1) / kTangleBlock), dim3(kTangleBlock), 0, h->stream, h->nSend, (const int*)h->dSendShared,
                           (const int*)h->dSharedLocal, (const uint8_t*)q.marks, q.sendT);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(qd, q.dev, sizeof(QcDev), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemsetAsync(q.dev, 0, sizeof(QcDev), h->stream));
    return checkDeviceError(h);
}

// the coupled form (qualityConstraintSet below dispatches the six entries): name names the entry called, in its refusals, serial
// the entry a serial engine takes; full: one of the two entries with volume buffers in d (10.17, 10.18), which the refusal of the
// other coupled entry names; else more is all off and d's tail null
static int qualityConstraintCoupledEnable(smgpu_handle* h, const char* name, bool full, const smgpu_quality_constraint_params& prm, const QcMore& more,
                                          const smgpu_quality_constraint_halo_desc_full* d, const QcShapeLimits& shape, const char* serial) {
    const std::string api(name);
    if (qualityConstraintRefusals(h, api, prm, more, shape, true, serial)) return 1;
    if (h->qc.on && h->qc.coupled && h->qc.full != full)
        return fail(api + ": the quality constraint is on through " + (full ? "smgpu_set_quality_constraint_coupled" : "smgpu_set_quality_constraint_limits_coupled") +
                    "; switch it off first");
    if (h->iterOpen) return fail(api + ": between smgpu_iter_begin and smgpu_iter_end");
    if (!d || !d->coupling || (h->nSend && !d->sendT) || (h->nRecv && !d->recvT)) return fail(api + ": null exchange buffer");
    const MeshView& m = h->mv;
    std::vector<int32_t> key;
    std::vector<int> procFace, slot;
    int64_t nProc = 0, notCounted = 0;
    if (qualityCouplingTables(name, m, d->coupling, key, procFace, slot, nProc, notCounted)) return 1;
    if (nProc > 0 && (!d->sendCc || !d->recvCc)) return fail(api + ": null exchange buffer");
    if (nProc > 0 && more.ratioOn && (!d->sendVc || !d->recvVc)) return fail(api + ": null exchange buffer (minVolRatio is on: sendVc / recvVc)");
    if (qualityConstraintAllocate(h, prm, more, shape)) return 1;
    const size_t nB = (size_t)(m.nFaces - m.nInternalFaces);
    QualityConstraintHost& q = h->qc;
    if (q.block.alloc(&q.counted, (size_t)std::max(1, h->nShared)) || q.block.alloc(&q.procFace, (size_t)std::max<int64_t>(1, nProc)) ||
        q.block.alloc(&q.slot, std::max<size_t>(1, nB)))
        return q.block.failed("the quality constraint");
    if (h->nShared > 0) HIP_OK(hipMemcpyAsync(q.counted, h->sharedMasterHost.data(), (size_t)h->nShared, hipMemcpyHostToDevice, h->stream));
    if (nProc) HIP_OK(hipMemcpyAsync(q.procFace, procFace.data(), sizeof(int) * (size_t)nProc, hipMemcpyHostToDevice, h->stream));
    if (nB) HIP_OK(hipMemcpyAsync(q.slot, slot.data(), sizeof(int) * nB, hipMemcpyHostToDevice, h->stream));
    q.nProc = (int)nProc;
    q.sendT = (int*)d->sendT; q.recvT = (int*)d->recvT;
    q.sendCc = (double*)d->sendCc; q.recvCc = (double*)d->recvCc;
    q.sendVc = (double*)d->sendVc; q.recvVc = (double*)d->recvVc;
    q.full = full;
    q.coupled = true;                                // from here the evaluation's kernels take the coupling
    // the exempt cells and faces: one evaluation of the current points, its second half behind the host's exchange of Cc
    // (the wait inside also covers the uploads from the host vectors above)
    if (qualityConstraintCoupledGeometry(h, true)) { q.release(); return 1; }
    q.count = 0;
    q.k = -1;
    q.stage = 0;
    q.pending = true;
    q.on = true;
    return 0;
}
// The six entries.  What one asks for: the widest limits, the name of the entry called, and for a coupled entry the name of the
// entry a serial engine takes (NULL: a serial entry) and `full`.  Each widens its limits over the defaults (NULL: the defaults;
// a narrower struct is the head of the widest, quality_state.hpp), names itself, and goes through the one body.
struct QcRequest { smgpu_quality_constraint_limits_all l; const char *name, *serial; bool full; };
static int qualityConstraintSet(smgpu_handle* h, int32_t on, const QcRequest& r, const smgpu_quality_constraint_halo_desc_full* d) {
    if (!h) return fail("null handle");
    HIP_OK(hipSetDevice(h->device));
    if (!on) return qualityConstraintOff(h);
    const smgpu_quality_constraint_params prm = qcHead<smgpu_quality_constraint_params>(r.l);
    if (r.serial) return qualityConstraintCoupledEnable(h, r.name, r.full, prm, qualityConstraintMore(r.l), d, qualityConstraintShape(r.l), r.serial);
    return qualityConstraintEnable(h, r.name, prm, qualityConstraintMore(r.l), qualityConstraintShape(r.l));
}
int smgpu_set_quality_constraint(smgpu_handle* h, const smgpu_quality_constraint_params* p, int32_t on) {
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint", nullptr, false}, nullptr);
}
int smgpu_set_quality_constraint_limits(smgpu_handle* h, const smgpu_quality_constraint_limits* p, int32_t on) {
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint_limits", nullptr, false}, nullptr);
}
int smgpu_set_quality_constraint_limits_all(smgpu_handle* h, const smgpu_quality_constraint_limits_all* p, int32_t on) {
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint_limits_all", nullptr, false}, nullptr);
}
int smgpu_set_quality_constraint_coupled(smgpu_handle* h, const smgpu_quality_constraint_params* p, const smgpu_quality_constraint_halo_desc* d, int32_t on) {
    const smgpu_quality_constraint_halo_desc_full df = qcWiden(d, smgpu_quality_constraint_halo_desc_full{});
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint_coupled", "smgpu_set_quality_constraint", false},
                                d ? &df : nullptr);
}
int smgpu_set_quality_constraint_limits_coupled(smgpu_handle* h, const smgpu_quality_constraint_limits* p, const smgpu_quality_constraint_halo_desc_full* d,
                                                int32_t on) {
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint_limits_coupled", "smgpu_set_quality_constraint_limits", true}, d);
}
int smgpu_set_quality_constraint_limits_all_coupled(smgpu_handle* h, const smgpu_quality_constraint_limits_all* p, const smgpu_quality_constraint_halo_desc_full* d,
                                                    int32_t on) {
    return qualityConstraintSet(h, on, QcRequest{qcWiden(p, kQcLimitsDefault), "smgpu_set_quality_constraint_limits_all_coupled", "smgpu_set_quality_constraint_limits_all", true},
                                d);
}
int smgpu_quality_constraint_coupled_exempt(smgpu_handle* h) {
    if (!h) return fail("null handle");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled || !q.pending)
        return fail("smgpu_quality_constraint_coupled_exempt: no coupled quality constraint waits for its exempt faces (smgpu_set_quality_constraint_coupled)");
    if (h->iterOpen) return fail("smgpu_quality_constraint_coupled_exempt: between smgpu_iter_begin and smgpu_iter_end");
    HIP_OK(hipSetDevice(h->device));
    QcDev qd{};
    if (qualityConstraintCoupledVerdicts(h, true, &qd)) { (void)qualityConstraintOff(h); return 1; }
    q.nExemptCells = qd.t.badNow;
    q.nExemptFaces = qd.facesNow;
    q.nExemptDet = qd.underDetNow;
    q.nExemptVol = qd.smallVolNow;
    q.pending = false;
    return 0;
}
// behind smgpu_iter_end: the iteration waits for its passes
static void qualityConstraintCoupledIterEnd(smgpu_handle* h, const double* x) {
    h->qc.x = x;
    h->qc.k = 0;
    h->qc.reverting = 0;
    h->qc.stage = 0;
    h->qc.kept = false;                         // (10.20: the scale state does not outlive an iteration)
    h->qc.nScaleRan = h->qc.sweepsDue = 0;
}
int smgpu_quality_constraint_pass_begin(smgpu_handle* h) {
    if (!h) return fail("null handle");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled) return fail("smgpu_quality_constraint_pass_begin: the coupled quality constraint is not on (smgpu_set_quality_constraint_coupled)");
    if (q.pending) return fail("smgpu_quality_constraint_pass_begin: the exempt faces have not been taken (smgpu_quality_constraint_coupled_exempt)");
    if (h->iterOpen) return fail("smgpu_quality_constraint_pass_begin: between smgpu_iter_begin and smgpu_iter_end");
    if (q.k < 0) return fail("smgpu_quality_constraint_pass_begin: no iteration waits for its passes (the passes follow smgpu_iter_end)");
    if (q.stage != 0) return fail("smgpu_quality_constraint_pass_begin: the pass in hand has not been closed (smgpu_quality_constraint_pass_faces / _end)");
    HIP_OK(hipSetDevice(h->device));
    if (q.k == 0 && (!q.slabFresh || q.slabUsed >= QualityConstraintHost::kChunk)) {
        if (qualityConstraintCoupledFlush(h)) return 1;
        if (q.slab.begin(h->stream, QualityConstraintHost::kChunk)) return 1;
        q.slabFresh = true;
    }
    if (qualityConstraintCoupledGeometry(h, false)) return 1;
    q.stage = 1;
    return 0;
}
int smgpu_quality_constraint_pass_faces(smgpu_handle* h, int64_t* nBadLocal) {
    if (!h || !nBadLocal) return fail("null argument");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled) return fail("smgpu_quality_constraint_pass_faces: the coupled quality constraint is not on (smgpu_set_quality_constraint_coupled)");
    if (q.stage != 1 || q.k < 0) return fail("smgpu_quality_constraint_pass_faces without smgpu_quality_constraint_pass_begin");
    HIP_OK(hipSetDevice(h->device));
    QcDev qd{};
    if (qualityConstraintCoupledVerdicts(h, false, &qd)) return 1;
    if (q.k == 0) {
        q.n0[0] = qd.t.badNow; q.n0[1] = qd.tangledNow; q.n0[2] = qd.nonOrthoNow; q.n0[3] = qd.skewNow;
        q.n0[4] = qd.lowTetNow; q.n0[5] = qd.lowTwistNow; q.n0[6] = qd.lowTriNow; q.n0[7] = qd.lowWeightNow; q.n0[8] = qd.lowRatioNow; q.n0[9] = qd.underDetNow;
        q.n0[10] = qd.concaveNow; q.n0[11] = qd.warpedNow; q.n0[12] = qd.smallAreaNow; q.n0[13] = qd.smallVolNow;
    }
    q.stage = 2;
    *nBadLocal = qd.t.badNow;
    return 0;
}
static int qualityConstraintPassEndScaled(smgpu_handle* h, int64_t nBadGlobal, int32_t* done);
int smgpu_quality_constraint_pass_end(smgpu_handle* h, int64_t nBadGlobal, int32_t* done) {
    if (!h || !done) return fail("null argument");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled) return fail("smgpu_quality_constraint_pass_end: the coupled quality constraint is not on (smgpu_set_quality_constraint_coupled)");
    if (q.scaleCoupled) return qualityConstraintPassEndScaled(h, nBadGlobal, done);   // 10.20, below
    if (q.stage != 2 || q.k < 0) return fail("smgpu_quality_constraint_pass_end without smgpu_quality_constraint_pass_faces");
    if (nBadGlobal < 0) return fail("smgpu_quality_constraint_pass_end: nBadGlobal < 0");
    HIP_OK(hipSetDevice(h->device));
    smgpu_quality_constraint_record_scaled* wide = nullptr;
    if (q.slab.slot(q.slabUsed, &wide)) return 1;
    smgpu_quality_constraint_record_all* const rec = reinterpret_cast<smgpu_quality_constraint_record_all*>(wide);   // (its head; no scaling in the coupled form)
    const bool full = nBadGlobal > 0 && q.k == q.prm.passes;
    // the record begins with the tangle constraint's (kernels_quality_constraint.hpp)
    if (nBadGlobal > 0 && coupledRevert(h, full, q.recvT, q.marks, q.x, q.counted, reinterpret_cast<smgpu_tangle_record*>(rec), q.reverting)) return 1;
    const bool close = nBadGlobal == 0 || full;
    if (close) {
        QcCounts c{};   // (10.15's entry: the counts of 10.16 and 10.18 are 0, as the zeroed slot's were)
        for (int i = 0; i < 14; ++i) c.n[i] = (long long)q.n0[i];
        hipLaunchKernelGGL(k_qc_close, dim3(1), dim3(64), 0, h->stream, rec, (long long)(q.count + 1), q.reverting, full ? 1 : 0, c);
        ++q.count;
        ++q.slabUsed;
        q.k = -1;
    } else ++q.k;
    q.stage = 0;
    *done = close ? 1 : 0;
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- the scaling passes of the coupled form (kernels_quality_scale_coupled.hpp, DESIGN.md "Mesh quality", 10.20) ----
// 10.19's scale field on every rank, driven by the host like the passes of 10.15: the pass runs to S + P, and between the move of
// T and smgpu_quality_constraint_pass_end stand smgpu_quality_constraint_pass_scale and, per sweep, _pass_sweep behind the host's
// move of S.  The memory is the constraint's second block, as the serial form's.
int smgpu_set_quality_constraint_scaling_coupled(smgpu_handle* h, const smgpu_quality_constraint_scaling* p, const smgpu_quality_scale_coupling* c) {
    if (!h) return fail("null handle");
    const std::string api("smgpu_set_quality_constraint_scaling_coupled");
    const smgpu_quality_constraint_scaling prm = p ? *p : smgpu_quality_constraint_scaling{0, 4, 0.75};
    if (prm.scalePasses < 0) return fail(api + ": scalePasses < 0");
    if (!(prm.errorReduction >= 0.0 && prm.errorReduction < 1.0)) return fail(api + ": errorReduction is outside 0 <= errorReduction < 1");
    if (prm.nSmoothScale < 0) return fail(api + ": nSmoothScale < 0");
    if (!h->haloOn) return fail(api + ": the engine has no halo (smgpu_halo_configure); a serial engine takes smgpu_set_quality_constraint_scaling");
    if (h->bndOn && h->bndRevert)
        return fail(api + ": not available on an engine with boundary point smoothing: scaling passes with boundary point smoothing are not available (a scaled "
                    "boundary point leaves the target surface)");
    if (h->bndOn) return fail(api + ": not available on an engine with boundary point smoothing (nor is the quality constraint)");
    if (h->tg.on)
        return fail(api + ": the coupled tangle constraint is on (smgpu_set_tangle_constraint_coupled), and it has no scaling passes; the coupled quality "
                    "constraint with its three criteria off is the tangle constraint");
    QualityConstraintHost& q = h->qc;
    if (!q.on || !q.coupled) return fail(api + ": the coupled quality constraint is off (smgpu_set_quality_constraint_coupled); switch it on first");
    if (q.pending) return fail(api + ": the exempt faces have not been taken (smgpu_quality_constraint_coupled_exempt)");
    if (h->iterOpen) return fail(api + ": between smgpu_iter_begin and smgpu_iter_end");
    if (q.k >= 0) return fail(api + ": the passes of an iteration are due (smgpu_quality_constraint_pass_begin / _end)");
    if ((int64_t)prm.scalePasses + (int64_t)q.prm.passes > 0x7fffffffLL) return fail(api + ": scalePasses + passes is above 2147483647");
    const int nS = h->nShared, nP = h->mv.nPoints;
    std::vector<int> rowOff, rowPt, deg;
    if (prm.scalePasses > 0) {
        if (!c || (nS > 0 && (!c->rowOffsets || !c->sharedDeg))) return fail(api + ": null table");
        if ((h->nSend && !c->sendS) || (h->nRecv && !c->recvS)) return fail(api + ": null exchange buffer");
        rowOff.assign((size_t)nS + 1, 0);
        deg.assign((size_t)std::max(1, nS), 0);
        for (int i = 0; i <= nS && nS > 0; ++i) rowOff[(size_t)i] = c->rowOffsets[i];
        if (rowOff[0] != 0) return fail(api + ": rowOffsets does not start at 0");
        for (int i = 0; i < nS; ++i) {
            if (rowOff[(size_t)i + 1] < rowOff[(size_t)i]) return fail(api + ": rowOffsets decreases");
            deg[(size_t)i] = c->sharedDeg[i];
            if (deg[(size_t)i] < rowOff[(size_t)i + 1] - rowOff[(size_t)i]) return fail(api + ": sharedDeg is below the counted entries of a row");
        }
        const int nE = rowOff[(size_t)nS];
        if (nE > 0 && !c->rowPoints) return fail(api + ": null table");
        rowPt.assign((size_t)std::max(1, nE), 0);
        for (int k = 0; k < nE; ++k) {
            rowPt[(size_t)k] = c->rowPoints[k];
            if (rowPt[(size_t)k] < 0 || rowPt[(size_t)k] >= nP) return fail(api + ": rowPoints out of range");
        }
    }
    HIP_OK(hipSetDevice(h->device));
    if (q.scaleBlock.live()) {
        HIP_OK(hipStreamSynchronize(h->stream));
        q.releaseScaling();
    }
    if (prm.scalePasses == 0) return 0;
    const size_t nPts = (size_t)std::max(1, nP), nScale = (nPts + 1) & ~(size_t)1;
    if (q.scaleBlock.alloc(&q.L, 3 * nPts) || q.scaleBlock.alloc(&q.scaleA, nScale) || q.scaleBlock.alloc(&q.scaleB, nScale) ||
        q.scaleBlock.alloc(&q.scRowOff, rowOff.size()) || q.scaleBlock.alloc(&q.scRowPt, rowPt.size()) || q.scaleBlock.alloc(&q.scDeg, deg.size()) ||
        q.scaleBlock.alloc(&q.scPart, (size_t)std::max(1, nS))) {
        const int rc = q.scaleBlock.failed("the quality constraint's scaling passes");
        q.releaseScaling();
        return rc;
    }
    // (the host vectors live until the wait below)
    hipError_t e = hipMemcpyAsync(q.scRowOff, rowOff.data(), sizeof(int) * rowOff.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q.scRowPt, rowPt.data(), sizeof(int) * rowPt.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q.scDeg, deg.data(), sizeof(int) * deg.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        q.releaseScaling();
        return fail(api + ": " + hipGetErrorString(e));
    }
    q.nScale = (long long)nScale;
    q.maxGrid = std::max(1, envInt("SMGPU_QS_MAX_GRID", kQsMaxGrid));
    q.sendS = (double*)c->sendS; q.recvS = (double*)c->recvS;
    q.scaling = prm;
    q.scaleCoupled = true;
    return 0;
}
// the local half of a sweep: 10.19's sweep over every point from the rank's rows, and the partial sums of the shared points from
// the same field into scPart and sendS
static void qualityConstraintSweepHalf(smgpu_handle* h) {
    QualityConstraintHost& q = h->qc;
    const int nP = h->mv.nPoints, gPoint = std::max(1, (int)std::min<int64_t>(q.maxGrid, ((int64_t)nP + kQsBlock - 1) / kQsBlock));
    hipLaunchKernelGGL(k_qs_sweep, dim3(gPoint), dim3(kQsBlock), 0, h->stream, h->mv, (const double*)q.sCur, q.sNext, (const QcDev*)q.dev, (const smgpu_iter_stats*)nullptr);
    if (h->nShared > 0) {
        const int gShared = std::max(1, (int)std::min<int64_t>(q.maxGrid, ((int64_t)h->nShared + kQsBlock - 1) / kQsBlock));
        hipLaunchKernelGGL(k_qsc_partial, dim3(gShared), dim3(kQsBlock), 0, h->stream, h->nShared, (const int*)q.scRowOff, (const int*)q.scRowPt, (const double*)q.sCur,
                           q.scPart, (const int*)h->dSendOff, (const int*)h->dSendSlots, q.sendS);
    }
}
int smgpu_quality_constraint_pass_scale(smgpu_handle* h, int64_t nBadGlobal) {
    if (!h) return fail("null handle");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled) return fail("smgpu_quality_constraint_pass_scale: the coupled quality constraint is not on (smgpu_set_quality_constraint_coupled)");
    if (!q.scaleCoupled) return fail("smgpu_quality_constraint_pass_scale: the scaling passes are off (smgpu_set_quality_constraint_scaling_coupled)");
    if (q.stage == 3) return fail("smgpu_quality_constraint_pass_scale: called twice in one pass");
    if (q.stage != 2 || q.k < 0) return fail("smgpu_quality_constraint_pass_scale without smgpu_quality_constraint_pass_faces");
    if (nBadGlobal <= 0) return fail("smgpu_quality_constraint_pass_scale: nBadGlobal <= 0 (a clean pass goes to smgpu_quality_constraint_pass_end)");
    HIP_OK(hipSetDevice(h->device));
    const int nP = h->mv.nPoints, S = q.scaling.scalePasses, total = S + q.prm.passes;
    const bool full = q.k == total;
    if (!full) {
        if (computeAfterExch(h)) return 1;      // exchange T has been enqueued by the host
        if (h->nShared > 0 && h->nRecv > 0)
            hipLaunchKernelGGL(k_tangle_combine, dim3((h->nShared + kTangleBlock - 1) / kTangleBlock), dim3(kTangleBlock), 0, h->stream, h->nShared,
                               (const int*)h->dSharedLocal, (const int*)h->dCombOff, (const int*)h->dCombSlots, (const int*)q.recvT, q.marks);
    }
    if (!q.kept) {                              // the iteration's first pass that is not clean
        const long long nL = 3 * (long long)nP;
        const int gKeep = (int)std::max<long long>(1, ((nL >> 1) + (long long)kGuardBlock * kGuardPer - 1) / ((long long)kGuardBlock * kGuardPer));
        q.sCur = q.scaleA; q.sNext = q.scaleB;
        hipLaunchKernelGGL(k_qs_keep, dim3(gKeep), dim3(kGuardBlock), 0, h->stream, (const double*)h->st.ptsCur, q.L, nL, q.sCur, q.nScale, (const QcDev*)q.dev,
                           (const smgpu_iter_stats*)nullptr);
        q.kept = true;
    }
    const int gWord = std::max(1, (int)((((int64_t)nP + 3) / 4 + kQsBlock - 1) / kQsBlock));
    hipLaunchKernelGGL(k_qs_mark, dim3(gWord), dim3(kQsBlock), 0, h->stream, q.marks, q.sCur, nP, q.scaling.errorReduction,
                       full ? (int)kQsFull : (q.k < S ? (int)kQsScale : (int)kQsZero), (const QcDev*)q.dev, (const smgpu_iter_stats*)nullptr);
    q.sweepsDue = full ? 0 : q.scaling.nSmoothScale;
    if (!full) {
        ++q.reverting;
        if (q.k < S) ++q.nScaleRan;
    }
    if (q.sweepsDue > 0) qualityConstraintSweepHalf(h);
    HIP_OK(hipGetLastError());
    q.scaleBad = nBadGlobal;
    q.stage = 3;
    return q.sweepsDue > 0 ? checkDeviceError(h) : 0;     // sendS is the host's to move
}
int smgpu_quality_constraint_pass_sweep(smgpu_handle* h) {
    if (!h) return fail("null handle");
    QualityConstraintHost& q = h->qc;
    if (!q.coupled) return fail("smgpu_quality_constraint_pass_sweep: the coupled quality constraint is not on (smgpu_set_quality_constraint_coupled)");
    if (!q.scaleCoupled) return fail("smgpu_quality_constraint_pass_sweep: the scaling passes are off (smgpu_set_quality_constraint_scaling_coupled)");
    if (q.stage != 3 || q.k < 0) return fail("smgpu_quality_constraint_pass_sweep without smgpu_quality_constraint_pass_scale");
    if (q.sweepsDue <= 0) return fail("smgpu_quality_constraint_pass_sweep: no sweep of the pass is due (nSmoothScale of them follow a marked pass, none the full revert)");
    HIP_OK(hipSetDevice(h->device));
    if (computeAfterExch(h)) return 1;          // exchange S has been enqueued by the host
    if (h->nShared > 0) {
        const int gShared = std::max(1, (int)std::min<int64_t>(q.maxGrid, ((int64_t)h->nShared + kQsBlock - 1) / kQsBlock));
        hipLaunchKernelGGL(k_qsc_combine, dim3(gShared), dim3(kQsBlock), 0, h->stream, h->nShared, (const int*)h->dSharedLocal, (const int*)h->dCombOff,
                           (const int*)h->dCombSlots, (const double*)q.scPart, (const double*)q.recvS, (const int*)q.scDeg, (const double*)q.sCur, q.sNext);
    }
    std::swap(q.sCur, q.sNext);
    --q.sweepsDue;
    if (q.sweepsDue > 0) qualityConstraintSweepHalf(h);
    HIP_OK(hipGetLastError());
    return q.sweepsDue > 0 ? checkDeviceError(h) : 0;
}
// smgpu_quality_constraint_pass_end while the scaling passes are on: a clean pass closes as before, through k_qc_close's twin;
// one with bad cells applies the scale field smgpu_quality_constraint_pass_scale and the sweeps have left
static int qualityConstraintPassEndScaled(smgpu_handle* h, int64_t nBadGlobal, int32_t* done) {
    QualityConstraintHost& q = h->qc;
    if (q.k < 0 || (q.stage != 2 && q.stage != 3)) return fail("smgpu_quality_constraint_pass_end without smgpu_quality_constraint_pass_faces");
    if (nBadGlobal < 0) return fail("smgpu_quality_constraint_pass_end: nBadGlobal < 0");
    if (nBadGlobal > 0 && q.stage != 3) return fail("smgpu_quality_constraint_pass_end: the scaling passes are on and cells are bad; smgpu_quality_constraint_pass_scale comes first");
    if (q.stage == 3 && nBadGlobal != q.scaleBad) return fail("smgpu_quality_constraint_pass_end: nBadGlobal differs from the one given to smgpu_quality_constraint_pass_scale");
    if (q.stage == 3 && q.sweepsDue > 0)
        return fail("smgpu_quality_constraint_pass_end: " + std::to_string(q.sweepsDue) + " sweeps of the pass are due (smgpu_quality_constraint_pass_sweep)");
    HIP_OK(hipSetDevice(h->device));
    smgpu_quality_constraint_record_scaled* rec = nullptr;
    if (q.slab.slot(q.slabUsed, &rec)) return 1;
    const int nP = h->mv.nPoints, total = q.scaling.scalePasses + q.prm.passes;
    const bool full = nBadGlobal > 0 && q.k == total;
    if (nBadGlobal > 0) {
        const int gPoint = std::max(1, (int)std::min<int64_t>(q.maxGrid, ((int64_t)nP + kQsBlock - 1) / kQsBlock));
        hipLaunchKernelGGL(k_qsc_open, dim3(1), dim3(64), 0, h->stream, rec);
        hipLaunchKernelGGL(k_qsc_apply, dim3(gPoint), dim3(kQsBlock), 0, h->stream, q.x, (const double*)q.L, h->st.ptsCur, (const double*)q.sCur, nP,
                           (const int*)h->dSharedSlot, (const uint8_t*)q.counted, rec);
        // points moved: the geometry smgpu_iter_ahead left for the next iteration is that of other points
        h->geomAheadDone = false;
        h->q.epoch++;
    }
    const bool close = nBadGlobal == 0 || full;
    if (close) {
        QcCounts c{};
        for (int i = 0; i < 14; ++i) c.n[i] = (long long)q.n0[i];
        hipLaunchKernelGGL(k_qsc_close, dim3(1), dim3(64), 0, h->stream, rec, (long long)(q.count + 1), q.reverting, full ? 1 : 0, c, q.nScaleRan, q.kept ? 0 : 1);
        ++q.count;
        ++q.slabUsed;
        q.k = -1;
        q.kept = false;
        q.nScaleRan = 0;
    } else ++q.k;
    q.stage = 0;
    *done = close ? 1 : 0;
    HIP_OK(hipGetLastError());
    return 0;
}
