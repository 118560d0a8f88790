// setup_create.hpp -- the stages of smgpu_create (included into smgpu.hip): what is in flight while an engine is set up and who
// frees it, the start of the tile tasks beside the addressing, the installs of the addressing and of the tile sets, the work arrays.
#pragma once

// What a create has in flight: the host threads that build the tile tables (they read the handle's tables), the corner chains
// (tiles_dev.hip; taken over by the smoothing task's device build, or released here) and the arrays of a device build of the
// addressing until the handle adopts them.  The destructor joins every task, then frees what the handle has not taken over -- owner /
// neighbour never join the handle: only the device builds of the tile tables read them.
struct SetupTasks {
    std::vector<int32_t> pointOrder;      // the Z-curve of the points, once fetched (smoothing and edge tiles)
    std::future<std::vector<int32_t>> fPointOrder;
    std::future<TileTables> geom, smooth, edge;
    CornerChains chains;
    DeviceTopologyArrays owned;
    void fetchPointOrder() { if (fPointOrder.valid()) pointOrder = fPointOrder.get(); }
    void join() {
        if (fPointOrder.valid()) fPointOrder.wait();
        for (std::future<TileTables>* f : {&geom, &smooth, &edge}) if (f->valid()) f->wait();
    }
    ~SetupTasks() { join(); releaseCornerChains(chains); releaseOwned(owned); }
};
// The one-off host work is pipelined: the Z-curve of the points (needs the coordinates only) starts at once; the geometry tile
// tables start as soon as the cell -> face lists stand (the addressing's afterCells hook) and are built next to the rest of the
// addressing, the corner chains of the smoothing tables beside them; the smoothing tables from afterPoints; the edge tables (face-angle
// filter) behind the edge lists of a device build (its afterEdges hook), else behind the addressing.  Tile boundaries on the host,
// the tables on the device where the addressing was built there (tiles_dev.hip), else on the host.
static int startTasksAndAddressing(smgpu_handle* h, const smgpu_mesh_desc* d, SetupTasks& tasks) {
    const TilePlan& plan = h->plan;
    const DeviceTopologyArrays& lists = h->devLists;      // (what the tasks read; tasks.owned holds the ownership)
    h->gt.latticeKeys = h->stl.latticeKeys = h->etl.latticeKeys = plan.latticeKeys;
    if (plan.wantTiles && plan.morton) tasks.fPointOrder = std::async(std::launch::async, [d, &plan] { return mortonOrderOf(d->nPoints, d->points, plan.latticeKeys); });
    const std::vector<int32_t>* po = &tasks.pointOrder;
    const auto afterCells = [&] {
        if (!plan.wantTiles || !plan.shapesOk()) return;
        // (the corner chains need the device addressing only: started here, they run beside the rest of the download and the host's
        // boundary passes)
        if (plan.deviceTiles == 1 && lists.valid) {
            std::string why;
            if (startCornerChains(lists, d->nPoints, h->device, tasks.chains, why) == 2) tasks.chains = CornerChains();
        }
        tasks.geom = startTileTask("geometry", plan, lists,
            [h, d, &plan, &lists] {
                std::vector<int32_t> cellOrder;      // (a device build: the Z-curve of the cells there too -- the order the host would find)
                if (plan.morton && plan.deviceTiles == 1 && lists.valid) {
                    std::string why;
                    if (cellMortonOrderOnDevice(lists, d->nCells, d->nPoints, d->points, h->device, cellOrder, why, plan.latticeKeys) != 0) cellOrder.clear();
                }
                return h->gt.buildBoundaries(h->topo, d->points, plan.morton, plan.geomT, plan.geomCells, plan.capGeomPoints, plan.capGeomFaces, plan.capGeomWeighted,
                                             SMGPU_GEOM_AOS ? kGF : 6, cellOrder.empty() ? nullptr : &cellOrder);
            },
            [h, d, &lists](std::string& why) { return buildGeomTablesOnDevice(h->gt, lists, d->nCells, h->device, h->gtDev, why); },
            [h] { return h->gt.buildTables(h->topo); });
    };
    const auto afterPoints = [&] {
        if (!plan.wantTiles || !plan.shapesOk()) return;
        tasks.fetchPointOrder();
        h->isInternalHost.resize((size_t)d->nPoints);
        for (int p = 0; p < d->nPoints; ++p) h->isInternalHost[(size_t)p] = d->isInternalPoint[p] ? 1 : 0;
        tasks.smooth = startTileTask("smoothing", plan, lists,
            [h, d, &plan, po] {
                return h->stl.buildBoundaries(h->topo, d->points, plan.morton, plan.smoothT, plan.capSmoothCells, plan.capSmoothNbrs, (plan.morton && !po->empty()) ? po : nullptr, nullptr,
                                              plan.capSmoothTotal);
            },
            [h, d, &lists, chains = &tasks.chains](std::string& why) {
                return buildSmoothTablesOnDevice(h->stl, lists, d->nPoints, h->topo.maxPointPoints, h->isInternalHost.data(), h->device, h->stDev, why, chains);
            },
            [h] { return h->stl.buildTables(h->topo, h->isInternalHost.data()); });
    };
    const std::function<void()> startEdge = [&] {
        if (!plan.wantTiles || !plan.wantFilter || tasks.edge.valid()) return;
        tasks.fetchPointOrder();
        tasks.edge = startTileTask("edge", plan, lists,
            [h, d, &plan, po] {
                return h->etl.buildBoundaries(h->topo, d->points, plan.morton, 256, plan.capEdgePoints, plan.capEdgeFaces, plan.capEdgeCells, (plan.morton && !po->empty()) ? po : nullptr,
                                              plan.capEdgeTotal);
            },
            [h, &lists](std::string& why) { return buildEdgeTablesOnDevice(h->etl, lists, h->topo.nEdges, h->device, h->etDev, why); },
            [h] { return h->etl.buildTables(h->topo); });
    };
    // the addressing on the device (topology_dev.hip: sorts + per-edge kernels, ~0.2 s for 10 M cells against 3.5 s of host
    // loops); the host build where the device path hands the mesh back (unusual meshes; it also words the reference's errors)
    int dev = envInt("SMGPU_DEVICE_TOPOLOGY", 1) ? 1 : -1;
    if (dev > 0) {
        std::string why;
        dev = buildTopologyOnDevice(h->topo, d->nPoints, d->nCells, d->nFaces, d->nInternalFaces, d->faceOffsets, d->facePoints, d->owner, d->neighbour, h->device, why,
                                    afterCells, afterPoints, &h->devLists, startEdge, plan.deviceTiles != 0 && plan.wantTiles);
        tasks.owned = h->devLists;      // (a failed device build included: the arrays it had already handed over)
        if (dev == 2) return fail("smgpu_create: device addressing: " + why);
        if (plan.verbose >= 1) std::fprintf(stderr, "[smgpu] addressing on the %s (%.2f s since create)\n", dev == 0 ? "device" : "host (device path handed the mesh back)", setupClock());
    }
    if (dev != 0) {
        h->topo = Topology();
        const std::string terr = h->topo.build(d->nPoints, d->nCells, d->nFaces, d->nInternalFaces, d->faceOffsets, d->facePoints, d->owner, d->neighbour, afterCells, afterPoints);
        if (!terr.empty()) return fail("smgpu_create: " + terr);
    }
    startEdge();
    return 0;
}

// the addressing on the device: a device build's own arrays (topology_dev.hip), else uploads of the host build's lists
static int installAddressing(smgpu_handle* h, const smgpu_mesh_desc* d, SetupTasks& tasks) {
    const Topology& t = h->topo;
    MeshView& m = h->mv;
    m.nPoints = t.nPoints; m.nCells = t.nCells; m.nFaces = t.nFaces; m.nInternalFaces = t.nInternalFaces; m.nEdges = t.nEdges;
    std::vector<uint8_t> flags(t.nPoints);
    for (int p = 0; p < t.nPoints; ++p)
        flags[p] = (d->isInternalPoint[p] ? PF_INTERNAL : 0) |
                   ((d->isSmoothingSurfacePoint && d->isSmoothingSurfacePoint[p]) ? PF_SMOOTHSURF : 0);
    int rc = 0;
    const bool onDev = tasks.owned.valid;
#define SMGPU_X(name, list) rc |= place(h, onDev, m.name, tasks.owned.name, t.list);
    SMGPU_ADDRESSING(SMGPU_X)
#undef SMGPU_X
    rc |= devUpload(h, &m.pflags, flags);
    return rc;
}

// the knobs of the loop that are read once per engine
static void readLoopKnobs(smgpu_handle* h) {
    h->useTiles = h->plan.wantTiles;
    h->useFilter = h->plan.wantFilter;
    h->xcdMap = envInt("SMGPU_XCD_MAP", 1) != 0;
    h->walkStar = envInt("SMGPU_WALK_STAR", 1) != 0;
    h->starBlocks = std::max(1, envInt("SMGPU_STAR_BLOCKS", 256 * 32));
    h->walkPack = envInt("SMGPU_WALK_PACK", 1) != 0;
    h->walkCache = envInt("SMGPU_WALK_CACHE", 1) != 0;
    h->faLists = envInt("SMGPU_FA_LISTS", 1) != 0;
    h->faSideExact = envInt("SMGPU_FA_SIDE_EXACT", 1) != 0;
    h->bndInGeom = envInt("SMGPU_BND_IN_GEOM", 1) != 0;
    h->qt.fusedWanted = envInt("SMGPU_QUALITY_TRACE_FUSED", 1) != 0;
    { const char* fv = std::getenv("SMGPU_FOAM_VARIANT"); h->foamOrg = fv && std::string(fv) == "org"; }
    { const char* sv = std::getenv("SMGPU_SYNC_VARIANT"); h->st.ownFold = (sv && std::string(sv) == "own") ? 1 : 0; }
}

// Joins the three tile tasks and installs their tables.  A set the builders refuse (meshes with huge cells / valences) turns the
// tiles off: the direct-gather kernels still apply.
static int installTiles(smgpu_handle* h, SetupTasks& tasks, double tTopo, const std::function<void(const char*)>& lap) {
    const TilePlan& plan = h->plan;
    h->geomT = plan.geomT;
    h->smoothT = plan.smoothT;
    if (!TilePlan::shapeOk(plan.geomT)) return fail("SMGPU_GEOM_T must be 64, 128 or 256");
    if (!TilePlan::shapeOk(plan.smoothT)) return fail("SMGPU_SMOOTH_T must be 64, 128 or 256");
    tasks.join();
    // (a device build that handed a table set back: the host builds it now that all of its lists have arrived)
    auto fetched = [&](int groups) { std::string why; return downloadDeferredLists(h->topo, h->devLists, h->device, why, groups) == 0; };
    const bool geomOk = tileTablesStand(tasks.geom, [&] { return h->gt.buildTables(h->topo); });
    const bool smoothOk = tileTablesStand(tasks.smooth, [&] { return fetched(1) ? h->stl.buildTables(h->topo, h->isInternalHost.data()) : std::string("no lists"); });
    const bool edgeOk = tileTablesStand(tasks.edge, [&] { return fetched(2) ? h->etl.buildTables(h->topo) : std::string("no lists"); });
    if (plan.verbose) std::fprintf(stderr, "[smgpu] set-up: addressing %.2f s, tile tables (3 host threads) %.2f s\n", tTopo, setupClock() - tTopo);
    releaseOwned(tasks.owned);      // owner / neighbour: their readers are all joined now (4 (nFaces + nInternalFaces) bytes)
    lap("tile tasks joined");
    if (!geomOk || !smoothOk) { h->useTiles = false; return 0; }
    if (installGeomTiles(h)) return 1;
    if (installSmoothTiles(h, h->stl, h->stDev, h->sv, h->topo.maxPointPoints <= 16 ? 1 : 0, true)) return 1;
    if (h->useFilter && edgeOk && installEdgeTiles(h)) return 1;
    {   // the largest footprint of one tile (geomLds lays the arrays out by the tile's own counts)
        size_t mx = 0;
        for (int ti = 0; ti < h->gt.nTiles; ++ti)
            mx = std::max(mx, 3 * (size_t)(h->gt.tpOff[(size_t)ti + 1] - h->gt.tpOff[(size_t)ti]) +
                                  (size_t)(SMGPU_GEOM_AOS ? kGF : 6) * (size_t)(h->gt.tfOff[(size_t)ti + 1] - h->gt.tfOff[(size_t)ti]));
        h->geomLds = sizeof(double) * mx;
    }
    h->smoothLds = sizeof(double) * 3 * maxTileTotal(h->stl.nTiles, {&h->stl.tcOff, &h->stl.tnOff});
    if (plan.verbose)
        std::fprintf(stderr, "[smgpu] tiles: geom T=%d n=%d LDS=%zu B (maxP %d maxF %d; staged faces x%.3f, points x%.3f of the mesh's)  smooth T=%d n=%d LDS=%zu B (maxC %d maxN %d)\n",
                     h->geomT, h->gt.nTiles, h->geomLds, h->gv.maxPoints, h->gv.maxFaces, (double)h->gt.tfOff.back() / std::max(1, h->topo.nFaces),
                     (double)h->gt.tpOff.back() / std::max(1, h->topo.nPoints), h->smoothT, h->stl.nTiles, h->smoothLds, h->sv.maxCells, h->sv.maxPoints);
    return 0;
}

// the wave-cooperative edge-angle kernel stages the entries of kEaPointsPerBlock points (SMGPU_EDGE_ANGLE=faithful: the per-angle acos form)
static void sizeEdgeAngle(smgpu_handle* h) {
    const Topology& t = h->topo;
    const char* ea = std::getenv("SMGPU_EDGE_ANGLE");
    h->eaCoop = !(ea && std::string(ea) == "faithful");
    for (int p0 = 0; p0 < t.nPoints; p0 += kEaPointsPerBlock) {
        const int p1 = std::min(t.nPoints, p0 + kEaPointsPerBlock);
        h->eaMaxEntries = std::max(h->eaMaxEntries, t.pointEdges.off[p1] - t.pointEdges.off[p0]);
    }
    if (sizeof(double) * 9 * (size_t)h->eaMaxEntries > 60 * 1024) h->eaCoop = false;   // extreme valences: per-point form
}

static int allocWorkArrays(smgpu_handle* h) {
    const Topology& t = h->topo;
    State& s = h->st;
    const size_t P = t.nPoints, C = t.nCells, F = t.nFaces, E = t.nEdges;
    int rc = 0;
    rc |= devAlloc(h, &h->bufA, 3 * P);
    rc |= devAlloc(h, &h->bufB, 3 * P);
    rc |= devAlloc(h, &s.prop, 3 * P);
    rc |= devAlloc(h, &h->dStepSqr, P + 4);
    rc |= devAlloc(h, &s.fCtr, 3 * F);
    rc |= devAlloc(h, &s.fArea, 3 * F);
    s.avgPacked = (h->useTiles && h->edgeTilesOk && h->avgPackedCount) ? 1 : 0;
    rc |= devAlloc(h, &s.fAvg, 3 * (s.avgPacked ? h->avgPackedCount : F));
    rc |= devAlloc(h, &s.cellCtr, 3 * C);
    rc |= devAlloc(h, &s.frozen, P);
    rc |= devAlloc(h, &s.edgeMin, E);
    rc |= devAlloc(h, &s.edgeMax, E);
    rc |= devAlloc(h, &s.ptMin, P);
    rc |= devAlloc(h, &s.ptMax, P);
    rc |= devAlloc(h, &s.faActive, P + 16);    // + 16: the compaction kernels read the marks 16 bytes at a time (chunkMarks)
    rc |= devAlloc(h, &h->dFaMaybe, P + 16);
    rc |= devAlloc(h, &s.faEdgeList, E);
    rc |= devAlloc(h, &s.faPointList, P);
    rc |= devAlloc(h, &h->dEaMaybe, P);
    rc |= devAlloc(h, &s.faS, P);
    rc |= devAlloc(h, &s.faN, t.pointPoints.size());
    rc |= devAlloc(h, &s.walkStack, P + 64);
    rc |= devAlloc(h, &s.acc, 1);
    rc |= devAlloc(h, &s.nearTotal, 4);
    // + the boundary points' partials when k_bnd_fix finishes them (smgpu_set_boundary_smoothing)
    const size_t nPart = (size_t)std::max(gridFor(t.nPoints), h->useTiles ? h->stl.nTiles : 0) + 2 * (size_t)gridFor(t.nPoints) + 1;
    rc |= devAlloc(h, &s.blkMax, nPart);
    rc |= devAlloc(h, &s.blkCnt, nPart);
    return rc;
}

static int uploadPoints(smgpu_handle* h, const smgpu_mesh_desc* d) {
    State& s = h->st;
    const size_t P = (size_t)h->topo.nPoints;
    if (hipMemset(s.acc, 0, sizeof(Accum)) != hipSuccess) return fail("hipMemset failed");
    if (hipMemsetAsync(s.nearTotal, 0, 4 * sizeof(unsigned long long), h->stream) != hipSuccess) return fail("hipMemset failed");
    if (hipMemset(s.frozen, 0, P) != hipSuccess) return fail("hipMemset failed");
    if (hipMemcpy(h->bufA, d->points, 3 * P * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail("upload of points failed");
    if (hipMemcpy(s.prop, h->bufA, 3 * P * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess) return fail("upload of points failed");
    s.ptsCur = h->bufA;
    s.ptsNext = h->bufB;
    s.stats = nullptr;
    s.sharedSlot = nullptr;
    s.combA = nullptr;
    return 0;
}

// the word through which the GPU tells the host how busy the face-angle walk is (updateWalkMode)
static void mapWalkWord(smgpu_handle* h) {
    void* dp = nullptr;
    if (hipHostMalloc((void**)&h->nActiveHost, 64, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(&dp, h->nActiveHost, 0) == hipSuccess) {
        *(volatile int*)h->nActiveHost = -1;
        h->st.nActiveHost = (int*)dp;
    } else {
        (void)hipGetLastError();
        if (h->nActiveHost) (void)hipHostFree(h->nActiveHost);
        h->nActiveHost = nullptr;
        h->st.nActiveHost = nullptr;      // the replay form then stays as first decided
    }
}
