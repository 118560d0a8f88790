// setup_tiles.hpp -- the tile sets in an engine's set-up (included into smgpu.hip): the plan of their knobs, the asynchronous build
// of one set, and one install per set -- the tables onto the device or adopted there, the sharing pass, the meta records, the view.
#pragma once

// Records a tile may stage in total: its LDS footprint, which is what sets the kernels' occupancy (the LDS is allocated in
// 512-byte steps).  Smoothing tiles of 256 points: 1 112 records of 24 bytes = 26.7 KB -- SIX workgroups per CU; the greedy pass
// otherwise reaches 512 cells + 619..623 neighbours on the large meshes = 27.2 KB and five (same box, alternating three times: gather
// kernel 335.4 -> 329.4 us on the 10 M-cell polyhedral mesh, 340.1 -> 333.0 us on hex215; the 1 M-cell block sits below by itself).
// Edge tiles of 256 edges: 852 records = 20 448 B -- EIGHT workgroups of the face-angle filter per CU instead of seven (the
// face-angle group 716 -> 705 us on the 10 M-cell mesh, the iteration 3.066 -> 3.047 ms; a tighter cap makes too many tiles: 720 us).
// largest sum over the tiles of the entries of some per-tile offset lists (a tile's staged records of all kinds)
static size_t maxTileTotal(int nTiles, std::initializer_list<const std::vector<int32_t>*> offs) {
    size_t mx = 0;
    for (int t = 0; t < nTiles; ++t) {
        size_t n = 0;
        for (const std::vector<int32_t>* o : offs) n += (size_t)((*o)[(size_t)t + 1] - (*o)[(size_t)t]);
        mx = std::max(mx, n);
    }
    return mx;
}
// Geometry tiles: 3 x points + 7 x faces doubles; 3 980 = 31 840 B -- five workgroups per CU (32 256 B each with the kernel's 48
// static bytes at the 512-byte granularity), which the kernel's 96 VGPRs (SMGPU_GEOM_WAVES = 5) allow.  A hexahedral tile of 128
// cells (~250 points, ~450 faces = 3 900) fits as it is; the polyhedral ones are cut a little earlier.
static int defaultGeomCapWeighted(int T) { return (T == 256 && SMGPU_GEOM_WAVES >= 5) ? 3980 : 0x7fffffff; }
static int defaultSmoothCapTotal(int T) { return T == 256 ? 1112 : 0x7fffffff; }
static int defaultEdgeCapTotal() { return 852; }

// The knobs of the tile sets, read here and nowhere else: the tasks, the installs, the shared-point tiles of a halo and the verbose
// lines all read the plan on the handle.
static TilePlan makeTilePlan(const smgpu_mesh_desc* d) {
    TilePlan p;
    p.wantTiles = envInt("SMGPU_TILES", 1) != 0;      // LDS staging tiles; 0 keeps the direct-gather kernels (A/B and fallback)
    p.wantFilter = envInt("SMGPU_FILTER", 1) != 0;
    p.morton = envInt("SMGPU_TILE_MORTON", 1) != 0;
    // Lattice Z-curve keys by default on meshes of hexahedra alone, bounding-box keys on the others; SMGPU_TILE_LATTICE = 1 / 0 forces
    // either on any mesh (tiles.hpp, tileLatticeKnob: the measurements behind the default)
    p.latticeKeys = tileLatticeKnob(tileLatticeDefault(d->nCells, d->nFaces, d->nInternalFaces, d->nFaces > 0 ? (int64_t)d->faceOffsets[d->nFaces] - d->faceOffsets[0] : 0));
    const int devTiles = envInt("SMGPU_DEVICE_TILES", 1);
    p.deviceTiles = devTiles == 0 ? 0 : devTiles == 2 ? 2 : 1;
    p.share = tileShareKnob();
    p.verbose = envInt("SMGPU_VERBOSE", 0);
    p.geomT = envInt("SMGPU_GEOM_T", 256);
    p.smoothT = envInt("SMGPU_SMOOTH_T", 256);
    // capacities sized for a 160 KiB LDS: a tile must leave room for >= 2 workgroups per CU
    p.geomCells = envInt("SMGPU_GEOM_CELLS", p.geomT / 2);   // cells per tile (<= threads)
    p.capGeomPoints = envInt("SMGPU_GEOM_CAPP", std::min(6 * p.geomCells, 1400));
    p.capGeomFaces = envInt("SMGPU_GEOM_CAPF", std::min(4 * p.geomCells, 1400));   // two rounds of 256 face threads at 128 cells
    p.capGeomWeighted = envInt("SMGPU_GEOM_CAPWEIGHTED", defaultGeomCapWeighted(p.geomT));
    p.capSmoothCells = envInt("SMGPU_SMOOTH_CAPC", std::min(2 * p.smoothT, 1500));
    p.capSmoothNbrs = envInt("SMGPU_SMOOTH_CAPN", std::min(3 * p.smoothT, 1500));
    p.capSmoothTotal = envInt("SMGPU_SMOOTH_CAPTOTAL", defaultSmoothCapTotal(p.smoothT));
    p.capEdgePoints = envInt("SMGPU_EDGE_CAPP", 512);
    p.capEdgeFaces = envInt("SMGPU_EDGE_CAPF", 768);
    p.capEdgeCells = envInt("SMGPU_EDGE_CAPC", 512);
    p.capEdgeTotal = envInt("SMGPU_EDGE_CAPTOTAL", defaultEdgeCapTotal());
    return p;
}

// ---- ownership of device arrays ------------------------------------------------------------------------------------------------------
// The handle takes an array over: onto its allocation list, into its byte count, and out of the source -- which whoever releases
// the source's struct afterwards finds empty.
template <class T>
static void adopt(smgpu_handle* h, T*& dst, DevArr& a) {
    dst = (T*)a.p; h->allocs.push_back(a.p); h->deviceBytes += (int64_t)a.bytes;
    a = DevArr();
}
// what a struct of device arrays still owns (DeviceTopologyArrays, GeomTilesDev, SmoothTilesDev, EdgeTilesDev)
template <class Arrays>
static void releaseOwned(Arrays& arrays) {
    arrays.each([](DevArr& a) { if (a.p) (void)hipFree(a.p); a = DevArr(); });
    arrays.valid = false;
}
// one array of a table set onto the handle: a device build's stays where it is, a host build's is uploaded
template <class T, class U>
static int place(smgpu_handle* h, bool onDevice, const T*& dst, DevArr& a, const std::vector<U>& host) {
    if (!onDevice) return devUpload(h, &dst, host);
    adopt(h, dst, a);
    return 0;
}

// ---- the asynchronous build of one tile set --------------------------------------------------------------------------------------------
enum class TileTables { ready, hostPending, notBuilt, failed };      // hostPending: a device build of the addressing that leaves this
                                                                     // set's tables to the host, whose lists are still arriving
// boundaries() -> error text; onDevice(why) -> 0 built, 1 handed back, 2 a HIP error; onHost() -> error text.  `lists`: the
// addressing's device arrays, valid where it was built there.
template <class Boundaries, class OnDevice, class OnHost>
static std::future<TileTables> startTileTask(const char* name, const TilePlan& plan, const DeviceTopologyArrays& lists, Boundaries boundaries, OnDevice onDevice, OnHost onHost) {
    return std::async(std::launch::async, [name, &plan, &lists, boundaries, onDevice, onHost] {
        if (!boundaries().empty()) return TileTables::failed;
        if (!lists.valid) return onHost().empty() ? TileTables::ready : TileTables::failed;
        if (plan.deviceTiles == 0) return TileTables::hostPending;
        std::string why;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = plan.deviceTiles == 2 ? 1 : onDevice(why);
        if (plan.verbose >= 2)
            std::fprintf(stderr, "[smgpu] %s tiles: tables on the %s %.2f s   (done at +%.3f s)\n", name, rc == 0 ? "device" : "host (device build handed them back)",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), setupClock());
        return rc == 0 ? TileTables::ready : rc == 2 ? TileTables::failed : TileTables::hostPending;
    });
}
// a task's verdict; tables left to the host are built now (onHost() -> error text).  A set that fails is done without, whatever the
// reason: the callers fall back to kernels that need no tiles.
template <class OnHost>
static bool tileTablesStand(std::future<TileTables>& f, OnHost onHost) {
    const TileTables s = f.valid() ? f.get() : TileTables::notBuilt;
    return s == TileTables::ready || (s == TileTables::hostPending && onHost().empty());
}

// ---- one install per tile set ------------------------------------------------------------------------------------------------------------
// Shared topology blocks (tiles.hpp): tiles whose rows are byte-identical read the first copy.  The pass runs on the tables of
// whichever side built them (a device build's rows are hashed and compared where they are, tiles_dev.hip) and only changes the
// bases in the meta records.  (one array of a device build: lenOf(t) entries at the tile's base)
template <class LenOf>
static int shareOnDevice(smgpu_handle* h, TileShare& out, int nT, const uint16_t* a, const uint16_t* b, const std::vector<int32_t>& base, const std::vector<uint8_t>& width, LenOf lenOf) {
    std::vector<int32_t> len((size_t)nT), key(width.begin(), width.end());
    for (int t = 0; t < nT; ++t) len[(size_t)t] = (int32_t)lenOf(t);
    std::string why;
    return shareBlocksOnDevice(nT, a, b, base, len, key, h->device, out, why) ? fail("smgpu_create: shared tile blocks: " + why) : 0;
}
static int putMeta(smgpu_handle* h, const int*& dst, const std::vector<int>& meta) {      // a device build's records are overwritten in place
    if (!dst) return devUpload(h, &dst, meta);
    if (!meta.empty() && hipMemcpy((void*)dst, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail("smgpu_create: upload of the tile records failed");
    return 0;
}

// SMGPU_VERBOSE=1, per tile set: tiles, distinct blocks per array (= tiles where every tile reads its own), staged elements per
// element of the mesh
static int installGeomTiles(smgpu_handle* h) {
    const TilePlan& plan = h->plan;
    const GeomTiles& gt = h->gt;
    GeomTilesDev& dev = h->gtDev;
    GeomTileView& g = h->gv;
    const bool onDev = dev.valid;
    int rc = 0;
    rc |= place(h, onDev, g.cellOrder, dev.cellOrder, gt.order); rc |= place(h, onDev, g.cellBeg, dev.cellBeg, gt.cellBeg);
    rc |= place(h, onDev, g.tpIds, dev.tpIds, gt.tpIds); rc |= place(h, onDev, g.tfIds, dev.tfIds, gt.tfIds);
    rc |= place(h, onDev, g.faceVerts, dev.faceVerts, gt.faceVerts); rc |= place(h, onDev, g.cellFaces, dev.cellFaces, gt.cellFaces);
    if (onDev) adopt(h, g.meta, dev.meta);
    dev.valid = false;
    rc |= devUpload(h, &g.tpOff, gt.tpOff); rc |= devUpload(h, &g.tfOff, gt.tfOff); rc |= devUpload(h, &g.fvBase, gt.fvBase); rc |= devUpload(h, &g.fvWidth, gt.fvWidth);
    rc |= devUpload(h, &g.cfBase, gt.cfBase); rc |= devUpload(h, &g.cfWidth, gt.cfWidth); rc |= devUpload(h, &g.tileFlags, gt.tileFlags);
    if (rc) return 1;
    int dFv = gt.nTiles, dCf = gt.nTiles;
    if (!g.meta || plan.share) {
        TileShare fv, cf;
        if (gt.faceVerts.empty() && g.faceVerts) {
            if (shareOnDevice(h, fv, gt.nTiles, g.faceVerts, nullptr, gt.fvBase, gt.fvWidth, [&](int t) { return (size_t)(gt.tfOff[(size_t)t + 1] - gt.tfOff[(size_t)t]) * gt.fvWidth[(size_t)t]; }) ||
                shareOnDevice(h, cf, gt.nTiles, g.cellFaces, nullptr, gt.cfBase, gt.cfWidth, [&](int t) { return (size_t)gt.cfWidth[(size_t)t] * (size_t)gt.threads; })) return 1;
        } else shareGeomBlocks(gt, gt.faceVerts.data(), gt.cellFaces.data(), fv, cf);
        if (putMeta(h, g.meta, gt.metaRecords(&fv, &cf))) return 1;
        dFv = fv.distinct; dCf = cf.distinct;
    }
    if (plan.verbose)
        std::fprintf(stderr, "[smgpu] geometry tiles: %d tiles, distinct blocks: faceVerts %d, cellFaces %d (SMGPU_TILE_LATTICE=%d SMGPU_TILE_SHARE=%d), staged faces x%.4f, "
                     "staged points x%.4f\n", gt.nTiles, dFv, dCf, (int)gt.latticeKeys, (int)plan.share, (double)gt.tfOff.back() / std::max(1, h->topo.nFaces),
                     (double)gt.tpOff.back() / std::max(1, h->topo.nPoints));
    g.maxPoints = gt.maxPoints; g.maxFaces = gt.maxFaces;
    return 0;
}

// The regular smoothing tiles (smgpu_create), or the tiles over the shared points of a halo (smgpu_halo_configure): those take no
// sharing pass and print no line of their own.
static int installSmoothTiles(smgpu_handle* h, const SmoothTiles& st, SmoothTilesDev& dev, SmoothTileView& v, int usePairShare, bool regular) {
    const TilePlan& plan = h->plan;
    const bool onDev = dev.valid;
    int rc = 0;
    rc |= place(h, onDev, v.ptOrder, dev.order, st.order); rc |= place(h, onDev, v.ptBeg, dev.ptBeg, st.ptBeg); rc |= place(h, onDev, v.tcIds, dev.tcIds, st.tcIds);
    rc |= place(h, onDev, v.tnIds, dev.tnIds, st.tnIds); rc |= place(h, onDev, v.selfLoc, dev.selfLoc, st.selfLoc); rc |= place(h, onDev, v.pcEll, dev.pcEll, st.pcEll);
    rc |= place(h, onDev, v.ppEll, dev.ppEll, st.ppEll); rc |= place(h, onDev, v.pairEll, dev.pairEll, st.pairEll); rc |= place(h, onDev, v.pfEll, dev.pfEll, st.pfEll);
    if (onDev) adopt(h, v.meta, dev.meta);
    dev.valid = false;
    rc |= devUpload(h, &v.tcOff, st.tcOff); rc |= devUpload(h, &v.tnOff, st.tnOff); rc |= devUpload(h, &v.pcBase, st.pcBase); rc |= devUpload(h, &v.pcWidth, st.pcWidth);
    rc |= devUpload(h, &v.ppBase, st.ppBase); rc |= devUpload(h, &v.ppWidth, st.ppWidth); rc |= devUpload(h, &v.pfBase, st.pfBase);
    rc |= devUpload(h, &v.pfWidth, st.pfWidth);
    if (rc) return 1;
    int dPc = st.nTiles, dPp = st.nTiles, dPf = st.nTiles;
    if (!v.meta || (regular && plan.share)) {
        TileShare pc, pp, pf;
        if (regular && st.pcEll.empty() && v.pcEll) {
            const size_t T = (size_t)st.threads;
            if (shareOnDevice(h, pc, st.nTiles, v.pcEll, nullptr, st.pcBase, st.pcWidth, [&](int t) { return st.pcWidth[(size_t)t] * T; }) ||
                shareOnDevice(h, pp, st.nTiles, v.ppEll, v.pairEll, st.ppBase, st.ppWidth, [&](int t) { return st.ppWidth[(size_t)t] * T; }) ||
                shareOnDevice(h, pf, st.nTiles, v.pfEll, nullptr, st.pfBase, st.pfWidth, [&](int t) { return st.pfWidth[(size_t)t] * T; })) return 1;
        } else if (regular) shareSmoothBlocks(st, st.pcEll.data(), st.ppEll.data(), st.pairEll.data(), st.pfEll.data(), pc, pp, pf);
        if (putMeta(h, v.meta, st.metaRecords(&pc, &pp, &pf))) return 1;
        if (regular) { dPc = pc.distinct; dPp = pp.distinct; dPf = pf.distinct; }
    }
    if (regular && plan.verbose)
        std::fprintf(stderr, "[smgpu] smoothing tiles: %d tiles, distinct blocks: pcEll %d, ppEll+pairEll %d, pfEll %d, staged cell centres x%.4f, staged points x%.4f (per point)\n",
                     st.nTiles, dPc, dPp, dPf, (double)st.tcOff.back() / std::max(1, h->topo.nPoints), (double)st.tnOff.back() / std::max(1, h->topo.nPoints));
    v.maxCells = st.maxCells; v.maxPoints = st.maxPoints;
    v.usePairShare = usePairShare;
    return 0;
}

// The edge tiles of the face-angle filter, behind the geometry tiles: the filter reads the face averages where those store them,
// so the tiles' face ids become positions in the face list of the face's owner's tile.  Then the filter's side stream.
static int installEdgeTiles(smgpu_handle* h) {
    const TilePlan& plan = h->plan;
    EdgeTiles& et = h->etl;
    EdgeTilesDev& dev = h->etDev;
    EdgeTileView& ev = h->ev;
    const Topology& t = h->topo;
    const size_t nGeomTf = (size_t)h->gt.tfOff.back();
    h->avgPackedCount = nGeomTf;
    const bool onDev = dev.valid;
    if (onDev) {      // a device build: the remap there too, the tables stay where they are
        std::string why;
        if (remapEdgeFaceIdsOnDevice(h->gv.tfIds, (long long)nGeomTf, t.nFaces, (int*)dev.tfIds.p, dev.nTf, h->device, why)) return fail("smgpu_create: edge tile face positions: " + why);
    } else {
        if (h->gt.tfIds.size() != nGeomTf) {      // (a device build of the geometry tables that kept its face ids there)
            h->gt.tfIds.resize(nGeomTf);
            if (hipMemcpy(h->gt.tfIds.data(), h->gv.tfIds, nGeomTf * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("smgpu_create: download of the tile face ids failed");
        }
        std::vector<int32_t> facePos((size_t)t.nFaces, -1);
        for (size_t k = 0; k < h->gt.tfIds.size(); ++k)
            if (h->gt.tfIds[k] < 0) facePos[(size_t)(h->gt.tfIds[k] & 0x7fffffff)] = (int32_t)k;
        for (int32_t& f : et.tfIds) f = facePos[(size_t)f];
    }
    int rc = 0;
    rc |= place(h, onDev, ev.order, dev.order, et.order); rc |= place(h, onDev, ev.edgeBeg, dev.edgeBeg, et.edgeBeg);
    rc |= place(h, onDev, ev.tpIds, dev.tpIds, et.tpIds); rc |= place(h, onDev, ev.tfIds, dev.tfIds, et.tfIds); rc |= place(h, onDev, ev.tcIds, dev.tcIds, et.tcIds);
    rc |= place(h, onDev, ev.epLoc, dev.epLoc, et.epLoc); rc |= place(h, onDev, ev.efEll, dev.efEll, et.efEll); rc |= place(h, onDev, ev.ecEll, dev.ecEll, et.ecEll);
    if (onDev) adopt(h, ev.meta, dev.meta);
    dev.valid = false;
    rc |= devUpload(h, &ev.tpOff, et.tpOff); rc |= devUpload(h, &ev.tfOff, et.tfOff); rc |= devUpload(h, &ev.tcOff, et.tcOff); rc |= devUpload(h, &ev.efBase, et.efBase);
    rc |= devUpload(h, &ev.ecBase, et.ecBase); rc |= devUpload(h, &ev.efWidth, et.efWidth); rc |= devUpload(h, &ev.ecWidth, et.ecWidth);
    if (rc) return 1;
    int dEf = et.nTiles, dEc = et.nTiles;
    if (!ev.meta || plan.share) {
        TileShare ef, ec;
        if (et.efEll.empty() && ev.efEll) {
            const size_t T = (size_t)et.threads;
            if (shareOnDevice(h, ef, et.nTiles, ev.efEll, nullptr, et.efBase, et.efWidth, [&](int ti) { return et.efWidth[(size_t)ti] * T; }) ||
                shareOnDevice(h, ec, et.nTiles, ev.ecEll, nullptr, et.ecBase, et.ecWidth, [&](int ti) { return et.ecWidth[(size_t)ti] * T; })) return 1;
        } else shareEdgeBlocks(et, et.efEll.data(), et.ecEll.data(), ef, ec);
        if (putMeta(h, ev.meta, et.metaRecords(&ef, &ec))) return 1;
        dEf = ef.distinct; dEc = ec.distinct;
    }
    if (plan.verbose)
        std::fprintf(stderr, "[smgpu] edge tiles: %d tiles, distinct blocks: efEll %d, ecEll %d, staged points x%.4f, faces x%.4f, cells x%.4f (per edge)\n", et.nTiles, dEf, dEc,
                     (double)et.tpOff.back() / std::max(1, t.nEdges), (double)et.tfOff.back() / std::max(1, t.nEdges), (double)et.tcOff.back() / std::max(1, t.nEdges));
    ev.maxPoints = et.maxPoints; ev.maxFaces = et.maxFaces; ev.maxCells = et.maxCells;
    h->edgeLds = sizeof(double) * 3 * maxTileTotal(et.nTiles, {&et.tpOff, &et.tfOff, &et.tcOff});
    h->edgeTilesOk = h->edgeLds <= 64 * 1024;
    if (plan.verbose)
        std::fprintf(stderr, "[smgpu] edge tiles: n=%d LDS=%zu B (maxP %d maxF %d maxC %d)\n", et.nTiles, h->edgeLds, ev.maxPoints, ev.maxFaces, ev.maxCells);
    if (h->edgeTilesOk && envInt("SMGPU_SIDE_STREAM", sideStreamDefault(t.nPoints))) {
        if (depInit(h)) return 1;
        if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->evFork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->evJoin, hipEventDisableTiming) != hipSuccess)
            return fail("side stream creation failed");
    }
    return 0;
}
