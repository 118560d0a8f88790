// quality_reports.hpp -- the mesh quality reports (include/smgpu.h smgpu_mesh_quality*, smgpu_quality_*; DESIGN.md "Mesh quality"):
// three kinds, their per-element fields and sets, serial and coupled.  Host code; included by smgpu.hip once, inside its
// extern "C", behind runGeometry.  State: smgpu_handle::q (quality_state.hpp).
// ---- mesh quality report (kernels_quality.hpp) ------------------------------------------------------------------------------
// the report's device memory, on the first call: owner / neighbour by face (derived on the device from the cell -> face rows),
// the two partial slabs and the report
static int qualityEnsure(smgpu_handle* h) {
    QualityReportHost& q = h->q;
    if (q.base.live()) return 0;
    const MeshView& m = h->mv;
    const size_t nFB = (size_t)std::max(1, qualityGrid(m.nFaces)), nCB = (size_t)std::max(1, qualityGrid(m.nCells));
    if (q.base.alloc(&q.own, (size_t)std::max(1, m.nFaces)) || q.base.alloc(&q.nei, (size_t)std::max(1, m.nInternalFaces)) ||
        q.base.alloc(&q.facePart, nFB) || q.base.alloc(&q.cellPart, nCB) || q.base.alloc(&q.out, 1))
        return q.base.failed("the report");
    HIP_OK(hipMemsetAsync(h->q.own, 0, sizeof(int) * (size_t)std::max(1, m.nFaces), h->stream));   // (every face has an owner row; no
    HIP_OK(hipMemsetAsync(h->q.nei, 0, sizeof(int) * (size_t)std::max(1, m.nInternalFaces), h->stream));   //  id is left undefined)
    if (m.nCells > 0) hipLaunchKernelGGL(k_quality_owners, dim3(gridFor(m.nCells)), dim3(kQualityBlock), 0, h->stream, m, h->q.own, h->q.nei);
    HIP_OK(hipGetLastError());
    return 0;
}

static const char* kQualityHaloRefusal = "mesh quality: not available on an engine with a halo (a sub-domain's processor faces are internal faces of "
                                         "the global mesh, whose neighbour cell centres this report does not exchange); report on the undecomposed mesh, or use "
                                         "smgpu_quality_coupled_pack / _report";
// while one lives, what the engine launches stays outside its launch counters and timing events
class Uncounted {
    smgpu_handle* h;
    bool timing;
    int64_t launches[K_COUNT];
  public:
    explicit Uncounted(smgpu_handle* handle) : h(handle), timing(handle->timing) { std::memcpy(launches, h->launches, sizeof(launches)); h->timing = false; }
    Uncounted(const Uncounted&) = delete;
    Uncounted& operator=(const Uncounted&) = delete;
    ~Uncounted() { h->timing = timing; std::memcpy(h->launches, launches, sizeof(launches)); }
};
// the loop's geometry launch with writeFaces, uncounted
static int qualityGeometry(smgpu_handle* h) {
    Uncounted scope(h);
    h->writeFaces = true;
    // a loop that relTol stopped leaves its stop word set until the next smgpu_iterate clears it, and the geometry kernels return at
    // once on that word: the report would be one of the face values and cell centres of the last iteration's start
    HIP_OK(hipMemsetAsync(&h->st.acc->stop, 0, sizeof(int), h->stream));
    const int rcg = runGeometry(h);
    h->writeFaces = false;
    return rcg;
}
// start of a serial call: the refusal with a halo, the memory of its report kind, the geometry of the current points
static int qualitySerialBegin(smgpu_handle* h, int (*ensure)(smgpu_handle*)) {
    if (h->haloOn) return fail(kQualityHaloRefusal);
    HIP_OK(hipSetDevice(h->device));
    if (ensure(h)) return 1;
    return qualityGeometry(h);
}
static QualityThresholds qualityThresholds(const smgpu_quality_params* p) {
    const smgpu_quality_params prm = p ? *p : smgpu_quality_params{70.0, 4.0, 1e-6, 1000.0};
    return QualityThresholds{std::cos(prm.nonOrthThreshold * (SMGPU_PI / 180.0)), prm.skewThreshold, prm.closedThreshold, prm.aspectThreshold};
}
static QualityGeomThresholds geomThresholds(const smgpu_quality_geometry_params* p) {
    const smgpu_quality_geometry_params prm = p ? *p : smgpu_quality_geometry_params{10.0, 0.8, 0.05, 0.01, 0.001};
    return QualityGeomThresholds{std::sin(prm.concaveThreshold * (SMGPU_PI / 180.0)), prm.flatnessThreshold, prm.weightThreshold,
                                 prm.volRatioThreshold, prm.determinantThreshold};
}
static QualityMotionThresholds motionThresholds(const smgpu_quality_motion_params* p) {
    const smgpu_quality_motion_params prm = p ? *p : smgpu_quality_motion_params{1e-15, 0.02, -1.0};
    // k = 8 / (9 sqrt 3) is the host's double, as the contract says: the kernel takes it as an argument
    return QualityMotionThresholds{prm.tetThreshold, prm.twistThreshold, prm.triangleTwistThreshold, 8.0 / (9.0 * std::sqrt(3.0))};
}
// a coupled call's refusals: the geometry and the coupling are those of the last pack (DESIGN.md "Mesh quality", 10.4); `buf` is the
// device buffer the call may not go without (`what`) when there are processor faces
static int qualityCoupledReady(smgpu_handle* h, const char* api, const void* buf, const char* what = "recvCc") {
    if (h->iterOpen) return fail(std::string(api) + ": not between smgpu_iter_begin and smgpu_iter_end");
    if (!h->q.partOut || h->q.packEpoch != h->q.epoch)
        return fail(std::string(api) + ": call smgpu_quality_coupled_pack first (the points may have moved since the last pack)");
    if (h->q.nProc > 0 && !buf) return fail(std::string(api) + ": null " + what);
    return 0;
}
// ... and of a coupled geometry call: the volumes are those of a pack_volumes on the same pack
static int qualityCoupledGeomReady(smgpu_handle* h, const char* api, const void* recvCc, const void* recvVc) {
    if (qualityCoupledReady(h, api, recvCc)) return 1;
    if (!h->q.gPartOut || h->q.volEpoch != h->q.epoch || h->q.volCoupling != h->q.coupling)
        return fail(std::string(api) + ": call smgpu_quality_coupled_pack_volumes after smgpu_quality_coupled_pack first");
    if (h->q.nProc > 0 && !recvVc) return fail(std::string(api) + ": null recvVc");
    return 0;
}
static QCoupling<true> qualityCoupling(const smgpu_handle* h, const void* recvCc, const void* recvVc) {
    return QCoupling<true>{h->q.slot, (const double*)recvCc, (const double*)recvVc};
}
static double* const kQualityNoFields[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};

static int qualityGeomEnsure(smgpu_handle* h) {
    if (qualityEnsure(h)) return 1;
    QualityReportHost& q = h->q;
    if (q.geom.live()) return 0;
    const MeshView& m = h->mv;
    const size_t nFB = (size_t)std::max(1, qualityGrid(m.nFaces)), nCB = (size_t)std::max(1, qualityGrid(m.nCells));
    if (q.geom.alloc(&q.vol, (size_t)std::max(1, m.nCells)) || q.geom.alloc(&q.gFacePart, nFB) || q.geom.alloc(&q.gCellPart, nCB) ||
        q.geom.alloc(&q.gOut, 1))
        return q.geom.failed("the geometry report");
    return 0;
}
static int qualityMotionEnsure(smgpu_handle* h) {
    if (qualityEnsure(h)) return 1;
    QualityReportHost& q = h->q;
    if (q.motion.live()) return 0;
    const size_t nFB = (size_t)std::max(1, qualityGrid(h->mv.nFaces));
    if (q.motion.alloc(&q.mFacePart, nFB) || q.motion.alloc(&q.mOut, 1)) return q.motion.failed("the motion criteria");
    return 0;
}

// Every report is one function for the serial mesh (Coupled = false: cp is empty, api unused) and for a sub-domain (Coupled = true,
// on the geometry of the last pack): the same launches of the same kernels, with or without the coupling.  o: the optional
// per-element outputs, in the order of the report's field table below.
extern "C++" {
// the record a report's final reduction left on the device, to the host
template <class T>
static int qualityCopyOut(smgpu_handle* h, T* out, const T* dev) {
    HIP_OK(hipMemcpyAsync(out, dev, sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

// serial: geometry of the current points (the loop's own kernel, publishing face values by id as for smgpu_debug_propose; not counted
// in the engine's statistics), then the face pass, the cell pass and the final reduction into h->q.out; coupled: into h->q.partOut
template <bool Coupled>
static int runQuality(smgpu_handle* h, const char* api, const smgpu_quality_params* p, const QCoupling<Coupled>& cp, double* const* o) {
    if constexpr (Coupled) {
        if (qualityCoupledReady(h, api, cp.recvCc)) return 1;
        HIP_OK(hipSetDevice(h->device));
    } else {
        if (qualitySerialBegin(h, qualityEnsure)) return 1;
    }
    const MeshView& m = h->mv;
    const QualityThresholds thr = qualityThresholds(p);
    const int nFB = qualityGrid(m.nFaces), nCB = qualityGrid(m.nCells);
    const State& s = h->st;
    if (nFB > 0)
        hipLaunchKernelGGL(k_quality_faces<Coupled>, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.fArea, s.cellCtr, h->q.own,
                           h->q.nei, cp, thr, h->q.facePart, o[0], o[1]);
    if (nCB > 0)
        hipLaunchKernelGGL(k_quality_cells, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, s.fCtr, s.fArea, thr, h->q.cellPart, o[2], o[3], o[4]);
    if constexpr (Coupled)
        hipLaunchKernelGGL(k_quality_final<smgpu_quality_part>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.facePart, nFB, h->q.cellPart, nCB,
                           m.nCells, m.nFaces - h->q.notCounted, m.nInternalFaces + h->q.countedProc, h->q.partOut);
    else
        hipLaunchKernelGGL(k_quality_final<smgpu_quality>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.facePart, nFB, h->q.cellPart, nCB,
                           m.nCells, m.nFaces, m.nInternalFaces, h->q.out);
    HIP_OK(hipGetLastError());
    return 0;
}

// the -allGeometry checks (DESIGN.md "Mesh quality", 10.6 and 10.8).  serial: geometry, the cell pass (volumes into h->q.vol), the face
// pass, the final reduction into h->q.gOut; coupled: the volumes are those of the last pack_volumes, the record goes to h->q.gPartOut
template <bool Coupled>
static int runQualityGeom(smgpu_handle* h, const char* api, const smgpu_quality_geometry_params* p, const QCoupling<Coupled>& cp, double* const* o) {
    if constexpr (Coupled) {
        if (qualityCoupledGeomReady(h, api, cp.recvCc, cp.recvVc)) return 1;
        HIP_OK(hipSetDevice(h->device));
    } else {
        if (qualitySerialBegin(h, qualityGeomEnsure)) return 1;
    }
    const MeshView& m = h->mv;
    const QualityGeomThresholds thr = geomThresholds(p);
    const int nFB = qualityGrid(m.nFaces), nCB = qualityGrid(m.nCells);
    const State& s = h->st;
    if (nCB > 0) {
        if constexpr (Coupled)
            hipLaunchKernelGGL(k_quality_geom_cells_coupled, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, s.fArea, cp.slot, thr, h->q.gCellPart, o[4]);
        else
            hipLaunchKernelGGL(k_quality_geom_cells, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, s.fCtr, s.fArea, thr, h->q.gCellPart, h->q.vol, o[4]);
    }
    if (nFB > 0) {
        if constexpr (Coupled)
            hipLaunchKernelGGL(k_quality_geom_faces_coupled, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.fArea, s.cellCtr,
                               h->q.vol, h->q.own, h->q.nei, cp.slot, cp.recvCc, cp.recvVc, thr, h->q.gFacePart, o[0], o[1], o[2], o[3]);
        else
            hipLaunchKernelGGL(k_quality_geom_faces, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.fArea, s.cellCtr, h->q.vol,
                               h->q.own, h->q.nei, thr, h->q.gFacePart, o[0], o[1], o[2], o[3]);
    }
    if constexpr (Coupled)
        hipLaunchKernelGGL(k_quality_geom_final<smgpu_quality_geometry_part>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.gFacePart, nFB,
                           h->q.gCellPart, nCB, m.nCells, m.nFaces - h->q.notCounted, m.nInternalFaces + h->q.countedProc, h->q.gPartOut);
    else
        hipLaunchKernelGGL(k_quality_geom_final<smgpu_quality_geometry>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.gFacePart, nFB,
                           h->q.gCellPart, nCB, m.nCells, m.nFaces, m.nInternalFaces, h->q.gOut);
    HIP_OK(hipGetLastError());
    return 0;
}

// the motion criteria (DESIGN.md "Mesh quality", 10.7 and 10.8).  serial: geometry, the face pass, the final reduction into h->q.mOut;
// coupled: the record goes to h->q.mPartOut
template <bool Coupled>
static int runQualityMotion(smgpu_handle* h, const char* api, const smgpu_quality_motion_params* p, const QCoupling<Coupled>& cp, double* const* o) {
    if constexpr (Coupled) {
        if (qualityCoupledReady(h, api, cp.recvCc)) return 1;
        HIP_OK(hipSetDevice(h->device));
        if (qualityMotionEnsure(h)) return 1;
        if (!h->q.mPartOut) HIP_OK(h->q.coupled.alloc(&h->q.mPartOut, 1));
    } else {
        if (qualitySerialBegin(h, qualityMotionEnsure)) return 1;
    }
    const MeshView& m = h->mv;
    const QualityMotionThresholds thr = motionThresholds(p);
    const int nFB = qualityGrid(m.nFaces);
    const State& s = h->st;
    if (nFB > 0) {
        if constexpr (Coupled)
            hipLaunchKernelGGL(k_quality_motion_faces_coupled, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.cellCtr, h->q.own,
                               h->q.nei, cp.slot, cp.recvCc, thr, h->q.mFacePart, o[0], o[1], o[2], o[3]);
        else
            hipLaunchKernelGGL(k_quality_motion_faces, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.cellCtr, h->q.own, h->q.nei,
                               thr, h->q.mFacePart, o[0], o[1], o[2], o[3]);
    }
    if constexpr (Coupled)
        hipLaunchKernelGGL(k_quality_motion_final<smgpu_quality_motion_part>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.mFacePart, nFB,
                           m.nFaces - h->q.notCounted, h->q.mPartOut);
    else
        hipLaunchKernelGGL(k_quality_motion_final<smgpu_quality_motion>, dim3(1), dim3(kQualityBlock), 0, h->stream, h->q.mFacePart, nFB, m.nFaces,
                           h->q.mOut);
    HIP_OK(hipGetLastError());
    return 0;
}

// the per-element fields of a report kind: names[0, n), those from firstCell on per cell, and the refusal of any other name
struct QualityFields { int n, firstCell; const char* names[5]; const char* unknown; const char* known; };
static const QualityFields kQualityFields{5, 2, {"faceNonOrthogonality", "faceSkewness", "cellVolume", "cellOpenness", "cellAspectRatio"},
                                          "unknown quality field ", " (cellVolume, cellOpenness, cellAspectRatio, faceNonOrthogonality, faceSkewness)"};
static const QualityFields kQualityGeomFields{5, 4, {"faceConcavity", "faceFlatness", "faceWeight", "faceVolumeRatio", "cellDeterminant"},
                                              "unknown quality geometry field ",
                                              " (faceConcavity, faceFlatness, faceWeight, faceVolumeRatio, cellDeterminant)"};
static const QualityFields kQualityMotionFields{4, 4, {"faceTetQuality", "faceBaseTetQuality", "faceTwist", "faceTriangleTwist"},
                                                "unknown quality motion field ", " (faceTetQuality, faceBaseTetQuality, faceTwist, faceTriangleTwist)"};
// one per-element field: `run(o)` launches the report's passes with the outputs o, the named one set to a buffer allocated for
// this call (outside deviceBytes)
template <class Run>
static int qualityField(smgpu_handle* h, const QualityFields& t, const char* api, const char* name, double* out, int64_t* n, Run run) {
    int which = -1;
    for (int i = 0; i < t.n; ++i)
        if (std::strcmp(name, t.names[i]) == 0) which = i;
    if (which < 0) return fail(std::string(t.unknown) + name + t.known);
    const int64_t cnt = which >= t.firstCell ? h->mv.nCells : h->mv.nFaces;
    *n = cnt;
    if (!out) return 0;
    HIP_OK(hipSetDevice(h->device));
    double* buf = nullptr;   // transient: one field's worth for this call only
    HIP_OK(hipMalloc((void**)&buf, sizeof(double) * (size_t)std::max<int64_t>(1, cnt)));
    double* o[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    o[which] = buf;
    int rc = run(o);
    if (rc == 0 && cnt > 0) {
        const hipError_t e = hipMemcpyAsync(out, buf, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(std::string(api) + ": " + hipGetErrorString(e));
    }
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (rc == 0 && es != hipSuccess) rc = fail(std::string(api) + ": " + hipGetErrorString(es));
    (void)hipFree(buf);
    return rc;
}
}  // extern "C++"

int smgpu_mesh_quality(smgpu_handle* h, const smgpu_quality_params* p, smgpu_quality* out) {
    if (!h || !out) return fail("null argument");
    if (runQuality(h, nullptr, p, QCoupling<false>{}, kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.out);
}
int smgpu_quality_field(smgpu_handle* h, const char* name, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    return qualityField(h, kQualityFields, "smgpu_quality_field", name, out, n,
                        [&](double** o) { return runQuality(h, nullptr, nullptr, QCoupling<false>{}, o); });
}

int smgpu_mesh_quality_geometry(smgpu_handle* h, const smgpu_quality_geometry_params* p, smgpu_quality_geometry* out) {
    if (!h || !out) return fail("null argument");
    if (runQualityGeom(h, nullptr, p, QCoupling<false>{}, kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.gOut);
}
int smgpu_quality_geometry_field(smgpu_handle* h, const char* name, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    return qualityField(h, kQualityGeomFields, "smgpu_quality_geometry_field", name, out, n,
                        [&](double** o) { return runQualityGeom(h, nullptr, nullptr, QCoupling<false>{}, o); });
}

int smgpu_mesh_quality_motion(smgpu_handle* h, const smgpu_quality_motion_params* p, smgpu_quality_motion* out) {
    if (!h || !out) return fail("null argument");
    if (runQualityMotion(h, nullptr, p, QCoupling<false>{}, kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.mOut);
}
int smgpu_quality_motion_field(smgpu_handle* h, const char* name, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    if (h->haloOn) return fail(kQualityHaloRefusal);
    return qualityField(h, kQualityMotionFields, "smgpu_quality_motion_field", name, out, n,
                        [&](double** o) { return runQualityMotion(h, nullptr, nullptr, QCoupling<false>{}, o); });
}

// ---- the coupled reports of a sub-domain (DESIGN.md "Mesh quality", 10.4 and 10.8) -----------------------------------------
// A coupling description, checked (the patches inside the boundary faces, disjoint, one per neighbour, none to this rank), as
// 10.4's tables: key (what two couplings are compared by), procFace (the processor faces in patch order), slot (by boundary face:
// -1 on a physical patch, else the face's place in patch order | kQualityNotCounted on the side with myRank > neighbRank)
extern "C++" {
static int qualityCouplingTables(const std::string& api, const MeshView& m, const smgpu_quality_coupling* c, std::vector<int32_t>& key,
                                 std::vector<int>& procFace, std::vector<int>& slot, int64_t& nProc, int64_t& notCounted) {
    if (c->nPatches < 0 || (c->nPatches && (!c->patchStart || !c->patchSize || !c->neighbRank)))
        return fail(api + ": bad coupling description");
    key = {c->myRank, c->nPatches};
    std::vector<std::pair<int, int>> ranges;
    std::vector<int> seen;
    nProc = 0; notCounted = 0;
    for (int i = 0; i < c->nPatches; ++i) {
        const int32_t st = c->patchStart[i], sz = c->patchSize[i], o = c->neighbRank[i];
        if (sz < 0 || st < m.nInternalFaces || (int64_t)st + sz > m.nFaces)
            return fail(api + ": processor patch " + std::to_string(i) + " is not a range of boundary faces");
        if (o < 0 || o == c->myRank) return fail(api + ": processor patch " + std::to_string(i) + " has a bad neighbour rank");
        if (std::find(seen.begin(), seen.end(), o) != seen.end())
            return fail(api + ": two processor patches to rank " + std::to_string(o) +
                        " (processorCyclic patches or several patches per neighbour are not supported)");
        seen.push_back(o);
        ranges.emplace_back(st, sz);
        nProc += sz;
        if (c->myRank > o) notCounted += sz;
        key.insert(key.end(), {st, sz, o});
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i)
        if (ranges[i - 1].first + ranges[i - 1].second > ranges[i].first) return fail(api + ": processor patches overlap");
    // face list and slots of this coupling (small: the boundary faces)
    const int nB = m.nFaces - m.nInternalFaces;
    procFace.assign((size_t)nProc, 0);
    slot.assign((size_t)nB, -1);
    int k = 0;
    for (int i = 0; i < c->nPatches; ++i) {
        const int flag = c->myRank > c->neighbRank[i] ? kQualityNotCounted : 0;
        for (int j = 0; j < c->patchSize[i]; ++j, ++k) {
            const int f = c->patchStart[i] + j;
            procFace[(size_t)k] = f;
            slot[(size_t)(f - m.nInternalFaces)] = k | flag;
        }
    }
    return 0;
}
}  // extern "C++"

int smgpu_quality_coupled_pack(smgpu_handle* h, const smgpu_quality_coupling* c, void* sendCc, int64_t* nProcFaces) {
    if (!h || !c) return fail("null argument");
    if (h->iterOpen) return fail("smgpu_quality_coupled_pack: not between smgpu_iter_begin and smgpu_iter_end");
    const MeshView& m = h->mv;
    std::vector<int32_t> key;
    std::vector<int> procFace, slot;
    int64_t nProc = 0, notCounted = 0;
    if (qualityCouplingTables("smgpu_quality_coupled_pack", m, c, key, procFace, slot, nProc, notCounted)) return 1;
    if (nProc > 0 && !sendCc) return fail("smgpu_quality_coupled_pack: null sendCc");
    HIP_OK(hipSetDevice(h->device));
    if (qualityEnsure(h)) return 1;
    if (key != h->q.coupling) {
        // uploaded once per coupling
        const int nB = m.nFaces - m.nInternalFaces;
        h->q.coupled.release();   // (the three records with it: each comes back with the first call that writes it)
        h->q.coupling.clear();
        HIP_OK(h->q.coupled.alloc(&h->q.procFace, (size_t)std::max<int64_t>(1, nProc)));
        HIP_OK(h->q.coupled.alloc(&h->q.slot, (size_t)std::max(1, nB)));
        if (nProc) HIP_OK(hipMemcpyAsync(h->q.procFace, procFace.data(), sizeof(int) * (size_t)nProc, hipMemcpyHostToDevice, h->stream));
        if (nB) HIP_OK(hipMemcpyAsync(h->q.slot, slot.data(), sizeof(int) * (size_t)nB, hipMemcpyHostToDevice, h->stream));
        HIP_OK(hipStreamSynchronize(h->stream));   // (the host vectors go out of scope)
        h->q.coupling = key;
        h->q.nProc = (int)nProc;
        h->q.notCounted = (int)notCounted;
        h->q.countedProc = (int)(nProc - notCounted);
    }
    if (!h->q.partOut) HIP_OK(h->q.coupled.alloc(&h->q.partOut, 1));
    if (qualityGeometry(h)) return 1;
    if (h->q.nProc > 0)
        hipLaunchKernelGGL(k_quality_pack, dim3(gridFor(h->q.nProc)), dim3(kQualityBlock), 0, h->stream, h->q.own, h->st.cellCtr, h->q.procFace, h->q.nProc,
                           (double*)sendCc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(h->stream));       // sendCc is the host's to move
    h->q.packEpoch = h->q.epoch;
    if (nProcFaces) *nProcFaces = h->q.nProc;
    return 0;
}

int smgpu_quality_coupled_report(smgpu_handle* h, const smgpu_quality_params* p, const void* recvCc, smgpu_quality_part* out) {
    if (!h || !out) return fail("null argument");
    if (runQuality(h, "smgpu_quality_coupled_report", p, qualityCoupling(h, recvCc, nullptr), kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.partOut);
}
int smgpu_quality_coupled_field(smgpu_handle* h, const char* name, const void* recvCc, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    const char* api = "smgpu_quality_coupled_field";
    return qualityField(h, kQualityFields, api, name, out, n,
                        [&](double** o) { return runQuality(h, api, nullptr, qualityCoupling(h, recvCc, nullptr), o); });
}

int smgpu_quality_coupled_pack_volumes(smgpu_handle* h, void* sendVc, int64_t* nProcFaces) {
    if (!h) return fail("null argument");
    if (qualityCoupledReady(h, "smgpu_quality_coupled_pack_volumes", sendVc, "sendVc")) return 1;
    HIP_OK(hipSetDevice(h->device));
    if (qualityGeomEnsure(h)) return 1;
    if (!h->q.gPartOut) HIP_OK(h->q.coupled.alloc(&h->q.gPartOut, 1));
    const MeshView& m = h->mv;
    const int nCB = qualityGrid(m.nCells);
    if (nCB > 0)
        hipLaunchKernelGGL(k_quality_cell_volumes, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, h->st.fCtr, h->st.fArea, h->q.vol);
    if (h->q.nProc > 0)
        hipLaunchKernelGGL(k_quality_pack_volumes, dim3(gridFor(h->q.nProc)), dim3(kQualityBlock), 0, h->stream, h->q.own, h->q.vol, h->q.procFace,
                           h->q.nProc, (double*)sendVc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(h->stream));       // sendVc is the host's to move
    h->q.volEpoch = h->q.epoch;
    h->q.volCoupling = h->q.coupling;
    if (nProcFaces) *nProcFaces = h->q.nProc;
    return 0;
}

int smgpu_quality_coupled_geometry_report(smgpu_handle* h, const smgpu_quality_geometry_params* p, const void* recvCc, const void* recvVc,
                                          smgpu_quality_geometry_part* out) {
    if (!h || !out) return fail("null argument");
    if (runQualityGeom(h, "smgpu_quality_coupled_geometry_report", p, qualityCoupling(h, recvCc, recvVc), kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.gPartOut);
}
int smgpu_quality_coupled_geometry_field(smgpu_handle* h, const char* name, const void* recvCc, const void* recvVc, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    const char* api = "smgpu_quality_coupled_geometry_field";
    return qualityField(h, kQualityGeomFields, api, name, out, n,
                        [&](double** o) { return runQualityGeom(h, api, nullptr, qualityCoupling(h, recvCc, recvVc), o); });
}

int smgpu_quality_coupled_motion_report(smgpu_handle* h, const smgpu_quality_motion_params* p, const void* recvCc, smgpu_quality_motion_part* out) {
    if (!h || !out) return fail("null argument");
    if (runQualityMotion(h, "smgpu_quality_coupled_motion_report", p, qualityCoupling(h, recvCc, nullptr), kQualityNoFields)) return 1;
    return qualityCopyOut(h, out, h->q.mPartOut);
}
int smgpu_quality_coupled_motion_field(smgpu_handle* h, const char* name, const void* recvCc, double* out, int64_t* n) {
    if (!h || !name || !n) return fail("null argument");
    const char* api = "smgpu_quality_coupled_motion_field";
    return qualityField(h, kQualityMotionFields, api, name, out, n,
                        [&](double** o) { return runQualityMotion(h, api, nullptr, qualityCoupling(h, recvCc, nullptr), o); });
}

// ---- the failing elements as sets (DESIGN.md "Mesh quality", 10.5 and 10.9) ------------------------------------------------
// One sequence for the three reports' sets, <NF, NC> being the report's set layout (NF face sets, then NC cell sets):
// flags(mask, cnt) launches the report's flag passes (faces: mask[0, F), the cnt rows of the face sets; cells: mask[F, F + C),
// cnt + NF * nFB); then the scan, one copy of the counts, and when ids fit the scatter and one copy of the ids.  Every buffer is
// this call's own (outside deviceBytes, as the field buffers).
extern "C++" {
template <int NF, int NC, class Flags>
static int qualitySetsOf(smgpu_handle* h, const char* api, Flags flags, int64_t* counts, int32_t* ids, int64_t cap) {
    const MeshView& m = h->mv;
    const int nFB = qualityGrid(m.nFaces), nCB = NC > 0 ? qualityGrid(m.nCells) : 0;
    const int nCnt = NF * nFB + NC * nCB;
    uint8_t* mask = nullptr;
    int* cnt = nullptr;
    long long *off = nullptr, *dCounts = nullptr;
    int* dIds = nullptr;
    int rc = 0;
    auto hipFail = [&](hipError_t e) { rc = fail(std::string(api) + ": " + hipGetErrorString(e)); };
    hipError_t e = hipMalloc((void**)&mask, (size_t)std::max<int64_t>(1, (int64_t)m.nFaces + (NC > 0 ? m.nCells : 0)));
    if (e == hipSuccess) e = hipMalloc((void**)&cnt, sizeof(int) * (size_t)std::max(1, nCnt));
    if (e == hipSuccess) e = hipMalloc((void**)&off, sizeof(long long) * ((size_t)nCnt + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&dCounts, sizeof(long long) * (NF + NC));
    if (e != hipSuccess) hipFail(e);
    if (rc == 0) {
        flags(mask, cnt, nFB, nCB);
        e = hipGetLastError();
        if (e != hipSuccess) hipFail(e);
    }
    if (rc == 0) {
        hipLaunchKernelGGL((k_quality_set_scan<NF, NC>), dim3(1), dim3(kQualityScanBlock), 0, h->stream, cnt, nCnt, nFB, nCB, off, dCounts);
        long long hc[NF + NC];
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hc, dCounts, sizeof(hc), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) hipFail(e);
        int64_t total = 0;
        for (int s = 0; s < NF + NC && rc == 0; ++s) { counts[s] = hc[s]; total += hc[s]; }
        if (rc == 0 && ids && cap < total)
            rc = fail(std::string(api) + ": ids holds " + std::to_string(cap) + " labels, the sets need " + std::to_string(total));
        if (rc == 0 && ids && total > 0) {
            e = hipMalloc((void**)&dIds, sizeof(int) * (size_t)total);
            if (e == hipSuccess) {
                hipLaunchKernelGGL((k_quality_set_scatter<NF, NC>), dim3(nFB + nCB), dim3(kQualityBlock), 0, h->stream, mask, m.nFaces, m.nCells, nFB,
                                   nCB, off, dIds, (long long)total);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(ids, dIds, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) hipFail(e);
        }
    }
    (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)mask, (void*)cnt, (void*)off, (void*)dCounts, (void*)dIds})
        if (p) (void)hipFree(p);
    return rc;
}

template <bool Coupled>
static int qualitySets(smgpu_handle* h, const char* api, const smgpu_quality_params* p, const QCoupling<Coupled>& cp, int64_t counts[7], int32_t* ids,
                       int64_t cap) {
    const QualityThresholds thr = qualityThresholds(p);
    return qualitySetsOf<kQualityFaceSets, kQualityCellSets>(h, api, [&](uint8_t* mask, int* cnt, int nFB, int nCB) {
        const MeshView& m = h->mv;
        const State& s = h->st;
        if (nFB > 0)
            hipLaunchKernelGGL(k_quality_face_flags<Coupled>, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.fArea, s.cellCtr,
                               h->q.own, h->q.nei, cp, thr, mask, cnt);
        if (nCB > 0)
            hipLaunchKernelGGL(k_quality_cell_flags, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, s.fCtr, s.fArea, thr, mask + m.nFaces,
                               cnt + (size_t)kQualityFaceSets * nFB);
    }, counts, ids, cap);
}
// the sets of the -allGeometry checks (10.9): the cell flag pass first (serial: it leaves the volumes in h->q.vol), then the
// face flag pass.  The caller has made the refusals and the geometry of the matching report (runQualityGeom).
template <bool Coupled>
static int qualityGeomSets(smgpu_handle* h, const char* api, const smgpu_quality_geometry_params* p, const QCoupling<Coupled>& cp, int64_t counts[5],
                           int32_t* ids, int64_t cap) {
    const QualityGeomThresholds thr = geomThresholds(p);
    return qualitySetsOf<kQualityGeomFaceSets, kQualityGeomCellSets>(h, api, [&](uint8_t* mask, int* cnt, int nFB, int nCB) {
        const MeshView& m = h->mv;
        const State& s = h->st;
        if (nCB > 0)
            hipLaunchKernelGGL(k_quality_geom_cell_flags<Coupled>, dim3(nCB), dim3(kQualityBlock), 0, h->stream, m, s.fCtr, s.fArea, cp, thr, h->q.vol,
                               mask + m.nFaces, cnt + (size_t)kQualityGeomFaceSets * nFB);
        if (nFB > 0)
            hipLaunchKernelGGL(k_quality_geom_face_flags<Coupled>, dim3(nFB), dim3(kQualityBlock), 0, h->stream, m, s.ptsCur, s.fCtr, s.fArea,
                               s.cellCtr, h->q.vol, h->q.own, h->q.nei, cp, thr, mask, cnt);
    }, counts, ids, cap);
}
// ... and of the motion criteria: face sets only
template <bool Coupled>
static int qualityMotionSets(smgpu_handle* h, const char* api, const smgpu_quality_motion_params* p, const QCoupling<Coupled>& cp, int64_t counts[4],
                             int32_t* ids, int64_t cap) {
    const QualityMotionThresholds thr = motionThresholds(p);
    return qualitySetsOf<kQualityMotionFaceSets, 0>(h, api, [&](uint8_t* mask, int* cnt, int nFB, int) {
        const State& s = h->st;
        if (nFB > 0)
            hipLaunchKernelGGL(k_quality_motion_face_flags<Coupled>, dim3(nFB), dim3(kQualityBlock), 0, h->stream, h->mv, s.ptsCur, s.fCtr, s.cellCtr,
                               h->q.own, h->q.nei, cp, thr, mask, cnt);
    }, counts, ids, cap);
}
}  // extern "C++"

int smgpu_quality_sets(smgpu_handle* h, const smgpu_quality_params* p, int64_t counts[7], int32_t* ids, int64_t cap) {
    if (!h || !counts) return fail("null argument");
    if (qualitySerialBegin(h, qualityEnsure)) return 1;
    return qualitySets(h, "smgpu_quality_sets", p, QCoupling<false>{}, counts, ids, cap);
}

int smgpu_quality_coupled_sets(smgpu_handle* h, const smgpu_quality_params* p, const void* recvCc, int64_t counts[7], int32_t* ids, int64_t cap) {
    if (!h || !counts) return fail("null argument");
    const char* api = "smgpu_quality_coupled_sets";
    if (qualityCoupledReady(h, api, recvCc)) return 1;
    HIP_OK(hipSetDevice(h->device));
    return qualitySets(h, api, p, qualityCoupling(h, recvCc, nullptr), counts, ids, cap);
}

int smgpu_quality_geometry_sets(smgpu_handle* h, const smgpu_quality_geometry_params* p, int64_t counts[5], int32_t* ids, int64_t cap) {
    if (!h || !counts) return fail("null argument");
    if (qualitySerialBegin(h, qualityGeomEnsure)) return 1;
    return qualityGeomSets(h, "smgpu_quality_geometry_sets", p, QCoupling<false>{}, counts, ids, cap);
}

int smgpu_quality_motion_sets(smgpu_handle* h, const smgpu_quality_motion_params* p, int64_t counts[4], int32_t* ids, int64_t cap) {
    if (!h || !counts) return fail("null argument");
    if (qualitySerialBegin(h, qualityEnsure)) return 1;
    return qualityMotionSets(h, "smgpu_quality_motion_sets", p, QCoupling<false>{}, counts, ids, cap);
}

int smgpu_quality_coupled_geometry_sets(smgpu_handle* h, const smgpu_quality_geometry_params* p, const void* recvCc, const void* recvVc,
                                        int64_t counts[5], int32_t* ids, int64_t cap) {
    if (!h || !counts) return fail("null argument");
    const char* api = "smgpu_quality_coupled_geometry_sets";
    if (qualityCoupledGeomReady(h, api, recvCc, recvVc)) return 1;
    HIP_OK(hipSetDevice(h->device));
    return qualityGeomSets(h, api, p, qualityCoupling(h, recvCc, recvVc), counts, ids, cap);
}

int smgpu_quality_coupled_motion_sets(smgpu_handle* h, const smgpu_quality_motion_params* p, const void* recvCc, int64_t counts[4], int32_t* ids,
                                      int64_t cap) {
    if (!h || !counts) return fail("null argument");
    const char* api = "smgpu_quality_coupled_motion_sets";
    if (qualityCoupledReady(h, api, recvCc)) return 1;
    HIP_OK(hipSetDevice(h->device));
    return qualityMotionSets(h, api, p, qualityCoupling(h, recvCc, nullptr), counts, ids, cap);
}

