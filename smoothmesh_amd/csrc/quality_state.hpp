// quality_state.hpp -- host state of the mesh quality features (DESIGN.md "Mesh quality"): the owners of their device memory and
// the four groups of members smgpu_handle carries.  Included by smgpu.hip once, before the handle (after fail() and HIP_OK).
// All of this memory lives outside the handle's `allocs`: deviceBytes stays what the loop holds.
#pragma once

// Owner of one feature's device memory: alloc() fills a pointer member and remembers where that member is, release() frees and
// nulls every member it filled: a feature names its pointers once, where it allocates them.
class DevBlock {
    std::vector<void**> slots;
    hipError_t err = hipSuccess;
  public:
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    // n elements of T into the null member *slot; an error (non-zero) leaves the block as it was: see failed()
    template <class T>
    hipError_t alloc(T** slot, size_t n) {
        void* p = nullptr;
        err = hipMalloc(&p, sizeof(T) * n);
        if (err != hipSuccess) return err;
        *slot = (T*)p;
        slots.push_back((void**)slot);
        return hipSuccess;
    }
    bool live() const { return !slots.empty(); }
    void release() {
        for (void** s : slots) { (void)hipFree(*s); *s = nullptr; }
        slots.clear();
    }
    // after an alloc() that returned an error: everything released, and the refusal "mesh quality: device memory for <what>: ..."
    int failed(const char* what) {
        release();
        return fail(std::string("mesh quality: device memory for ") + what + ": " + hipGetErrorString(err));
    }
};

// The records one smgpu_iterate call leaves on the device, one slot per record in queueing order, and those of earlier calls
// that nobody has fetched yet.  A record whose `iteration` is 0 was not written (its iteration did not run).
template <class Rec>
class RecordSlab {
    const char* what;            // the feature, in the refusals
    Rec* dev = nullptr;
    int cap = 0;
    std::vector<Rec> back;       // the read-back of the call
    std::vector<Rec> pending;
  public:
    explicit RecordSlab(const char* feature) : what(feature) {}
    RecordSlab(const RecordSlab&) = delete;
    RecordSlab& operator=(const RecordSlab&) = delete;
    // start of a call that queues up to n records: n zeroed slots (outgrown: replaced; nothing is in flight between two calls)
    int begin(hipStream_t stream, int n) {
        if (n > cap) {
            if (dev) {
                HIP_OK(hipStreamSynchronize(stream));
                release();
            }
            const hipError_t e = hipMalloc((void**)&dev, sizeof(Rec) * (size_t)n);
            if (e != hipSuccess) return fail(std::string("mesh quality: device memory for the ") + what + ": " + hipGetErrorString(e));
            cap = n;
        }
        if (n > 0) HIP_OK(hipMemsetAsync(dev, 0, sizeof(Rec) * (size_t)n, stream));
        return 0;
    }
    // *rec: the device address of slot i, one of those begin() made
    int slot(int i, Rec** rec) const {
        if (i >= cap) return fail(std::string("mesh quality: ") + what + " slab overrun");
        *rec = dev + i;
        return 0;
    }
    // queues the copy of the first n slots to the host; complete once the stream has been waited for
    int readBack(hipStream_t stream, int n) {
        back.resize((size_t)n);
        if (n > 0) HIP_OK(hipMemcpyAsync(back.data(), dev, sizeof(Rec) * (size_t)n, hipMemcpyDeviceToHost, stream));
        return 0;
    }
    // the written ones of the first n records read back become pending
    void keep(int n) {
        for (int i = 0; i < n; ++i)
            if (back[(size_t)i].iteration != 0) pending.push_back(back[(size_t)i]);
    }
    void discard() { pending.clear(); }
    // the getter of the pending records (out == NULL: their number only); a read clears them
    int drain(Rec* out, int64_t capOut, int64_t* n, const char* api) {
        const int64_t have = (int64_t)pending.size();
        if (!out) { *n = have; return 0; }
        if (capOut < have) return fail(std::string(api) + ": cap " + std::to_string(capOut) + " is below the " + std::to_string(have) + " pending records");
        if (have > 0) std::memcpy(out, pending.data(), sizeof(Rec) * (size_t)have);
        pending.clear();
        *n = have;
        return 0;
    }
    // drain() for a caller whose record is the head of Rec: each pending record's first sizeof(Head) bytes
    template <class Head>
    int drainHeads(Head* out, int64_t capOut, int64_t* n, const char* api) {
        static_assert(sizeof(Head) <= sizeof(Rec), "a head is no longer than the record");
        const int64_t have = (int64_t)pending.size();
        if (!out) { *n = have; return 0; }
        if (capOut < have) return fail(std::string(api) + ": cap " + std::to_string(capOut) + " is below the " + std::to_string(have) + " pending records");
        for (int64_t i = 0; i < have; ++i) std::memcpy(out + i, &pending[(size_t)i], sizeof(Head));
        pending.clear();
        *n = have;
        return 0;
    }
    // the device slab (the pending records stay)
    void release() { if (dev) (void)hipFree(dev); dev = nullptr; cap = 0; }
};

// The three reports (smgpu_mesh_quality, _geometry, _motion; kernels_quality*.hpp) and their coupled forms.  Each block is
// allocated by the first call that needs it.
struct QualityReportHost {
    // the base report: owner / neighbour by face, the two partial slabs and the report
    DevBlock base;
    int *own = nullptr, *nei = nullptr;
    QFace* facePart = nullptr;
    QCell* cellPart = nullptr;
    smgpu_quality* out = nullptr;
    // the -allGeometry checks: the cell volumes the face pass reads, the two partial slabs and the report
    DevBlock geom;
    double* vol = nullptr;
    QGFace* gFacePart = nullptr;
    QGCell* gCellPart = nullptr;
    smgpu_quality_geometry* gOut = nullptr;
    // the motion criteria: the partial slab and the report
    DevBlock motion;
    QMFace* mFacePart = nullptr;
    smgpu_quality_motion* mOut = nullptr;
    // a sub-domain's coupled reports (smgpu_quality_coupled_*): processor faces in patch order, the recvCc slot of every boundary
    // face (-1: physical patch), the coupling they were built from, the three records.  A pack with another coupling releases it
    DevBlock coupled;
    int *procFace = nullptr, *slot = nullptr;
    int nProc = 0, notCounted = 0, countedProc = 0;
    std::vector<int32_t> coupling;
    smgpu_quality_part* partOut = nullptr;
    smgpu_quality_geometry_part* gPartOut = nullptr;
    smgpu_quality_motion_part* mPartOut = nullptr;
    // epoch moves whenever the points (or the geometry variant) may have changed; packEpoch: that of the last pack; volEpoch,
    // volCoupling: epoch and coupling of the last pack_volumes (another coupling's slots differ: its sendVc / recvVc no longer fit)
    uint64_t epoch = 1, packEpoch = 0, volEpoch = 0;
    std::vector<int32_t> volCoupling;
    void release() { base.release(); geom.release(); motion.release(); coupled.release(); }
};

// The quality history (smgpu_set_quality_trace, kernels_quality_trace.hpp): allocated by the first traced smgpu_iterate.  Its
// geometry launch writes cell centres of its own and reads a stop word of its own (always 0): nothing the loop reads is written
struct QualityTraceHost {
    int interval = 0;                       // 0: off
    int64_t since = 0;                      // smgpu_handle::iterCount at switching on: a record's number is the count less this
    bool fusedWanted = true;                // SMGPU_QUALITY_TRACE_FUSED=0: the report's launches instead of k_quality_geom_tile
    QualityThresholds thr{};
    DevBlock block;
    double* cellCtr = nullptr;
    Accum* acc = nullptr;
    QFace* facePart = nullptr;
    QCell *cellPart = nullptr, *cellFold = nullptr;
    RecordSlab<smgpu_quality_trace_record> slab{"quality trace"};   // one record per due iteration of the call
    void release() { block.release(); slab.release(); }
};

// The guard on the trace (smgpu_set_quality_guard, kernels_quality_guard.hpp): allocated at arming.  pts / normal: the snapshot;
// rec: the record slot of the baseline; state: what smgpu_get_quality_guard answers
struct QualityGuardHost {
    bool armed = false;
    bool refining = false;                  // inside the search for the last good iteration: smgpu_iterate's body leaves no trace
    bool tripPending = false;               // the call that just read back tripped: roll back before it returns
    int lastVerdict = 0;                    // the verdict word after the last read-back
    smgpu_quality_guard_params prm{SMGPU_GUARD_NONPOSITIVE_VOLUME | SMGPU_GUARD_WRONG_ORIENTED, 1};
    smgpu_quality_guard_state state{};
    DevBlock block;
    GuardDev* dev = nullptr;
    smgpu_quality_trace_record* rec = nullptr;
    double *pts = nullptr, *normal = nullptr;
    void release() { block.release(); }
};

// The tangle constraint (smgpu_set_tangle_constraint, kernels_quality_tangle.hpp): allocated at enabling.  exempt: one byte per
// cell; marks: one per point (rounded up to whole words); cellCtr / acc: as the trace's, for the evaluation without tiles
struct TangleHost {
    bool on = false;
    int passes = 2;
    int64_t since = 0, nExempt = 0;         // smgpu_handle::iterCount at enabling (numbers as the trace's); exempt cells
    DevBlock block;
    uint8_t *exempt = nullptr, *marks = nullptr;
    TangleDev* dev = nullptr;
    double* cellCtr = nullptr;
    Accum* acc = nullptr;
    RecordSlab<smgpu_tangle_record> slab{"tangle constraint"};       // one record per iteration of the call
    // the coupled form (smgpu_set_tangle_constraint_coupled, 10.13) on an engine with a halo.  The host drives the passes, so the
    // state of the iteration in hand lives here: x (the buffer that holds the points the iteration started from), the pass
    // counter k (-1: no iteration waits for its passes), the reverting passes so far, the rank's count at k = 0.  count: the
    // iterations closed since enabling (smgpu_handle::iterCount does not move under a halo).  The slab is used in chunks of
    // kChunk records: slabUsed of them are written, slabFresh says the chunk has been zeroed and nothing of it read back.
    static constexpr int kChunk = 256;
    bool coupled = false, passOpen = false, slabFresh = false;
    int k = -1, reverting = 0, slabUsed = 0;
    int64_t count = 0, nBad0 = 0;
    const double* x = nullptr;
    uint8_t* counted = nullptr;             // one byte per shared point: 0 where a lower rank shares it (nPointsReverted)
    int *sendT = nullptr, *recvT = nullptr; // the caller's exchange buffers (device, nSend / nRecv int32)
    void release() { block.release(); slab.release(); coupled = passOpen = slabFresh = false; k = -1; slabUsed = 0; }
};

// The tiered structs of the quality constraint (include/smgpu.h, 10.14 - 10.19): every narrower struct is the head of the next
// wider one.  quality_loop.hpp relies on it: a setter widens its argument by copying it over the head of the widest defaults, a
// getter answers with the head of the widest struct.  QC_HEAD_OF asserts it completely: the fields listed tile the narrow
// struct with nothing between them but alignment (none is left out), each has the same offset and size in the wide one, and the
// first field the wide one adds sits at sizeof(narrow).
struct QcFieldAt { size_t narrow, wide, size, wideSize; };
template <size_t N>
constexpr bool qcHeadOf(const QcFieldAt (&f)[N], size_t narrowSize, size_t narrowAlign, size_t firstAdded) {
    size_t end = 0;
    for (size_t i = 0; i < N; ++i) {
        const size_t a = f[i].size < narrowAlign ? f[i].size : narrowAlign;   // scalars and pointers: aligned to their size
        if (f[i].narrow != (end + a - 1) / a * a || f[i].wide != f[i].narrow || f[i].wideSize != f[i].size) return false;
        end = f[i].narrow + f[i].size;
    }
    return (end + narrowAlign - 1) / narrowAlign * narrowAlign == narrowSize && firstAdded == narrowSize;
}
#define QC_FIELD(N, W, f) {offsetof(N, f), offsetof(W, f), sizeof(N::f), sizeof(W::f)},
#define QC_HEAD_OF(N, W, FIELDS, added)                                                                                        \
    static_assert([] { constexpr QcFieldAt at[] = {FIELDS(QC_FIELD, N, W)}; return qcHeadOf(at, sizeof(N), alignof(N), offsetof(W, added)); }(), \
                  #N " is the head of " #W)
#define QC_PARAMS_FIELDS(X, N, W) X(N, W, maxNonOrtho) X(N, W, maxInternalSkewness) X(N, W, maxBoundarySkewness) X(N, W, passes)
#define QC_LIMITS_FIELDS(X, N, W)                                                                                              \
    QC_PARAMS_FIELDS(X, N, W) X(N, W, minTetQuality) X(N, W, minTwist) X(N, W, minTriangleTwist) X(N, W, minFaceWeight) X(N, W, minVolRatio) X(N, W, minDeterminant)
#define QC_RECORD_FIELDS(X, N, W)                                                                                              \
    X(N, W, iteration) X(N, W, passes) X(N, W, fullRevert) X(N, W, nBadCells) X(N, W, nPointsReverted) X(N, W, nTangledCells) X(N, W, nNonOrthoFaces) X(N, W, nSkewFaces)
#define QC_RECORD_FULL_FIELDS(X, N, W)                                                                                         \
    QC_RECORD_FIELDS(X, N, W) X(N, W, nLowTetFaces) X(N, W, nLowTwistFaces) X(N, W, nLowTriangleTwistFaces) X(N, W, nLowWeightFaces) X(N, W, nLowVolRatioFaces) X(N, W, nUnderdeterminedCells)
#define QC_RECORD_ALL_FIELDS(X, N, W) QC_RECORD_FULL_FIELDS(X, N, W) X(N, W, nConcaveFaces) X(N, W, nWarpedFaces) X(N, W, nSmallAreaFaces) X(N, W, nSmallVolumeCells)
#define QC_STATE_FIELDS(X, N, W)                                                                                               \
    X(N, W, on) X(N, W, passes) X(N, W, maxNonOrtho) X(N, W, maxInternalSkewness) X(N, W, maxBoundarySkewness) X(N, W, nExemptCells) X(N, W, nExemptFaces) X(N, W, iteration)
#define QC_STATE_FULL_FIELDS(X, N, W)                                                                                          \
    QC_STATE_FIELDS(X, N, W) X(N, W, minTetQuality) X(N, W, minTwist) X(N, W, minTriangleTwist) X(N, W, minFaceWeight) X(N, W, minVolRatio) X(N, W, minDeterminant) X(N, W, nExemptDeterminantCells)
#define QC_STATE_ALL_FIELDS(X, N, W) QC_STATE_FULL_FIELDS(X, N, W) X(N, W, maxConcave) X(N, W, minFlatness) X(N, W, minVol) X(N, W, minArea) X(N, W, nExemptVolumeCells)
#define QC_HALO_FIELDS(X, N, W) X(N, W, sendT) X(N, W, recvT) X(N, W, sendCc) X(N, W, recvCc) X(N, W, coupling)
QC_HEAD_OF(smgpu_quality_constraint_params, smgpu_quality_constraint_limits, QC_PARAMS_FIELDS, minTetQuality);
QC_HEAD_OF(smgpu_quality_constraint_limits, smgpu_quality_constraint_limits_all, QC_LIMITS_FIELDS, maxConcave);
QC_HEAD_OF(smgpu_quality_constraint_record, smgpu_quality_constraint_record_full, QC_RECORD_FIELDS, nLowTetFaces);
QC_HEAD_OF(smgpu_quality_constraint_record_full, smgpu_quality_constraint_record_all, QC_RECORD_FULL_FIELDS, nConcaveFaces);
QC_HEAD_OF(smgpu_quality_constraint_record_all, smgpu_quality_constraint_record_scaled, QC_RECORD_ALL_FIELDS, nScalePasses);
QC_HEAD_OF(smgpu_quality_constraint_state, smgpu_quality_constraint_state_full, QC_STATE_FIELDS, minTetQuality);
QC_HEAD_OF(smgpu_quality_constraint_state_full, smgpu_quality_constraint_state_all, QC_STATE_FULL_FIELDS, maxConcave);
QC_HEAD_OF(smgpu_quality_constraint_state_all, smgpu_quality_constraint_state_scaled, QC_STATE_ALL_FIELDS, scalePasses);
QC_HEAD_OF(smgpu_quality_constraint_halo_desc, smgpu_quality_constraint_halo_desc_full, QC_HALO_FIELDS, sendVc);
// the head of `wide` as the narrower struct Head, and a narrower struct (NULL: nothing) over the head of `wide`
template <class Head, class Wide>
static Head qcHead(const Wide& wide) {
    static_assert(sizeof(Head) <= sizeof(Wide), "a head is no longer than the struct");
    Head out;
    std::memcpy(&out, &wide, sizeof(Head));
    return out;
}
template <class Wide, class Head>
static Wide qcWiden(const Head* head, Wide wide) {
    static_assert(sizeof(Head) <= sizeof(Wide), "a head is no longer than the struct");
    if (head) std::memcpy(&wide, head, sizeof(Head));
    return wide;
}

// The quality constraint (smgpu_set_quality_constraint, kernels_quality_constraint.hpp): allocated at enabling.  exemptCell /
// cellFlag / tangled: one byte per cell; exemptFace: one per face; marks: one per point (rounded up to whole words); cellCtr / acc: the
// cell centres and the stop word of its geometry launches, with and without tiles
struct QualityConstraintHost {
    bool on = false;
    smgpu_quality_constraint_params prm{65.0, 4.0, 20.0, 2};
    QcLimits lim{};
    int64_t since = 0, nExemptCells = 0, nExemptFaces = 0;   // smgpu_handle::iterCount at enabling (numbers as the trace's)
    DevBlock block;
    uint8_t *exemptCell = nullptr, *exemptFace = nullptr, *cellFlag = nullptr, *tangled = nullptr, *marks = nullptr;
    QcDev* dev = nullptr;
    double* cellCtr = nullptr;
    Accum* acc = nullptr;
    // one record per iteration of the call, the widest for every entry; without the limits of 10.16 the six counts behind its
    // head, smgpu_quality_constraint_record, are 0, without those of 10.18 the four behind them, and without the scaling of 10.19
    // the three behind those
    RecordSlab<smgpu_quality_constraint_record_scaled> slab{"quality constraint"};
    // the scaling passes of 10.19 (smgpu_set_quality_constraint_scaling, kernels_quality_scale.hpp; serial form only), off while
    // scaling.scalePasses is 0.  Allocated when they are switched on: L, the points the loop produced (3 doubles per point), and
    // the two scale fields the sweeps alternate between (nScale doubles each: one per point, rounded up to an even number)
    smgpu_quality_constraint_scaling scaling{0, 4, 0.75};
    DevBlock scaleBlock;
    double *L = nullptr, *scaleA = nullptr, *scaleB = nullptr;
    long long nScale = 0;
    int maxGrid = 8192;                     // workgroups of a sweep / apply launch at most (kQsMaxGrid; SMGPU_QS_MAX_GRID)
    // the scaling passes of the coupled form (10.20, smgpu_set_quality_constraint_scaling_coupled, kernels_quality_scale_coupled.hpp):
    // the same parameters, L and scale fields, in the same block, and with them the caller's tables of the shared points -- scRowOff /
    // scRowPt: the counted neighbours of every shared point (CSR, local ids, row order), scDeg: its degree in the whole mesh -- the
    // partial sums of a sweep (scPart, one double per shared point) and the caller's exchange buffers (sendS / recvS, device,
    // nSend / nRecv doubles).  State of the iteration in hand: kept (L and s = 1 are this iteration's), sCur / sNext (which field
    // is current), sweepsDue (sweep calls the pass in hand still waits for), nScaleRan (marked passes with k < S so far); stage 3:
    // behind smgpu_quality_constraint_pass_scale
    bool scaleCoupled = false, kept = false;
    int *scRowOff = nullptr, *scRowPt = nullptr, *scDeg = nullptr;
    double *scPart = nullptr, *sendS = nullptr, *recvS = nullptr, *sCur = nullptr, *sNext = nullptr;
    int sweepsDue = 0, nScaleRan = 0;
    int64_t scaleBad = 0;
    void releaseScaling() {
        scaleBlock.release(); scaling = smgpu_quality_constraint_scaling{0, 4, 0.75}; nScale = 0;
        scaleCoupled = kept = false; sendS = recvS = sCur = sNext = nullptr; sweepsDue = nScaleRan = 0;
    }
    // the limits of 10.16 (smgpu_set_quality_constraint_limits, kernels_quality_limits.hpp).  faceMore: a new face criterion is
    // on; cellMore: minVolRatio or minDeterminant is; with neither the launches are 10.14's.  vol, exemptDet: allocated with
    // cellMore, 8 bytes and 1 byte per cell
    QcMore more{-1e30, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0};
    bool faceMore = false, cellMore = false;
    int64_t nExemptDet = 0;
    // the limits of 10.18 (smgpu_set_quality_constraint_limits_all): maxConcave in degrees as given, its sine in shape; a face
    // criterion of theirs sets faceMore, minVol cellMore; exemptDet then holds a bit set (bit 0 determinant, bit 1 volume)
    double maxConcave = 180.0;
    QcShape shape{0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0};
    int64_t nExemptVol = 0;
    double* vol = nullptr;
    uint8_t* exemptDet = nullptr;
    // the coupled form (smgpu_set_quality_constraint_coupled, 10.15) on an engine with a halo: TangleHost's coupled members with
    // the same meaning (x, k, reverting, count, the slab in chunks, counted, sendT / recvT), and what the face verdicts add.
    // pending: enabled, the exempt faces not taken yet.  stage: 0 no pass open, 1 behind pass_begin, 2 behind pass_faces.  n0: the
    // rank's counts at k = 0 in the record's order from nBadCells on, as k_qc_close takes them.  procFace / slot: 10.4's tables of
    // the coupling given at enabling, the constraint's own copies: a report packed with another coupling releases only the report's.
    // coupled is set before the enabling evaluation: its kernels take the form from it (withQcCoupling, quality_loop.hpp).
    static constexpr int kChunk = 256;
    bool coupled = false, pending = false, slabFresh = false;
    int k = -1, stage = 0, reverting = 0, slabUsed = 0, nProc = 0;
    // (full: enabled through smgpu_set_quality_constraint_limits_coupled, 10.17, or _limits_all_coupled, 10.18, which the
    // refusal of the other coupled entry names; sendVc / recvVc: the caller's volume buffers, one double per processor face, used while minVolRatio is on)
    bool full = false;
    int64_t count = 0, n0[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double *sendVc = nullptr, *recvVc = nullptr;
    const double* x = nullptr;
    uint8_t* counted = nullptr;
    int *procFace = nullptr, *slot = nullptr;
    int *sendT = nullptr, *recvT = nullptr;        // the caller's exchange buffers (device, nSend / nRecv int32)
    double *sendCc = nullptr, *recvCc = nullptr;   // ... (device, 3 doubles per processor face, patch order)
    void release() { block.release(); releaseScaling(); slab.release(); coupled = pending = slabFresh = full = false; sendVc = recvVc = nullptr; k = -1; stage = 0; slabUsed = 0; nProc = 0; }
};
