/* smgpu.h -- C-ABI of the MI355X (gfx950) smoothing-iteration engine.
 *
 * Drop-in boundary for the hot path of tkeskita/smoothMesh: the body of the smoothing loop
 * src/smoothMesh.C:2257-2437 (cell-centre recompute, centroidalSmoothing :96-166,
 * aspectRatioSmoothing :548-593, constrainMaxStepLength :684-754, restrictEdgeShortening
 * :602-652, restrictMinEdgeAngleDecrease :900-930, restrictFaceAngleDeterioration :1320-1437,
 * restore/count :2384-2392, calculateResidual :1546-1570, mesh.movePoints :2399).
 *
 * The reference has no FFI: those are free functions over OpenFOAM types (const fvMesh&,
 * pointField&, boolList&) called from main().  A host (the bundled `smoothMesh` front-end in
 * smoothmesh_amd/csrc/host, or an OpenFOAM-linked main) hands over what a
 * polyMesh directory contains -- points, faces, owner, neighbour, point masks -- as plain
 * arrays; all other addressing is derived inside the library.
 *
 * Conventions: every call returns 0 on success, non-zero on error (message through
 * smgpu_last_error); the reference aborts the process on FatalError, the host does the same.
 * Host arrays are borrowed for the duration of the call only.  A handle owns one HIP device
 * stream and all its device memory; it is not thread-safe.  label = int32, scalar = f64,
 * point = 3 x f64 (AoS), boolList = 1 byte per element.
 */
#ifndef SMGPU_H
#define SMGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smgpu_handle smgpu_handle;

/* What createMesh.H (SM.C:1814-1818) + findInternalMeshPoints (SM.C:40-91) +
 * classifyBoundaryPoints (BPS.C:269-441) give the loop. */
typedef struct smgpu_mesh_desc {
    int32_t nPoints, nCells, nFaces, nInternalFaces;
    const double* points;           /* [3*nPoints]            mesh.points()                  */
    const int32_t* faceOffsets;     /* [nFaces+1]             CSR of mesh.faces()            */
    const int32_t* facePoints;      /* [faceOffsets[nFaces]]                                  */
    const int32_t* owner;           /* [nFaces]               polyMesh::faceOwner()          */
    const int32_t* neighbour;       /* [nInternalFaces]       polyMesh::faceNeighbour()      */
    const uint8_t* isInternalPoint;          /* [nPoints]  SM.C:1978-1979                    */
    const uint8_t* isSmoothingSurfacePoint;  /* [nPoints]  BPS.C:404-412; NULL = all false   */
    int32_t device;                 /* HIP device ordinal                                     */
    void* stream;                   /* hipStream_t to run on (with useCallerStream)           */
    int32_t useCallerStream;        /* 0: library creates its own stream and ignores `stream`;
                                       1: run on `stream` as given -- NULL then means the HIP null
                                       stream (what torch.cuda.current_stream() is by default)   */
} smgpu_mesh_desc;

/* Loop parameters, SM.C:1861-1890 (names as the command-line options). */
typedef struct smgpu_params {
    double maxStepLength;
    double relStepFrac;
    double minEdgeLength;
    int32_t totalMinFreeze;
    int32_t edgeAngleConstraint;
    int32_t faceAngleConstraint;
    double minAngle;   /* degrees */
    double maxAngle;   /* degrees */
} smgpu_params;

/* One line of "Smoothing iteration=N nFrozenPoints=M residual=R" (SM.C:2396). */
typedef struct smgpu_iter_stats {
    double residual;
    int32_t nFrozenPoints;
    /* Near-tie census of this iteration (0 in a normal run): comparisons of an angle with minAngle / maxAngle or with the point's
     * current angle (SM.C:923, 1367, 1391-1394, 1421-1424) whose two sides were 1 .. 4 ulp apart.  The engine's acos and the
     * reference's (glibc) may differ in the last bit, so only such a comparison could be decided differently by the reference. */
    int32_t nNearTies;
} smgpu_iter_stats;

/* Mesh sizes derived by the library (for byte accounting and logs). */
typedef struct smgpu_sizes {
    int64_t nPoints, nCells, nFaces, nInternalFaces, nEdges;
    int64_t nnzFacePoints, nnzPointCells, nnzPointPoints, nnzPointFaces, nnzEdgeFaces, nnzEdgeCells, nnzCellFaces;
    int64_t deviceBytes;
} smgpu_sizes;

/* Per-kernel accumulated device time (hipEvent, milliseconds) and launch counts. */
#define SMGPU_MAX_KERNELS 24
typedef struct smgpu_counters {
    int32_t nKernels;
    const char* name[SMGPU_MAX_KERNELS];
    double ms[SMGPU_MAX_KERNELS];
    int64_t launches[SMGPU_MAX_KERNELS];
    int64_t algoBytesPerLaunch[SMGPU_MAX_KERNELS];
    int64_t algoF64OpsPerLaunch[SMGPU_MAX_KERNELS];   /* FP64 VALU instructions (per element, not per wave) the
                                                         reference's arithmetic needs, sqrt = 22 and div = 11 as the
                                                         compiler expands them; 0 = not counted for this kernel    */
} smgpu_counters;

const char* smgpu_last_error(void);
const char* smgpu_version(void);

/* Build addressing on the host, upload everything.  Replaces the setup SM.C:1978-2021. */
int smgpu_create(const smgpu_mesh_desc* desc, smgpu_handle** out);
int smgpu_destroy(smgpu_handle* h);

int smgpu_get_sizes(smgpu_handle* h, smgpu_sizes* out);
/* getMeshStats (SM.C:1478-1541): min / max edge length of the current coordinates. */
int smgpu_mesh_stats(smgpu_handle* h, double* minEdgeLength, double* maxEdgeLength);
int smgpu_set_params(smgpu_handle* h, const smgpu_params* p);
/* Which OpenFOAM's primitiveMesh geometry the cell centres follow (row a3 of the scope table; the reference is built against
 * either line, Allwmake:47 / README.md:30, and inherits its makeFaceCentresAndAreas / makeCellCentresAndVols):
 * COM = OpenFOAM.com v2312-v2506 (default; fan triangles of a face weighted by their area magnitude), ORG = OpenFOAM.org 12
 * (weighted by the area projected on the face normal; pyramid volumes clamped at vSmall).  The environment variable
 * SMGPU_FOAM_VARIANT=org selects ORG at smgpu_create.  Call before iterating. */
enum { SMGPU_FOAM_COM = 0, SMGPU_FOAM_ORG = 1 };
int smgpu_set_foam_variant(smgpu_handle* h, int32_t variant);
/* Multi-rank runs: which syncTools::syncPointList the shared-point combines of minMagSqrEqOp / maxMagSqrEqOp follow (SM.C:402-469
 * with isCloserPoint :246-272, OBB.C:359-365, :490-496).  MASTER (default) = globalMeshData::syncData, the form of every OpenFOAM
 * the reference builds against (Allwmake:47): the values of a point's sharers are folded ONCE, starting from the lowest rank's
 * value, in ascending rank order, and every sharer receives that result -- an exact tie hands the lower rank's vector to all, so a
 * rank can receive another rank's equal-length vector (the case isCloserPoint exists for) and a run cut through an exactly graded
 * mesh reproduces the serial aspect-ratio blend.  OWN = every sharer folds the others' values onto its own (a tie keeps the own
 * vector; the sharers may end with different vectors): the model of rounds 1-3 of this library, kept as the A/B.  The
 * environment variable SMGPU_SYNC_VARIANT=own selects OWN at smgpu_create.  The host-side combines of the step-wise set-ups
 * (smgpu_layers_shared / smgpu_boundary_shared) are the host's: smoothmesh_amd/halo.py and the smoothMesh front-end follow the
 * same switch.  Call before iterating. */
enum { SMGPU_SYNC_MASTER = 0, SMGPU_SYNC_OWN = 1 };
int smgpu_set_sync_variant(smgpu_handle* h, int32_t variant);

/* The loop SM.C:2257-2437 on one rank: up to nIters iterations, stops after the first iteration
 * whose residual < relTol (SM.C:2401).  stats (host, [nIters], may be NULL) receives one entry
 * per iteration done.  No host synchronisation happens inside the loop -- with one bounded exception while the face-angle
 * constraint is on: the form of the freeze-walk replay follows the number of points outside the good angle range the GPU has
 * published (updateWalkMode), and to bound how stale that number can be the host waits, every 8th iteration, for the iteration
 * it enqueued 8 iterations earlier (at most ~16 iterations are queued ahead; the GPU never idles).  The same holds for the
 * step-wise loop (smgpu_iter_begin). */
int smgpu_iterate(smgpu_handle* h, int32_t nIters, double relTol, smgpu_iter_stats* stats, int32_t* nDone);

/* smgpu_get_points also reports an error word a kernel raised since the last check (the step-wise loop below never
 * synchronises on its own): a non-zero return with smgpu_last_error() set. */
int smgpu_get_points(smgpu_handle* h, double* outPoints /* [3*nPoints] */);
/* Waits for the engine's stream and reports any error word a kernel has raised since the last check (a grid barrier or a
 * peer-store wait that timed out, a point without two usable neighbours SM.C:354-362, a projection failure BPS.C:932-938 ...).
 * The step-wise loop never synchronises on its own; hosts call this at the end of every chunk of iterations (smgpu_get_points
 * does the same check). */
int smgpu_check_error(smgpu_handle* h);
/* Near-tie census since smgpu_create (see smgpu_iter_stats::nNearTies; also counted in the step-wise multi-rank loop):
 * out = {total, edge-angle test SM.C:923, good-range test SM.C:1367, walk verdicts SM.C:1391-1394 / 1421-1424}.  The front-ends
 * print a warning when the total is not zero.  Window: SMGPU_NEARTIE_ULPS (default 4). */
int smgpu_get_near_ties(smgpu_handle* h, int64_t out[4]);
int smgpu_set_points(smgpu_handle* h, const double* points /* [3*nPoints] */);

/* ---- mesh quality report of the current points (DESIGN.md "Mesh quality") ------------------------------------------------
 * One pass on the device over the loop's own face centres / area vectors / cell centres: cell volumes, face areas,
 * non-orthogonality (degrees), skewness, face pyramids, cell openness and aspect ratio, after OpenFOAM primitiveMeshCheck.
 * Needs no smgpu_set_params; leaves points, freeze state, walk mode, statistics and the iteration count as they were.
 * Refused on an engine with a halo (a sub-domain's processor faces are internal faces of the global mesh).
 * Ties of the max / min ids go to the lowest id; every sum is reduced in a fixed order (bitwise repeatable).
 * p == NULL: the defaults 70 degrees, 4, 1e-6, 1000. */
typedef struct smgpu_quality_params { double nonOrthThreshold, skewThreshold, closedThreshold, aspectThreshold; } smgpu_quality_params;
typedef struct smgpu_quality {
    int64_t nCells, nFaces, nInternalFaces;
    double minVolume, maxVolume, totalVolume;  int64_t nNonPositiveVolume;  int32_t minVolumeCell;
    double minFaceArea, maxFaceArea;           int64_t nZeroAreaFaces;
    double maxNonOrth, avgNonOrth;             int64_t nSevereNonOrth, nErrorNonOrth;  int32_t maxNonOrthFace;
    double maxSkewness;                        int64_t nSkewFaces;  int32_t maxSkewFace;
    int64_t nWrongOrientedFaces;
    double maxOpenness;                        int64_t nOpenCells;
    double maxAspectRatio;                     int64_t nHighAspectCells;
} smgpu_quality;
int smgpu_mesh_quality(smgpu_handle* h, const smgpu_quality_params* p, smgpu_quality* out);
/* per-element field in polyMesh order: "cellVolume", "cellOpenness", "cellAspectRatio" [nCells], "faceNonOrthogonality"
 * (degrees, 0 on boundary faces), "faceSkewness" [nFaces].  out == NULL: size only (*n). */
int smgpu_quality_field(smgpu_handle* h, const char* name, double* out, int64_t* n);

/* ---- a quality history of the run (DESIGN.md "Mesh quality", 10.10) -----------------------------------------------------
 * smgpu_set_quality_trace(interval > 0) switches the trace on: smgpu_iterate then numbers the iterations that run 1, 2, ...
 * across its calls, and after every iteration whose number is a multiple of `interval` it queues the trace's launches on the
 * engine's stream, behind that iteration's movePoints.  They leave one record on the device; the records of a call come to the
 * host together with its smgpu_iter_stats -- no synchronisation is added to the loop -- and wait in the engine until
 * smgpu_get_quality_trace takes them.  An iteration that did not run (queued behind the stop by relTol) leaves no record and
 * does not advance the number; the iteration that met relTol did run.
 *
 * A record holds every field of smgpu_quality that does not depend on the order of a floating-point sum (totalVolume and
 * avgNonOrth are left out), and EVERY FIELD EQUALS, BIT FOR BIT, the field of that name smgpu_mesh_quality returns for the
 * same points; definitions, thresholds and lowest-id tie rules are the report's.
 *
 * smgpu_set_quality_trace: interval > 0 also sets the running number to 0 and discards unread records; interval == 0 switches
 * the trace off and frees its device memory (allocated by the first traced smgpu_iterate, outside deviceBytes like the
 * report's); interval < 0 is an error.  Refused on an engine with a halo; smgpu_halo_configure is refused while the trace is
 * on.  p == NULL: the defaults of smgpu_mesh_quality.  With the trace off nothing the engine launches changes; with it on,
 * the loop's kernels, results, smgpu_counters and timing events are what they are without it.
 * SMGPU_QUALITY_TRACE_FUSED=0 (read at smgpu_create), or an engine without tiles (SMGPU_TILES=0), queues the report's own
 * launches in place of the fused tile kernel: the records are identical.
 *
 * smgpu_get_quality_trace: out == NULL returns the number of pending records in *n; otherwise cap below that number is an
 * error that clears nothing; otherwise the records are copied in ascending `iteration`, *n is their number, and they are
 * cleared. */
typedef struct smgpu_quality_trace_record {
    int64_t iteration;                      /* 1-based running number since smgpu_set_quality_trace */
    double minVolume, maxVolume;   int64_t nNonPositiveVolume;  int32_t minVolumeCell;
    double minFaceArea, maxFaceArea;  int64_t nZeroAreaFaces;
    double maxNonOrth;             int64_t nSevereNonOrth, nErrorNonOrth;  int32_t maxNonOrthFace;
    double maxSkewness;            int64_t nSkewFaces;  int32_t maxSkewFace;
    int64_t nWrongOrientedFaces;
    double maxOpenness;            int64_t nOpenCells;
    double maxAspectRatio;         int64_t nHighAspectCells;
} smgpu_quality_trace_record;
int smgpu_set_quality_trace(smgpu_handle* h, int32_t interval, const smgpu_quality_params* p);   /* 0 = off; p NULL = defaults */
int smgpu_get_quality_trace(smgpu_handle* h, smgpu_quality_trace_record* out, int64_t cap, int64_t* n);

/* ---- a guard on the quality history (DESIGN.md "Mesh quality", 10.11) ----------------------------------------------------
 * smgpu_set_quality_guard(p, on != 0) arms the guard; it needs the trace on.  Arming runs the trace's own launches once on the
 * current points: the result is `baseline` (iteration 0), kept on the device; and it takes the first snapshot of those points,
 * numbered with the trace's running number (0 when the guard is armed directly after smgpu_set_quality_trace).  From then
 * on smgpu_iterate queues, behind the trace of every traced iteration, a verdict and a snapshot on the engine's stream:
 *   verdict   for each criterion in `criteria`: record.count > baseline.count, with the counts nNonPositiveVolume,
 *             nWrongOrientedFaces and nErrorNonOrth of the trace record -- integers only, so the host can repeat every verdict
 *             from the records.  A record that fails TRIPS the guard: the device sets the loop's stop word, and everything queued
 *             behind is the no-op the stop by relTol makes it.
 *   snapshot  after a record that passed: a copy of the per-point state an iteration carries to the next -- the points and,
 *             with smgpu_set_layers, the layer normals -- in buffers of the guard (allocated at arming, outside deviceBytes).
 * While armed smgpu_iterate closes every iteration with k_finish (the deferred finish of relTol <= 0 is off: one more K_FINISH
 * launch per iteration in smgpu_counters) and polls the stop word every eighth iteration, as with relTol > 0.  The results of an
 * armed run that does not trip -- points, statistics, trace records, near-tie census -- are those of the run without a guard, bit
 * for bit.
 *
 * A call of smgpu_iterate that trips returns the statistics and trace records of every iteration that ran, the tripping one
 * included (*nDone counts it).  Before it returns it restores the snapshot and, with `refine`, looks for the exact last
 * iteration that passes: from the snapshot it steps one iteration at a time, each followed by a trace and a verdict, at most
 * interval - 1 times; the first step that fails ends the search and the last state that passed is restored.  These steps leave
 * no statistics, no trace records, and nothing in smgpu_counters or the near-tie census.  restoredIteration is the largest r for
 * which every traced or refined iteration from the snapshot through r passed; the trace's running number becomes r, so that the
 * number names the points.  The guard then disarms itself; smgpu_get_quality_guard keeps answering.
 *
 * smgpu_quality_guard_restore is the same rollback on request, for callers who judge the trace by criteria of their own: to
 * snapshotIteration, without refining; the guard stays armed and the running number becomes snapshotIteration.  Pending trace
 * records stay.  Refused when the guard is not armed.
 *
 * Not covered: an engine with a halo (refused with the trace's wording; so smoothMesh -parallel and the smoothers of halo.py
 * have no guard) and an engine with boundary point smoothing (refused: its point normals are a running blend across
 * iterations and its corner lists are host state, neither of which the snapshot holds).  smgpu_set_boundary_smoothing and
 * smgpu_halo_configure are refused while the guard is armed; smgpu_set_quality_trace disarms it, because it restarts the
 * numbering.  on == 0 disarms and frees the guard's device memory. */
enum { SMGPU_GUARD_NONPOSITIVE_VOLUME = 1, SMGPU_GUARD_WRONG_ORIENTED = 2, SMGPU_GUARD_ERROR_NONORTH = 4 };
typedef struct smgpu_quality_guard_params { uint32_t criteria; int32_t refine; } smgpu_quality_guard_params;   /* NULL params = {1|2, 1} */
typedef struct smgpu_quality_guard_state {
    int32_t armed, tripped;  uint32_t reasons;
    int64_t snapshotIteration, trippedIteration, restoredIteration;      /* trace numbers; 0 = the points at arming */
    smgpu_quality_trace_record baseline, tripRecord;
} smgpu_quality_guard_state;
int smgpu_set_quality_guard(smgpu_handle* h, const smgpu_quality_guard_params* p, int32_t on);
int smgpu_get_quality_guard(smgpu_handle* h, smgpu_quality_guard_state* out);
int smgpu_quality_guard_restore(smgpu_handle* h);

/* ---- the tangle constraint (DESIGN.md "Mesh quality", 10.12) --------------------------------------------------------------
 * A constraint of the engine's own, in the style of the reference's three: a point stays at its current coordinates when its
 * move would turn a cell bad.  Opt-in; with it off nothing the engine launches or returns changes.
 *
 * x: the points an iteration of smgpu_iterate starts from.  x': the points it has produced after everything the loop does
 * without the constraint (proposal, layers, the reference's constraints, the freeze walk, movePoints).  C_f, S_f, C_c: the
 * engine's geometry of a set of points under the current foam variant.
 *
 * A cell c is BAD at a set of points if V_c <= VSMALL -- the report's V_c: the mean of the face centres by a plain division,
 * signed pyramids, no clamp under either variant, the cellFacesGeom order -- or if one of its own-side pyramids is <= 0:
 * S_f.(C_f - C_c) for a face it owns, S_f.(C_c - C_f) for a face it neighbours, the operands and operation order of the
 * report's pO and pN.  So a face is in wrongOrientedFaces exactly when its owner or its neighbour is bad through it.
 *
 * smgpu_set_tangle_constraint(p, on != 0) evaluates the current points once: the cells bad there are EXEMPT for as long as the
 * constraint stays on, even if they heal (one byte per cell); they never count and never mark.  (The reference requires an
 * untangled initial mesh; without the exemption one bad initial cell would freeze the whole run.)  p == NULL: passes = 2.
 *
 * Then, per iteration that ran, behind its movePoints:
 *   for k = 0 .. passes:  evaluate the geometry of x'; B = the cells that are bad and not exempt;
 *                         B empty: stop;
 *                         k == passes: x' = x for every point (the FULL REVERT), stop;
 *                         otherwise x'_p = x_p for every point p of every face of every cell in B.
 * INVARIANT: if no non-exempt cell is bad at x, none is bad at the accepted x' -- by induction, from the moment of enabling.
 * The accepted x' is what the next iteration, smgpu_get_points, the quality trace and the guard see; the trace's launches of an
 * iteration are queued behind the constraint's.  The iteration's residual and nFrozenPoints keep their meaning -- the loop's own
 * values, computed before the passes -- so a run whose remaining moves are all reverted never meets relTol.
 *
 * One smgpu_tangle_record per iteration that ran: `iteration` a running number since enabling, across smgpu_iterate calls, as
 * the trace numbers them; `passes` the evaluations that found B non-empty and reverted marked points; `fullRevert` whether the
 * full revert ran; `nBadCells` the size of B at k = 0; `nPointsReverted` the points with accepted x'_p == x_p whose loop result
 * differed from x_p.  The records stay on the device until the call's read-back; smgpu_get_tangle_records has the semantics of
 * smgpu_get_quality_trace (out == NULL: the number; a short cap is an error that clears nothing; ascending; a read clears).
 *
 * While on, smgpu_iterate adds no host synchronisation; it closes every iteration with k_finish, like an armed guard (one more
 * K_FINISH launch per iteration in smgpu_counters with relTol <= 0), because every launch of the constraint is gated on the
 * written bit of the iteration's statistics.  The evaluations after the first stay queued and return at once on a device word
 * once one has found B empty.  The constraint's launches stay outside smgpu_counters and the timing events; its memory is
 * allocated at enabling, outside deviceBytes: nCells + nPoints bytes, and 32 bytes per iteration of the longest call.
 * An engine without tiles (SMGPU_TILES=0) evaluates with the direct geometry kernels: identical points and records.
 *
 * Refused (with the trace's wording where one exists): an engine with a halo -- it takes the coupled form below, which the
 * smoothers of halo.py drive; smoothMesh -parallel has no option for it yet; an engine with boundary point smoothing; smgpu_halo_configure and smgpu_set_boundary_smoothing while
 * the constraint is on; passes < 0.  Layers, both foam variants, the trace and the guard go together with it: the guard's
 * snapshot gains nothing (the exempt mask is static), and its refining steps replay the constraint deterministically; their
 * records are dropped like their statistics.  When the guard rolls the points back (a trip, or smgpu_quality_guard_restore)
 * the constraint's running number goes back by as many iterations as the trace's, so the two keep naming the same points; the
 * records of the iterations that ran stand, like the trace's.  on == 0 switches it off, discards unread records and frees its memory. */
typedef struct smgpu_tangle_params { int32_t passes; } smgpu_tangle_params;   /* NULL params = {2} */
typedef struct smgpu_tangle_record {
    int64_t iteration;                      /* 1-based running number since smgpu_set_tangle_constraint */
    int32_t passes, fullRevert;
    int64_t nBadCells, nPointsReverted;
} smgpu_tangle_record;
typedef struct smgpu_tangle_state { int32_t on, passes;  int64_t nExemptCells, iteration; } smgpu_tangle_state;
int smgpu_set_tangle_constraint(smgpu_handle* h, const smgpu_tangle_params* p, int32_t on);
int smgpu_get_tangle_records(smgpu_handle* h, smgpu_tangle_record* out, int64_t cap, int64_t* n);
int smgpu_get_tangle_state(smgpu_handle* h, smgpu_tangle_state* out);

/* ---- the tangle constraint on a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.13) --------------------------
 * The contract above, read on the GLOBAL mesh, for an engine whose halo is configured.  x, x', "bad" and "exempt" are the
 * definitions above.  A cell is judged by its own volume and its own-side pyramids, a processor face needs no neighbour data,
 * cells are never duplicated and a rank holds x and x' of every one of its points behind smgpu_iter_end: the evaluation is
 * local.  Two things cross ranks: the MARKS (a shared point marked by a bad cell of one rank goes back on every rank that holds
 * it) and the VERDICT ("B is empty", "this pass is the full revert": statements about the whole mesh).
 *
 * Exempt cells: one evaluation per rank at enabling; copies of shared points are identical, so this is the global mesh's answer.
 * Per iteration, behind every rank's smgpu_iter_end, for k = 0 .. passes:
 *   1. every rank evaluates its x'; B = the union of the ranks' bad cells that are not exempt;
 *   2. B empty on all ranks: stop;
 *   3. k == passes: every point of every rank goes back to x (the full revert), stop;
 *   4. otherwise every point of every face of every cell in B goes back, on every rank that holds a copy of it.
 * INVARIANT: the one above, on the global mesh; copies of a shared point stay bit-identical after every pass.
 *
 * The calls, on every rank, after smgpu_iter_end and before the next smgpu_iter_begin (which refuses while passes are due):
 *   smgpu_tangle_pass_begin   evaluates the points the engine holds, packs the mark of every shared point into its send slots
 *                             of sendT (int32, 0 / 1) and returns the rank's count of bad cells that are not exempt -- the one
 *                             host read of the pass; sendT is complete when it returns.
 *   the host                  sums the counts over ALL ranks; if the sum is positive and this is not the last pass (k < passes)
 *                             it moves sendT -> recvT exactly as it moves exchange F (on the exchange stream, if one is set).
 *   smgpu_tangle_pass_end     nBadGlobal == 0: closes the record, *done = 1.  k == passes: the full revert, the record closes,
 *                             *done = 1.  Otherwise ORs recvT into the marks of the shared points through combOffsets /
 *                             combSlots, applies the marked revert, *done = 0: the host begins the next pass.
 * The engine keeps k; a call out of order is an error.  The verdict is the host's on purpose: a clean iteration costs one
 * evaluation, one pack and one small closing launch, and none of the serial form's queued no-op passes.  With the peer-store
 * transport the T records still travel by the host's exchange.
 *
 * One smgpu_tangle_record per iteration and rank: `passes` and `fullRevert` are the global values, the same on every rank;
 * `nBadCells` is the rank's own count at k = 0; `nPointsReverted` the rank's own count, a shared point counting only on its
 * master, the lowest-rank sharer (the first entry of its combSlots row is -1).  Summed over the ranks (passes and fullRevert
 * taken from any one) they are the record of the undecomposed mesh.  smgpu_get_tangle_records and smgpu_get_tangle_state serve
 * both forms (nExemptCells: the rank's own; the records wait on the device until they are asked for, which synchronises).
 * residual and nFrozenPoints stay the loop's own values, as above.
 *
 * Goes together with layers, both foam variants, both sync variants, every transport and arrangement of the iteration.  Refused:
 * an engine without a halo (smgpu_set_tangle_constraint is its form, and keeps refusing an engine with one), boundary point
 * smoothing, passes < 0, a call between smgpu_iter_begin and smgpu_iter_end.  The trace and the guard stay refused on an engine
 * with a halo.  Memory, allocated at enabling outside deviceBytes: nCells + nPoints + nShared bytes and 8 KiB of records; the
 * caller owns sendT / recvT, 4 (nSend + nRecv) bytes.  on == 0 (either entry point) switches it off and releases everything. */
typedef struct smgpu_tangle_halo_desc { void* sendT; void* recvT; } smgpu_tangle_halo_desc;   /* device, nSend / nRecv int32, caller-owned */
int smgpu_set_tangle_constraint_coupled(smgpu_handle* h, const smgpu_tangle_params* p, const smgpu_tangle_halo_desc* d, int32_t on);
int smgpu_tangle_pass_begin(smgpu_handle* h, int64_t* nBadLocal);                 /* after smgpu_iter_end */
int smgpu_tangle_pass_end(smgpu_handle* h, int64_t nBadGlobal, int32_t* done);

/* ---- the quality constraint (DESIGN.md "Mesh quality", 10.14) --------------------------------------------------------------
 * The tangle constraint with up to three more criteria, taken from meshQualityDict: a point also stays at its current coordinates
 * when its move would push a face's non-orthogonality or skewness over a limit.  Opt-in; this entry is for an engine without a halo
 * (smgpu_set_quality_constraint_coupled below is the form for an engine with one);
 * with it off nothing the engine launches, prints or returns changes.
 *
 * Notation is the tangle constraint's (10.12): x are the points an iteration starts from, x' the points the loop produced, C_f,
 * S_f, C_c the engine's geometry of a set of points under the current foam variant.  ortho_f and skew_f are the report's values
 * (10.1) with the same operands and operation order as k_quality_faces; ortho_f exists for internal faces only, and the boundary
 * form of d applies to skew_f on boundary faces.
 *
 * PARAMETERS.  passes: an integer >= 0, default 2.  maxNonOrtho: degrees, default 65; a value >= 180 switches the criterion off.
 * maxInternalSkewness: default 4; a value <= 0 switches it off.  maxBoundarySkewness: default 20; a value <= 0 switches it off.
 * cosT = cos(maxNonOrtho) is formed exactly as the report forms its cosine: cos(maxNonOrtho * (pi / 180)) in double on the host.
 *
 * A face is BAD when it is internal and ortho_f < cosT (this includes ortho_f <= 0), or internal and skew_f > maxInternalSkewness,
 * or a boundary face and skew_f > maxBoundarySkewness.
 * A cell is BAD when 10.12's definition applies (V_c <= VSMALL or an own-side pyramid <= 0), or when it is the owner or the
 * neighbour of a bad face that is not exempt.
 *
 * EXEMPTION.  Enabling evaluates the current points once.  The cells bad there by 10.12's definition are exempt, as they are
 * under the tangle constraint; the faces bad there are exempt.  An exemption lasts for as long as the constraint stays on, even
 * if the element heals.  Exempt cells never count through their own volume or pyramids; exempt faces never make a cell bad.  A
 * cell that is exempt as a cell can still be bad through a bad face that is not exempt.
 *
 * Per iteration that ran, behind its movePoints, the loop is 10.12's with B = the bad cells of this definition:
 *   for k = 0 .. passes:  B empty: stop;  k == passes: x' = x everywhere (the FULL REVERT);
 *                         otherwise x'_p = x_p for every point p of every face of every cell in B.
 * Reverting all points of a bad face's owner and neighbour restores that face's C_O, C_N, C_f and S_f to their bits at x, so
 * 10.12's INVARIANT carries over: if no non-exempt face or cell is bad at x, none is bad at the accepted x'.
 * EQUIVALENCE.  With all three criteria off the accepted points of every iteration are bit for bit the tangle constraint's, and
 * so are passes, fullRevert, nBadCells and nPointsReverted.
 *
 * Unchanged from 10.12: residual and nFrozenPoints keep the loop's own values; the trace and the guard see the accepted points
 * and their launches are queued behind the constraint's; no host synchronisation enters the loop; every launch is gated on the
 * written bit of the iteration's statistics and on the "clean" word; a guard rollback takes the running number back.
 *
 * One smgpu_quality_constraint_record per iteration that ran: iteration, passes, fullRevert, nPointsReverted with 10.12's
 * meaning; nBadCells: |B| at k = 0, each cell counted once; nTangledCells: the cells bad by 10.12's definition alone at k = 0;
 * nNonOrthoFaces / nSkewFaces: the bad faces that are not exempt at k = 0 by the non-orthogonality criterion / by the skewness
 * criteria (a face that fails both counts in both).  smgpu_get_quality_constraint_records has the semantics of
 * smgpu_get_tangle_records.  The record begins with smgpu_tangle_record's five fields at the same offsets.
 *
 * Refused: a halo, boundary point smoothing, passes < 0 (10.12's refusals, in their wording); a NaN limit; enabling while the
 * tangle constraint is on, and enabling the tangle constraint while this one is on; smgpu_halo_configure and
 * smgpu_set_boundary_smoothing while it is on.  Layers, both foam variants, the trace and the guard go together with it.
 * Memory, allocated at enabling outside deviceBytes: 3 nCells + nFaces + nPoints bytes, 24 nCells bytes of cell centres, the
 * report's owner / neighbour lists if no report has made them (4 (nFaces + nInternalFaces) bytes), and 56 bytes per iteration of
 * the longest call.  p == NULL: the defaults.  on == 0 switches it off, discards unread records and frees its memory. */
typedef struct smgpu_quality_constraint_params {
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int32_t passes;
} smgpu_quality_constraint_params;            /* NULL params = {65, 4, 20, 2} */
typedef struct smgpu_quality_constraint_record {
    int64_t iteration;                      /* 1-based running number since smgpu_set_quality_constraint */
    int32_t passes, fullRevert;
    int64_t nBadCells, nPointsReverted;
    int64_t nTangledCells, nNonOrthoFaces, nSkewFaces;
} smgpu_quality_constraint_record;
typedef struct smgpu_quality_constraint_state {
    int32_t on, passes;
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int64_t nExemptCells, nExemptFaces, iteration;
} smgpu_quality_constraint_state;
int smgpu_set_quality_constraint(smgpu_handle* h, const smgpu_quality_constraint_params* p, int32_t on);
int smgpu_get_quality_constraint_records(smgpu_handle* h, smgpu_quality_constraint_record* out, int64_t cap, int64_t* n);
int smgpu_get_quality_constraint_state(smgpu_handle* h, smgpu_quality_constraint_state* out);

/* ---- the quality constraint: the tet, twist, weight, ratio and determinant limits (DESIGN.md "Mesh quality", 10.16) ---------
 * Six more criteria of meshQualityDict for the constraint above, for an engine without a halo.  All are off unless asked for; they
 * are judged behind every iteration by the reports' own measures and act through 10.14's loop, unchanged.  Notation and everything
 * not said here is 10.14's.
 *
 * VALUES, at the points being judged, with the operands and the operation order of the report kernels, so the bits of the report
 * fields: tet_f = faceTetQuality (10.7: the face-centre tets of both sides); tw_f = faceTwist and tri_f = faceTriangleTwist (faces
 * with more than 3 vertices only: a triangle is never bad by them); w_f = faceWeight and r_f = faceVolumeRatio (10.6, internal
 * faces only); det_c = cellDeterminant (10.6); V_c, which r_f needs, has the bits of the report's cell volumes.
 *
 * LIMITS.  A face is also BAD when
 *   tet_f < minTetQuality                        (any face;        off when minTetQuality    <= -1e30)
 *   tw_f  < minTwist                             (> 3 vertices;    off when minTwist         <= -1)
 *   tri_f < minTriangleTwist                     (> 3 vertices;    off when minTriangleTwist <= -1)
 *   it is internal and w_f < minFaceWeight       (                 off when minFaceWeight    <= 0)
 *   it is internal and r_f < minVolRatio         (                 off when minVolRatio      <= 0)
 * and a cell is also BAD when it is the owner or the neighbour of a face bad by one of these and not exempt, or when
 *   det_c < minDeterminant and the cell is not determinant-exempt      (off when minDeterminant <= 0).
 * The comparisons are the reports' own, strict.  A NaN limit is refused.  The defaults are all off.
 *
 * EXEMPTION.  Enabling evaluates the current points once.  A face bad there by any criterion that is on, of 10.14 or of this
 * section, is exempt: one byte per face, as in 10.14.  A cell under-determined there is exempt from the determinant criterion
 * only, in a byte of its own: it is no exempt cell in 10.12's sense and can still be bad through its volume, its pyramids or a
 * face.
 *
 * INVARIANT.  10.14's carries over: reverting every point of a bad face's owner and neighbour restores that face's points, C_f,
 * S_f, C_O, C_N, V_O and V_N to their bits at x, and with them all five face values; reverting every point of a cell restores the
 * S_f of its faces, and with them det_c.  So if no non-exempt face or cell is bad at x, none is bad at the accepted x'.
 * EQUIVALENCE.  With all six off the accepted points, the records and the state are bit for bit those of
 * smgpu_set_quality_constraint with the same three limits, and the engine queues exactly its launches: no further kernel.
 *
 * smgpu_quality_constraint_limits: smgpu_quality_constraint_params' four fields at their offsets, then the six limits.  NULL:
 * {65, 4, 20, 2} and six off values.  smgpu_set_quality_constraint_limits has the refusals of smgpu_set_quality_constraint, and
 * the two entries and the tangle constraint exclude each other as the one entry and the tangle constraint do; on == 0 is
 * smgpu_set_quality_constraint's.
 * smgpu_quality_constraint_record_full: the record above (56 bytes), then, at k = 0, the bad faces that are not exempt by tet
 * quality, twist, triangle twist, weight and volume ratio (a face that fails several counts in each) and the under-determined
 * cells that are not determinant-exempt.  Both getters drain the same pending records; the narrow one returns each record's
 * first 56 bytes.  smgpu_quality_constraint_state_full: the state above, then the six limits and the determinant-exempt cells.
 * Under smgpu_set_quality_constraint (and the coupled form) the new counts are 0 and the limits the off values.
 *
 * Not covered: the base-point tets (their walk is O(nv^2) per face and stays with the report), reading system/meshQualityDict;
 * maxConcave, minFlatness, minVol and minArea are smgpu_set_quality_constraint_limits_all's (10.18, below).  On a decomposed mesh
 * smgpu_set_quality_constraint_coupled takes the three limits of 10.14 only; smgpu_set_quality_constraint_limits_coupled (10.17,
 * below) takes all nine.
 * Memory, beyond 10.14's: 104 bytes per iteration of the longest call in place of 56; with minVolRatio or minDeterminant on,
 * 8 nCells bytes of volumes and nCells bytes of determinant exemptions. */
typedef struct smgpu_quality_constraint_limits {
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int32_t passes;
    double minTetQuality, minTwist, minTriangleTwist, minFaceWeight, minVolRatio, minDeterminant;
} smgpu_quality_constraint_limits;            /* NULL limits = {65, 4, 20, 2, -1e30, -1, -1, 0, 0, 0} */
typedef struct smgpu_quality_constraint_record_full {
    int64_t iteration;
    int32_t passes, fullRevert;
    int64_t nBadCells, nPointsReverted;
    int64_t nTangledCells, nNonOrthoFaces, nSkewFaces;
    int64_t nLowTetFaces, nLowTwistFaces, nLowTriangleTwistFaces, nLowWeightFaces, nLowVolRatioFaces, nUnderdeterminedCells;
} smgpu_quality_constraint_record_full;
typedef struct smgpu_quality_constraint_state_full {
    int32_t on, passes;
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int64_t nExemptCells, nExemptFaces, iteration;
    double minTetQuality, minTwist, minTriangleTwist, minFaceWeight, minVolRatio, minDeterminant;
    int64_t nExemptDeterminantCells;
} smgpu_quality_constraint_state_full;
int smgpu_set_quality_constraint_limits(smgpu_handle* h, const smgpu_quality_constraint_limits* p, int32_t on);
int smgpu_get_quality_constraint_records_full(smgpu_handle* h, smgpu_quality_constraint_record_full* out, int64_t cap, int64_t* n);
int smgpu_get_quality_constraint_state_full(smgpu_handle* h, smgpu_quality_constraint_state_full* out);

/* ---- the quality constraint on a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.15) -------------------------
 * The contract above (10.14), read on the GLOBAL mesh, for an engine whose halo is configured.  Unlike the tangle verdict of
 * 10.13 a face limit is not local to a rank: a PROCESSOR FACE is an internal face of the global mesh.  It takes the internal-face
 * definitions of ortho_f and skew_f with C_N = the neighbour rank's owner cell centre at the points being judged, and is tested
 * against maxNonOrtho and maxInternalSkewness, never against maxBoundarySkewness.  Physical boundary faces and internal faces are
 * judged as in 10.14.  processorCyclic patches and two patches to one neighbour stay refused, as for the coupled report.
 *
 * WHO JUDGES.  Both ranks that hold a processor face judge it, each on its own geometry; a rank that finds it bad (and not
 * exempt) flags its own cell, the face's owner in that sub-domain.  Reversing a face and swapping its cells leaves both values
 * unchanged to rounding, so the two sides agree EXCEPT WITHIN ROUNDING OF A LIMIT: at such a tie only one side's cell goes back
 * in that pass.  The loop still ends, at the latest with the full revert, and the invariant then holds in each rank's own
 * verdicts.  (A single-sided verdict would cost a third exchange per pass.)
 *
 * EXEMPTION.  Enabling evaluates the current points once on every rank, with one exchange of cell centres; a face bad there is
 * exempt on each rank that holds it; cells are exempt as in 10.13.
 * Per iteration, behind every rank's smgpu_iter_end, for k = 0 .. passes: 10.13's loop with B = the union of the ranks' bad cells
 * by the definition above; the marks of shared points and the verdict travel exactly as in 10.13.
 * INVARIANT: 10.14's, on the global mesh; copies of a shared point stay bit-identical after every pass.
 *
 * The calls, on every rank (a call out of order is an error):
 *   smgpu_set_quality_constraint_coupled(on != 0)  evaluates the current points, packs the owner cell centre of every processor
 *                             face into sendCc (patch order of `coupling`, as smgpu_quality_coupled_pack) and returns with sendCc
 *                             complete; the constraint is pending.
 *   the host                  moves sendCc -> recvCc as for the coupled report.
 *   smgpu_quality_constraint_coupled_exempt        the face verdicts with recvCc become the exempt faces; the constraint is on.
 * and behind every smgpu_iter_end, before the next smgpu_iter_begin (which refuses while passes are due), for each pass:
 *   smgpu_quality_constraint_pass_begin   the geometry of the points the engine holds into buffers of the constraint's own, the
 *                             pack of ITS cell centres into sendCc; returns with sendCc complete.
 *   the host                  moves sendCc -> recvCc (on the exchange stream, if one is set).
 *   smgpu_quality_constraint_pass_faces   the face verdicts with recvCc, the cells, the marks, the pack of sendT; returns the
 *                             rank's count of bad cells, with sendT complete.
 *   the host                  sums the counts over ALL ranks; sum > 0 and k < passes: moves sendT -> recvT as exchange F.
 *   smgpu_quality_constraint_pass_end     as smgpu_tangle_pass_end.
 *
 * One smgpu_quality_constraint_record per iteration and rank: passes and fullRevert are the global values; nBadCells and
 * nTangledCells the rank's own at k = 0; nPointsReverted the rank's own, a shared point counting on its master only (10.13);
 * nNonOrthoFaces / nSkewFaces the rank's own, a processor face counting only on the side with myRank < neighbRank.  Summed over
 * the ranks they are the record of the undecomposed mesh.  nExemptFaces of the state follows the same counted-once rule,
 * nExemptCells is the rank's own.  smgpu_get_quality_constraint_records / _state serve both forms.
 * EQUIVALENCES.  All three criteria off: the coupled tangle constraint's points and shared record fields, bit for bit.  A single
 * sub-domain without processor patches: the serial constraint's run, bit for bit.
 *
 * Goes together with layers, both foam variants, both sync variants, every transport and arrangement of the iteration.  Refused:
 * an engine without a halo (smgpu_set_quality_constraint is its form, and keeps refusing an engine with one), boundary point
 * smoothing, passes < 0, a NaN limit, a null buffer that is needed, a call between smgpu_iter_begin and smgpu_iter_end, enabling
 * while either tangle form is on and vice versa, smgpu_halo_configure while it is on.  The trace and the guard stay refused on an
 * engine with a halo.  Memory, allocated at enabling outside deviceBytes: 10.14's, plus nShared bytes, 4 (nProcFaces +
 * nBoundaryFaces) bytes of tables of its own (a coupled report packed with another coupling does not disturb them) and 14 KiB of
 * records; the caller owns the four exchange buffers.  on == 0 (either entry point) switches it off and releases everything. */
struct smgpu_quality_coupling;
typedef struct smgpu_quality_constraint_halo_desc {
    void *sendT, *recvT;                    /* device, nSend / nRecv int32, as smgpu_tangle_halo_desc */
    void *sendCc, *recvCc;                  /* device, 3 doubles per processor face in patch order, as smgpu_quality_coupled_pack */
    const struct smgpu_quality_coupling* coupling;   /* the processor patches (below); read during the call only */
} smgpu_quality_constraint_halo_desc;
int smgpu_set_quality_constraint_coupled(smgpu_handle* h, const smgpu_quality_constraint_params* p, const smgpu_quality_constraint_halo_desc* d, int32_t on);
int smgpu_quality_constraint_coupled_exempt(smgpu_handle* h);
int smgpu_quality_constraint_pass_begin(smgpu_handle* h);                                   /* after smgpu_iter_end */
int smgpu_quality_constraint_pass_faces(smgpu_handle* h, int64_t* nBadLocal);
int smgpu_quality_constraint_pass_end(smgpu_handle* h, int64_t nBadGlobal, int32_t* done);

/* ---- the six further limits on a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.17) --------------------------
 * 10.16 read on the GLOBAL mesh, for an engine whose halo is configured.  Everything not said here is 10.15's (passes, marks,
 * verdict, hazards, refusals) and 10.16's (values, strict <, off values, exemption bytes).
 *
 * PROCESSOR FACE (a slot >= 0 in the coupling).  It takes the internal-face branch of every face criterion, with the decomposed
 * reports' definitions (10.8): the tets with the neighbour side from the received C_N, the twist with d = C_N - C_O, the weight
 * with dN from the received C_N, the volume ratio with the received signed V_N; the triangle twist is local.  It is tested
 * against minFaceWeight and minVolRatio like an internal face.  A physical boundary face is judged as in 10.16.
 * CELL DETERMINANT.  Over the cell's internal AND processor faces, as the decomposed -allGeometry report forms it; S_f is local,
 * so nothing travels for it.
 * WHO JUDGES, TIES, COUNTED ONCE: 10.15's.  Both ranks judge a processor face, each flags its own owner cell; the new face
 * counts of the record and the face's share of nExemptFaces count only on the side with myRank < neighbRank;
 * nUnderdeterminedCells and nExemptDeterminantCells are the rank's own.  Summed over the ranks the full record and the state are
 * those of the undecomposed mesh under smgpu_set_quality_constraint_limits.
 * WHAT TRAVELS.  V_c of the owner cell of every processor face, one double per face in sendCc's slot order, only when minVolRatio
 * is on.  The volumes (and the determinant) are formed in the first half of an evaluation -- in smgpu_quality_constraint_pass_begin
 * and in the enabling call -- in front of the packs, so sendVc is complete where sendCc is and the host moves both in one step: a
 * pass still waits for its engine twice.
 * EQUIVALENCES.  All six off: smgpu_set_quality_constraint_coupled's run bit for bit -- points, records, state -- and exactly its
 * launches.  A single sub-domain without processor patches: the serial run under smgpu_set_quality_constraint_limits, bit for bit.
 *
 * smgpu_quality_constraint_halo_desc_full: smgpu_quality_constraint_halo_desc at its offsets, then sendVc / recvVc.
 * smgpu_quality_constraint_coupled_exempt and the three pass calls serve both entries, and so do the getters; the six counts and
 * nExemptDeterminantCells are filled under this entry and stay 0 and off under smgpu_set_quality_constraint_coupled.
 * Refused, naming smgpu_set_quality_constraint_limits_coupled: everything smgpu_set_quality_constraint_coupled refuses, a NaN
 * among the six, minVolRatio on with a null sendVc or recvVc (and a processor face), enabling while a tangle form is on.
 * Memory, beyond 10.15's: with minVolRatio or minDeterminant on 9 nCells bytes; the caller owns sendVc / recvVc (16 nProcFaces
 * bytes). */
typedef struct smgpu_quality_constraint_halo_desc_full {
    void *sendT, *recvT;
    void *sendCc, *recvCc;
    const struct smgpu_quality_coupling* coupling;
    void *sendVc, *recvVc;                  /* device, one double per processor face in sendCc's slot order; may be NULL while
                                               minVolRatio is off */
} smgpu_quality_constraint_halo_desc_full;
int smgpu_set_quality_constraint_limits_coupled(smgpu_handle* h, const smgpu_quality_constraint_limits* p,
                                                const smgpu_quality_constraint_halo_desc_full* d, int32_t on);

/* ---- the last four meshQualityDict limits: concavity, flatness, volume, area (DESIGN.md "Mesh quality", 10.18) -------------
 * 10.16 and 10.17 with four more criteria; everything not said here is theirs.  The values are taken at the points being judged,
 * with the operands and the operation order of the reports (smgpu_mesh_quality_geometry for concavity and flatness, |S_f| of the
 * face areas, V_c of smgpu_mesh_quality's cell volumes).  A face is also BAD when
 *   faceConcavity_f, evaluated with concaveThreshold = maxConcave, is > SMALL: a corner with both edges > SMALL,
 *     s >= sin(maxConcave) and (c/s).n < SMALL                         (degrees; off when maxConcave >= 180; < 0 refused)
 *   it is summed (nv > 3, |S_f| > ROOTVSMALL) and flat_f < minFlatness  (off when minFlatness <= 0)
 *   |S_f| < minArea                                                    (off when minArea     <= 0)
 * and a cell when it is the owner or the neighbour of such a face that is not exempt, or when
 *   V_c < minVol and the cell is not volume-exempt                     (off when minVol      <= 0: 10.12 holds V_c > 0).
 * sin(maxConcave) is formed as the geometry report forms sin(concaveThreshold).  Strict comparisons; NaN refused; all four off
 * by default.
 * EXEMPTION.  The face byte is set by any criterion that is on; a cell under minVol at enabling is exempt from the volume
 * criterion only (the determinant-exempt byte is a bit set: bit 0 determinant, bit 1 volume).
 * INVARIANT.  10.16's carries over: the three face values are functions of the face's own points and S_f, V_c of the cell's
 * points; reverting every point of a bad face's two cells, or of a bad cell, restores their bits at x.
 * EQUIVALENCE.  All four off: smgpu_set_quality_constraint_limits' (coupled: _limits_coupled's) run bit for bit -- points,
 * records, state -- and exactly its launches.
 * On a sub-domain (smgpu_set_quality_constraint_limits_all_coupled) a processor face is judged on the rank's own vertex order,
 * flags its owner only and counts on the counted side; nothing new travels.
 *
 * smgpu_quality_constraint_limits_all: smgpu_quality_constraint_limits at its offsets, then the four.  NULL: the old NULL and
 * {180, 0, 0, 0}.  smgpu_quality_constraint_record_all: the full record (104 bytes), then at k = 0 the bad, non-exempt concave,
 * warped and small-area faces (a face that fails several counts in each) and the cells under minVol that are not volume-exempt.
 * smgpu_quality_constraint_state_all: the full state, then the four limits and the volume-exempt cells.  All getters drain the
 * one pending list; the narrower ones return each record's prefix.  Under the older entries the four counts are 0 and the four
 * limits at their off values.  Memory, beyond 10.16's: 136 bytes per record in place of 104; minVol on allocates what
 * minVolRatio does. */
typedef struct smgpu_quality_constraint_limits_all {
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int32_t passes;
    double minTetQuality, minTwist, minTriangleTwist, minFaceWeight, minVolRatio, minDeterminant;
    double maxConcave, minFlatness, minVol, minArea;
} smgpu_quality_constraint_limits_all;        /* NULL limits = {65, 4, 20, 2, -1e30, -1, -1, 0, 0, 0, 180, 0, 0, 0} */
typedef struct smgpu_quality_constraint_record_all {
    int64_t iteration;
    int32_t passes, fullRevert;
    int64_t nBadCells, nPointsReverted;
    int64_t nTangledCells, nNonOrthoFaces, nSkewFaces;
    int64_t nLowTetFaces, nLowTwistFaces, nLowTriangleTwistFaces, nLowWeightFaces, nLowVolRatioFaces, nUnderdeterminedCells;
    int64_t nConcaveFaces, nWarpedFaces, nSmallAreaFaces, nSmallVolumeCells;
} smgpu_quality_constraint_record_all;
typedef struct smgpu_quality_constraint_state_all {
    int32_t on, passes;
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int64_t nExemptCells, nExemptFaces, iteration;
    double minTetQuality, minTwist, minTriangleTwist, minFaceWeight, minVolRatio, minDeterminant;
    int64_t nExemptDeterminantCells;
    double maxConcave, minFlatness, minVol, minArea;
    int64_t nExemptVolumeCells;
} smgpu_quality_constraint_state_all;
int smgpu_set_quality_constraint_limits_all(smgpu_handle* h, const smgpu_quality_constraint_limits_all* p, int32_t on);
int smgpu_set_quality_constraint_limits_all_coupled(smgpu_handle* h, const smgpu_quality_constraint_limits_all* p,
                                                    const smgpu_quality_constraint_halo_desc_full* d, int32_t on);
int smgpu_get_quality_constraint_records_all(smgpu_handle* h, smgpu_quality_constraint_record_all* out, int64_t cap, int64_t* n);
int smgpu_get_quality_constraint_state_all(smgpu_handle* h, smgpu_quality_constraint_state_all* out);

/* ---- scaling passes: a bad cell's points keep a fraction of their move before they go back (DESIGN.md "Mesh quality", 10.19) --
 * An opt-in extension of the SERIAL quality constraint (any of its three entries).  Off (scalePasses = 0, the state after
 * every smgpu_set_quality_constraint*): every launch, record and bit is what it is without this section.
 * Notation of 10.12 / 10.14: x the points the iteration started from, L the points the loop produced, B the bad, non-exempt
 * cells by whatever criteria are on.  Verdicts, exemptions and evaluation kernels are unchanged.
 * PARAMETERS.  scalePasses S >= 0 (0: off; < 0 refused); errorReduction r (refused outside 0 <= r < 1, and NaN);
 * nSmoothScale n >= 0 (< 0 refused); passes P, the constraint's own, keeps its meaning: marked revert passes before the full
 * revert.
 * PER ITERATION THAT RAN.
 *   1. A scale s_p = 1 for every point.
 *   2. For k = 0 .. S+P: evaluate the current points.  B empty: stop.  k == S+P: the full revert, s_p = 0 for every point.
 *      Otherwise, with M the points of every face of every cell in B (10.12's marks):
 *        k < S:        s_p <- s_p * r for p in M;
 *        S <= k < S+P: s_p <- 0       for p in M;
 *      then n Jacobi sweeps over ALL points, each reading the old field and writing the new:
 *        s_p <- min(s_p, 0.5 s_p + 0.5 (sum_q s_q) / deg_p),
 *      q over the engine's pointPoints row of p in row order, the sum a left fold from 0.0, the division one correctly rounded
 *      division, no contraction; a point with an empty row keeps its value.
 *   3. The current points become, per point: L_p where s_p == 1, with the loop's own bits, untouched; x_p where s_p == 0;
 *      x_p + s_p (L_p - x_p) per component otherwise.
 *   4. Scales only fall within an iteration.  They are 1 again at the next one.
 * INVARIANT.  10.14's holds unchanged: the last fallback is still the full revert.
 * EQUIVALENCES, both bit for bit.  S = 0: the constraint without this section -- points, every record field, launches.
 * S > 0, r = 0, n = 0: the accepted points of the constraint with passes = S + P.
 * RECORDS.  smgpu_quality_constraint_record_scaled: smgpu_quality_constraint_record_all's fields at their offsets (136 bytes),
 * then nScalePasses (the marked passes with k < S that ran), nPointsScaled (points with accepted 0 < s_p < 1 and L_p != x_p)
 * and minScale (the smallest accepted s_p: 1.0 in a clean iteration, 0 after a full revert).  nPointsReverted keeps its
 * definition, read on the accepted points: accepted point == x_p and L_p != x_p (a point scaled in one pass and reverted in a
 * later one counts once, as reverted); passes counts all marked passes, scaling and reverting.  While scaling is off the three
 * new fields are 0.  smgpu_quality_constraint_state_scaled: the _all state, then the three parameters ({0, 4, 0.75} while off).
 * The older getters keep working and return their prefixes; all drain the one pending list.
 * smgpu_set_quality_constraint_scaling is valid while the serial quality constraint is on; scalePasses = 0 (or p = NULL)
 * switches scaling off and frees its memory; clearing or re-enabling the constraint switches it off too.
 * REFUSED, by name: an engine with a halo (the coupled form has no scaling); boundary point smoothing; the tangle constraint
 * (it has no scaling: the quality constraint with its three criteria off is the tangle constraint); the quality constraint
 * off; between smgpu_iter_begin and smgpu_iter_end; scalePasses + passes above 2147483647.
 * ALLOWED TOGETHER: layers, both foam variants, all thirteen limits, the trace, the guard (its refining steps replay
 * deterministically: the scale state does not outlive an iteration), SMGPU_TILES=0.
 * Memory, outside deviceBytes, held while scaling is on: 40 bytes per point (L, and two scale fields); 160 bytes per record. */
typedef struct smgpu_quality_constraint_scaling {
    int32_t scalePasses, nSmoothScale;
    double errorReduction;
} smgpu_quality_constraint_scaling;           /* NULL = {0, 4, 0.75}: off */
typedef struct smgpu_quality_constraint_record_scaled {
    int64_t iteration;
    int32_t passes, fullRevert;
    int64_t nBadCells, nPointsReverted;
    int64_t nTangledCells, nNonOrthoFaces, nSkewFaces;
    int64_t nLowTetFaces, nLowTwistFaces, nLowTriangleTwistFaces, nLowWeightFaces, nLowVolRatioFaces, nUnderdeterminedCells;
    int64_t nConcaveFaces, nWarpedFaces, nSmallAreaFaces, nSmallVolumeCells;
    int64_t nScalePasses, nPointsScaled;
    double minScale;
} smgpu_quality_constraint_record_scaled;
typedef struct smgpu_quality_constraint_state_scaled {
    int32_t on, passes;
    double maxNonOrtho, maxInternalSkewness, maxBoundarySkewness;
    int64_t nExemptCells, nExemptFaces, iteration;
    double minTetQuality, minTwist, minTriangleTwist, minFaceWeight, minVolRatio, minDeterminant;
    int64_t nExemptDeterminantCells;
    double maxConcave, minFlatness, minVol, minArea;
    int64_t nExemptVolumeCells;
    int32_t scalePasses, nSmoothScale;
    double errorReduction;
} smgpu_quality_constraint_state_scaled;
int smgpu_set_quality_constraint_scaling(smgpu_handle* h, const smgpu_quality_constraint_scaling* p);
int smgpu_get_quality_constraint_records_scaled(smgpu_handle* h, smgpu_quality_constraint_record_scaled* out, int64_t cap, int64_t* n);
int smgpu_get_quality_constraint_state_scaled(smgpu_handle* h, smgpu_quality_constraint_state_scaled* out);

/* ---- scaling passes on a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.20) ------------------------------------
 * 10.19 read on the GLOBAL mesh, for an engine whose halo is configured and whose coupled quality constraint is on (through any of
 * its three coupled entries).  Notation of 10.19 (x, L, s_p, S, P, r, n) and 10.15.  Off (the state after every
 * smgpu_set_quality_constraint*_coupled): every launch, record and bit of a decomposed run is what it is without this section.
 * WHAT CROSSES THE RANKS.
 *   1. Marks and verdict travel exactly as in 10.15; a pass runs for k = 0 .. S+P.  The host knows k: a marked pass scales
 *      (k < S), reverts (S <= k < S+P) or is the full revert (k == S+P).
 *   2. Mark -> scale.  Behind the OR of the shared points' marks every rank applies s <- s r, s <- 0, or s <- 0 for all, to its own
 *      copy of the scale field.  The combined marks and r are the same on every sharer: copies of a shared point's scale stay
 *      bit-identical (an invariant).
 *   3. The sweep s_p <- min(s_p, 0.5 s_p + 0.5 (sum_q s_q) / deg_p) runs over the neighbours of p in the WHOLE mesh.
 *      Shared points are named by (global id, component) as the halo's tables name them.  COUNTED EDGE: a row entry (p, q) of rank
 *      R is counted iff R is the lowest rank whose sub-domain holds the edge pq; an entry with an unshared end is always counted.
 *      PARTIAL SUM: part_R(p), the left fold from 0.0 in rank R's row order over the counted entries of p's row (0.0 when none is).
 *      TOTAL: the left fold from 0.0 of part_R(p) over the sharers of p in ascending rank (the order of combOffsets / combSlots,
 *      -1: this rank).  DEGREE: deg_p, the counted entries of p over all ranks, formed once by the caller.  One correctly rounded
 *      division, no contraction, Jacobi between two fields, n sweeps behind every marked pass, none behind the full revert.  An
 *      unshared point is 10.19's.  One double per send slot travels per sweep: exchange S, laid out like exchange T.
 *   4. The accepted points are 10.19's item 3 on every rank.
 * RECORDS.  smgpu_quality_constraint_record_scaled per rank and iteration: passes, fullRevert and nScalePasses are global values;
 * nPointsReverted and nPointsScaled the rank's own, a shared point counting on its master only (10.13); minScale the rank's own
 * minimum.  Combined: sums, and min for minScale.  The state carries the three parameters as in the serial form.
 * EQUIVALENCES.  S = 0: 10.15 / 10.17 / 10.18 by bits and launches.  A single sub-domain without processor patches: the serial
 * scaled run (10.19), bit for bit.  S > 0, r = 0, n = 0: the accepted points of the coupled constraint with passes = S + P.
 * Against the undecomposed mesh the row orders and the fold over the ranks differ: the serial run to rounding, not to the bit.
 * A CLEAN ITERATION (summed count 0 at k = 0) adds no launch, wait, exchange or byte to 10.15's.
 *
 * smgpu_set_quality_constraint_scaling_coupled(h, p, c): p as 10.19's (NULL or scalePasses = 0: off, frees L and the two scale
 * fields; c is then not read).  c: the caller's tables, copied during the call, and its exchange buffers, used until scaling is
 * switched off.  Clearing or re-enabling the constraint switches scaling off; smgpu_halo_configure stays refused while the
 * constraint is on.
 * THE CALLS OF A PASS while scaling is on, on every rank (a call out of order is an error):
 *   smgpu_quality_constraint_pass_begin, the move of Cc, _pass_faces, the sum of the counts: as 10.15.
 *   sum == 0:  smgpu_quality_constraint_pass_end(0) closes the record.  Nothing else is called.
 *   sum > 0:   k < S+P: the host moves sendT -> recvT.  Then
 *     smgpu_quality_constraint_pass_scale(sum)   combines the marks (k < S+P), at the iteration's first such pass keeps L and
 *                             fills s = 1, applies mark -> scale, queues the local half of sweep 0 (k < S+P and n > 0) and
 *                             returns with sendS complete.
 *     n times (k < S+P):      the host moves sendS -> recvS as exchange T; smgpu_quality_constraint_pass_sweep finishes the sweep
 *                             (the shared points' totals), queues the next one's local half and returns with sendS complete.
 *     smgpu_quality_constraint_pass_end(sum)     the accepted points, the counts; k == S+P: the record closes, *done = 1.
 *   Refused: _pass_scale when scaling is off, without _pass_faces, twice in a pass, with sum <= 0; _pass_sweep without _pass_scale
 *   or when no sweep is due; _pass_end with sum > 0 without _pass_scale, with another sum than _pass_scale got, or with sweeps due.
 * REFUSED by smgpu_set_quality_constraint_scaling_coupled, by name: scalePasses < 0, errorReduction outside 0 <= r < 1 (and NaN),
 * nSmoothScale < 0; an engine without a halo (smgpu_set_quality_constraint_scaling is its form, and keeps refusing an engine with
 * one); boundary point smoothing; the coupled tangle constraint; the coupled quality constraint off, or its exempt faces not taken;
 * between smgpu_iter_begin and smgpu_iter_end; with the passes of an iteration due; scalePasses + passes above 2147483647; a null
 * table or buffer that is needed; a table out of range.
 * Memory, outside deviceBytes, held while scaling is on: 10.19's 40 bytes per point, 20 bytes per shared point and 4 per counted
 * row entry; the caller owns sendS / recvS. */
typedef struct smgpu_quality_scale_coupling {
    const int32_t* rowOffsets;              /* nShared + 1: CSR over the shared points, in the halo's order */
    const int32_t* rowPoints;               /* the counted neighbours of each shared point: local point ids, in row order */
    const int32_t* sharedDeg;               /* nShared: the degree of each shared point in the whole mesh */
    void *sendS, *recvS;                    /* device, nSend / nRecv doubles, moved by the caller like sendT / recvT */
} smgpu_quality_scale_coupling;
int smgpu_set_quality_constraint_scaling_coupled(smgpu_handle* h, const smgpu_quality_constraint_scaling* p, const smgpu_quality_scale_coupling* c);
int smgpu_quality_constraint_pass_scale(smgpu_handle* h, int64_t nBadGlobal);               /* after smgpu_quality_constraint_pass_faces */
int smgpu_quality_constraint_pass_sweep(smgpu_handle* h);

/* ---- the constraints and the guard with boundary point smoothing (DESIGN.md "Mesh quality", 10.21) ---------------------------
 * smgpu_set_boundary_revert(h, 1) is the opt-in under which smgpu_set_tangle_constraint, smgpu_set_quality_constraint, _limits,
 * _limits_all (all thirteen limits) and smgpu_set_quality_guard accept a serial engine with boundary point smoothing
 * (smgpu_set_boundary_smoothing), with or without layers.  Default 0: every refusal of 10.11, 10.12 and 10.14 stands as it was.
 * The switch launches nothing and allocates nothing: with it on and nothing armed the loop is the loop without it.
 *
 * THE CONTRACT.  10.12 and 10.14 hold unchanged with these additions:
 *   - x' is the loop's result INCLUDING everything boundary point smoothing does: the projection to corners, feature edges and
 *     the target surface, the prismatic projection, the step clamp and the restore.  A boundary point is a point like any other:
 *     marked by a bad cell it goes back to x_p bitwise, off the place the projection gave it.
 *   - THE POINT NORMALS ARE LOOP STATE, NOT POINT STATE.  They are blended once at the start of every iteration that runs, from
 *     the normals as they are and the boundary faces at the points that iteration starts from.  A marked pass or a full revert
 *     never puts them back: the next iteration blends from the current normals and the faces at the ACCEPTED points.
 *   - The sharp-edge flags, the feature edge projections and the inner-neighbour coordinates are recomputed by every iteration
 *     from the points it starts from; the corner and feature lists are fixed at set-up.  They need nothing.
 *   - The guard goes back across iterations, so its snapshot and its restore carry the point normals whenever boundary point
 *     smoothing (or layers) is on: a restored run replays the iterations bit for bit.
 *   - residual and nFrozenPoints stay the loop's own, as in 10.12.
 * Refused: an engine with a halo (the coupled entries keep refusing boundary point smoothing); on -> off while a constraint is on
 * or the guard armed over boundary point smoothing.  Unchanged: smgpu_set_boundary_smoothing stays refused while a constraint is
 * on or the guard armed (the exempt bytes and the snapshot are sized and evaluated at enabling); the scaling passes (10.19) stay
 * refused with boundary point smoothing -- a scaled boundary point leaves the target surface. */
int smgpu_set_boundary_revert(smgpu_handle* h, int32_t on);   /* default 0 */
int smgpu_get_boundary_revert(smgpu_handle* h, int32_t* on);

/* ---- the same report for a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.4) -----------------------------
 * Step-wise; the host moves the buffers between the calls, with or without a halo (not between smgpu_iter_begin and _end):
 *   1. smgpu_quality_coupled_pack: the geometry of the current points (the loop's own launch, uncounted), then the owner cell
 *      centre of every processor face, patch by patch in `c`'s order, 3 doubles per face, into the DEVICE buffer sendCc.
 *      Returns once sendCc is written.  Face i of patch r->o pairs with face i of patch o->r (decomposePar's convention).
 *   2. the host fills recvCc (device, same layout as sendCc): for each patch r->o, the neighbour o's sendCc of its patch o->r.
 *   3. smgpu_quality_coupled_report / _field on the geometry of step 1 (refused when the points may have moved since: a pack
 *      must follow smgpu_iterate, smgpu_iter_begin, smgpu_set_points, smgpu_set_foam_variant).
 * A processor face takes the internal-face definitions with C_N from recvCc.  The record counts it only on the side with
 * myRank < neighbRank, there as an internal face; fields carry its non-orthogonality and skewness on both sides.  Ids in the
 * record are local; combine the records of all ranks as DESIGN.md 10.4 says (smoothmesh_amd/quality.py combine_quality).
 * Refused: two patches to the same neighbour, a patch to myRank, patches outside the boundary faces or overlapping. */
typedef struct smgpu_quality_coupling {
    int32_t myRank, nPatches;          /* processor patches of this sub-domain, boundary-file order              */
    const int32_t* patchStart;         /* [nPatches] first face                                                   */
    const int32_t* patchSize;          /* [nPatches]                                                              */
    const int32_t* neighbRank;         /* [nPatches]                                                              */
} smgpu_quality_coupling;
/* smgpu_quality with sumNonOrth (Σθ over the counted internal faces) in place of the average; nFaces / nInternalFaces after
 * the counted-once rule; ids local (-1 where this rank has no such element). */
typedef struct smgpu_quality_part {
    int64_t nCells, nFaces, nInternalFaces;
    double minVolume, maxVolume, totalVolume;  int64_t nNonPositiveVolume;  int32_t minVolumeCell;
    double minFaceArea, maxFaceArea;           int64_t nZeroAreaFaces;
    double maxNonOrth, sumNonOrth;             int64_t nSevereNonOrth, nErrorNonOrth;  int32_t maxNonOrthFace;
    double maxSkewness;                        int64_t nSkewFaces;  int32_t maxSkewFace;
    int64_t nWrongOrientedFaces;
    double maxOpenness;                        int64_t nOpenCells;
    double maxAspectRatio;                     int64_t nHighAspectCells;
} smgpu_quality_part;
/* *nProcFaces (may be NULL) = the number of processor faces, i.e. sendCc / recvCc hold 3 * *nProcFaces doubles.  sendCc may be
 * NULL only when that number is 0. */
int smgpu_quality_coupled_pack(smgpu_handle* h, const smgpu_quality_coupling* c, void* sendCc, int64_t* nProcFaces);
int smgpu_quality_coupled_report(smgpu_handle* h, const smgpu_quality_params* p, const void* recvCc, smgpu_quality_part* out);
/* names and sizes as smgpu_quality_field */
int smgpu_quality_coupled_field(smgpu_handle* h, const char* name, const void* recvCc, double* out, int64_t* n);

/* ---- the failing elements of the report as sets (DESIGN.md "Mesh quality", 10.5) ---------------------------------------
 * names and order: DESIGN.md 10.5 (nonOrthoFaces, skewFaces, wrongOrientedFaces, zeroAreaFaces, zeroVolumeCells,
 * nonClosedCells, highAspectRatioCells).  counts[7] always filled; each equals the report's count under the same p.
 * ids: the seven sets concatenated in that order, each ascending, written when ids != NULL and cap >= sum(counts); ids != NULL
 * with a smaller cap is an error (counts still filled).  ids == NULL: counts only.  Refusals, side effects and state as
 * smgpu_mesh_quality (serial, refused on a halo engine) and smgpu_quality_coupled_report (a sub-domain, on the geometry of the
 * last pack; a processor face is a member only on the side that counts it).  Ids are local. */
int smgpu_quality_sets(smgpu_handle* h, const smgpu_quality_params* p, int64_t counts[7], int32_t* ids, int64_t cap);
int smgpu_quality_coupled_sets(smgpu_handle* h, const smgpu_quality_params* p, const void* recvCc,
                               int64_t counts[7], int32_t* ids, int64_t cap);

/* ---- the checks `checkMesh -allGeometry` adds (DESIGN.md "Mesh quality", 10.6) ------------------------------------------
 * Face concavity (the sine of the worst concave corner and its angle in degrees), face flatness, face interpolation weight,
 * owner / neighbour volume ratio (internal faces) and cell determinant, of the current points, on the same inputs as
 * smgpu_mesh_quality.  Refusals, side effects and state as smgpu_mesh_quality (refused on an engine with a halo; needs no
 * smgpu_set_params).  Ties go to the lowest id, sums are reduced in a fixed order.  An id is -1 where no element qualifies (no
 * concave face, no face with more than 3 vertices, no internal face, no cell); the minima and averages are then 1 (determinant:
 * 0) and the concavity figures 0.
 * p == NULL: the defaults 10 degrees, 0.8, 0.05, 0.01, 0.001. */
typedef struct smgpu_quality_geometry_params {
    double concaveThreshold, flatnessThreshold, weightThreshold, volRatioThreshold, determinantThreshold;
} smgpu_quality_geometry_params;
typedef struct smgpu_quality_geometry {
    int64_t nConcaveFaces;  double maxConcaveSin, maxConcaveAngle;  int32_t maxConcaveFace;
    double minFlatness, avgFlatness;        int64_t nFlatnessFaces, nWarpedFaces;  int32_t minFlatnessFace;
    double minFaceWeight, avgFaceWeight;    int64_t nLowWeightFaces;               int32_t minFaceWeightFace;
    double minVolRatio, avgVolRatio;        int64_t nLowVolRatioFaces;             int32_t minVolRatioFace;
    double minDeterminant, avgDeterminant;  int64_t nUnderdeterminedCells;         int32_t minDeterminantCell;
} smgpu_quality_geometry;
int smgpu_mesh_quality_geometry(smgpu_handle* h, const smgpu_quality_geometry_params* p, smgpu_quality_geometry* out);
/* per-element field in polyMesh order: "faceConcavity" (the sine, under the default concaveThreshold; 0 where no corner is
 * concave), "faceFlatness" (1 on triangles), "faceWeight", "faceVolumeRatio" (1 on boundary faces) [nFaces], "cellDeterminant"
 * [nCells].  out == NULL: size only (*n). */
int smgpu_quality_geometry_field(smgpu_handle* h, const char* name, double* out, int64_t* n);

/* ---- the motion criteria: what checkMesh -meshQuality / snappyHexMesh test beyond the two reports above (DESIGN.md "Mesh
 * quality", 10.7) --------------------------------------------------------------------------------------------------------
 * Per face, of the current points, on the same inputs as smgpu_mesh_quality: the worst tet of the face-centre decomposition
 * (minTetQuality), the best base point's worst tet of the base-point decomposition particle tracking uses (a face with none
 * at or above tetThreshold has no valid base point), face twist and triangle twist (faces with more than 3 vertices).  A tet
 * quality is the signed volume over that of the regular tetrahedron with the same circumradius: 1 at best, negative when
 * inverted.  Refusals, side effects and state as smgpu_mesh_quality (refused on an engine with a halo; needs no
 * smgpu_set_params).  Ties go to the lowest id, sums are reduced in a fixed order.  Where no face qualifies (no face; no face
 * with more than 3 vertices) the minima and averages are 1 and the id is -1.
 * p == NULL: the defaults 1e-15, 0.02, -1 (triangle twist off), as in the default meshQualityDict. */
typedef struct smgpu_quality_motion_params {
    double tetThreshold, twistThreshold, triangleTwistThreshold;
} smgpu_quality_motion_params;
typedef struct smgpu_quality_motion {
    double minTetQuality, avgTetQuality;        int64_t nLowTetFaces;                 int32_t minTetFace;
    double minBaseTetQuality;                   int64_t nNoBasePointFaces;            int32_t minBaseTetFace;
    double minTwist, avgTwist;                  int64_t nTwistFaces, nLowTwistFaces;  int32_t minTwistFace;
    double minTriangleTwist, avgTriangleTwist;  int64_t nLowTriangleTwistFaces;       int32_t minTriangleTwistFace;
} smgpu_quality_motion;
int smgpu_mesh_quality_motion(smgpu_handle* h, const smgpu_quality_motion_params* p, smgpu_quality_motion* out);
/* per-face field in polyMesh order [nFaces]: "faceTetQuality", "faceBaseTetQuality", "faceTwist", "faceTriangleTwist" (1 on
 * triangles).  out == NULL: size only (*n). */
int smgpu_quality_motion_field(smgpu_handle* h, const char* name, double* out, int64_t* n);

/* ---- the two reports above for a sub-domain of a decomposed mesh (DESIGN.md "Mesh quality", 10.8) -------------------------
 * The steps of smgpu_quality_coupled_pack / _report, with one more buffer for the geometry report:
 *   1. smgpu_quality_coupled_pack, then smgpu_quality_coupled_pack_volumes on the same points: the signed volume of every cell
 *      (formula and summation order of smgpu_mesh_quality_geometry) into the engine's scratch, and the owner cell's volume of
 *      every processor face into the DEVICE buffer sendVc: 1 double per face, the slot order of sendCc.
 *   2. the host fills recvCc as before and recvVc (device, same layout as sendVc) the same way.
 *   3. smgpu_quality_coupled_geometry_report / _field (recvCc and recvVc) and smgpu_quality_coupled_motion_report / _field (recvCc
 *      only; needs no pack_volumes), on the geometry of step 1.
 * A processor face takes the internal-face branch of every criterion (weight, volume ratio, both tet decompositions, twist) with
 * C_N and V_N of the neighbour rank, and a cell's determinant runs over its internal and its processor faces.  The records count a
 * processor face only on the side with myRank < neighbRank; fields carry its values on both sides.  Refusals, state and side
 * effects as smgpu_quality_coupled_report; the geometry calls are also refused when no pack_volumes followed the pack.  Field
 * names as smgpu_quality_geometry_field / smgpu_quality_motion_field.
 * The records are the serial structs with every average replaced by its sum, behind the denominators the combine needs (after the
 * counted-once rule); ids local, -1 where this rank has no such element; maxConcaveAngle is this rank's own (the combine takes the
 * winner's pair).  Combine them as DESIGN.md 10.8 says (smoothmesh_amd/quality.py combine_quality_geometry / _motion). */
typedef struct smgpu_quality_geometry_part {
    int64_t nCells, nFaces, nInternalFaces;
    int64_t nConcaveFaces;  double maxConcaveSin, maxConcaveAngle;  int32_t maxConcaveFace;
    double minFlatness, sumFlatness;        int64_t nFlatnessFaces, nWarpedFaces;  int32_t minFlatnessFace;
    double minFaceWeight, sumFaceWeight;    int64_t nLowWeightFaces;               int32_t minFaceWeightFace;
    double minVolRatio, sumVolRatio;        int64_t nLowVolRatioFaces;             int32_t minVolRatioFace;
    double minDeterminant, sumDeterminant;  int64_t nUnderdeterminedCells;         int32_t minDeterminantCell;
} smgpu_quality_geometry_part;
typedef struct smgpu_quality_motion_part {
    int64_t nFaces;
    double minTetQuality, sumTetQuality;        int64_t nLowTetFaces;                 int32_t minTetFace;
    double minBaseTetQuality;                   int64_t nNoBasePointFaces;            int32_t minBaseTetFace;
    double minTwist, sumTwist;                  int64_t nTwistFaces, nLowTwistFaces;  int32_t minTwistFace;
    double minTriangleTwist, sumTriangleTwist;  int64_t nLowTriangleTwistFaces;       int32_t minTriangleTwistFace;
} smgpu_quality_motion_part;
/* *nProcFaces (may be NULL) = the number of processor faces = the doubles of sendVc, which may be NULL only when that is 0 */
int smgpu_quality_coupled_pack_volumes(smgpu_handle* h, void* sendVc, int64_t* nProcFaces);
int smgpu_quality_coupled_geometry_report(smgpu_handle* h, const smgpu_quality_geometry_params* p, const void* recvCc, const void* recvVc,
                                          smgpu_quality_geometry_part* out);
int smgpu_quality_coupled_geometry_field(smgpu_handle* h, const char* name, const void* recvCc, const void* recvVc, double* out, int64_t* n);
int smgpu_quality_coupled_motion_report(smgpu_handle* h, const smgpu_quality_motion_params* p, const void* recvCc,
                                        smgpu_quality_motion_part* out);
int smgpu_quality_coupled_motion_field(smgpu_handle* h, const char* name, const void* recvCc, double* out, int64_t* n);

/* ---- the findings of the two reports above as sets (DESIGN.md "Mesh quality", 10.9) --------------------------------------
 * Geometry, counts[5]: concaveFaces, warpedFaces, lowWeightFaces, lowVolRatioFaces (face sets), underdeterminedCells (cell
 * set); sizes nConcaveFaces, nWarpedFaces, nLowWeightFaces, nLowVolRatioFaces, nUnderdeterminedCells of the report under the same
 * p.  Motion, counts[4]: lowQualityTetFaces, noBasePointFaces, twistedFaces, lowTriangleTwistFaces (face sets); sizes nLowTetFaces,
 * nNoBasePointFaces, nLowTwistFaces, nLowTriangleTwistFaces.  Membership is read off the record the report's per-element body
 * fills, so the sizes are identities.  counts, ids and cap exactly as smgpu_quality_sets: counts always filled; the sets
 * concatenated in that order, each ascending, into ids when ids != NULL and cap >= sum(counts); a smaller cap is an error (counts
 * still filled, ids untouched); ids == NULL: counts only.  Ids are local and bitwise repeatable.
 * Refusals, side effects and state as the matching report: smgpu_mesh_quality_geometry / _motion (serial, refused on a halo
 * engine) and smgpu_quality_coupled_geometry_report / _motion_report (a sub-domain, on the geometry of the last pack, the geometry
 * call after pack_volumes; a processor face is a member only on the side with myRank < neighbRank).  The seven-set calls above
 * are unchanged. */
int smgpu_quality_geometry_sets(smgpu_handle* h, const smgpu_quality_geometry_params* p, int64_t counts[5], int32_t* ids, int64_t cap);
int smgpu_quality_motion_sets(smgpu_handle* h, const smgpu_quality_motion_params* p, int64_t counts[4], int32_t* ids, int64_t cap);
int smgpu_quality_coupled_geometry_sets(smgpu_handle* h, const smgpu_quality_geometry_params* p, const void* recvCc, const void* recvVc,
                                        int64_t counts[5], int32_t* ids, int64_t cap);
int smgpu_quality_coupled_motion_sets(smgpu_handle* h, const smgpu_quality_motion_params* p, const void* recvCc,
                                      int64_t counts[4], int32_t* ids, int64_t cap);

/* Timing: when enabled every kernel launch is bracketed by hipEvents on the handle's stream. */
int smgpu_enable_timing(smgpu_handle* h, int32_t on);
int smgpu_get_counters(smgpu_handle* h, smgpu_counters* out);
int smgpu_reset_counters(smgpu_handle* h);

/* ---- multi-rank (domain decomposition, one handle per rank/GPU) --------------------------
 * Replaces syncTools::syncPointList at SM.C:134,142,402,429,455,472 (one fused exchange "A")
 * and SM.C:2374 (exchange "F").  The library packs/unpacks; the host moves the buffers
 * (RCCL all_to_all over xGMI) between the calls.  All buffers are DEVICE pointers owned by the
 * caller.  Record of exchange A = 13 doubles per slot {sum xyz, r1 xyz, r2 xyz, r3 xyz,
 * (int32 count, int32 hasCommonCell)}; record of exchange F = 1 int32 per slot. */
#define SMGPU_HALO_A_DOUBLES 13
typedef struct smgpu_halo_desc {
    int32_t nShared;              /* points of this rank shared with >= 1 other rank          */
    const int32_t* sharedLocal;   /* [nShared] local point ids                                */
    int32_t nSend;                /* send slots (concatenated by destination rank, ascending) */
    const int32_t* sendShared;    /* [nSend]   index into sharedLocal of each send slot       */
    int32_t nRecv;                /* recv slots (concatenated by source rank, ascending)      */
    const int32_t* combOffsets;   /* [nShared+1] CSR over sharers of each shared point        */
    const int32_t* combSlots;     /* recv slot of each sharer, ascending rank; -1 = this rank */
    void* sendA; void* recvA;     /* device, nSend / nRecv records of 13 doubles              */
    void* sendF; void* recvF;     /* device, nSend / nRecv int32                              */
    void* localStats;             /* device, 2 doubles {residual, nFrozenPoints} per iteration */
    void* sendL; void* recvL;     /* device, nSend / nRecv records sized for SMGPU_HALO_L_DOUBLES doubles; only used with the
                                     boundary layer treatment / boundary point smoothing (may be NULL otherwise),
                                     exchanged together with sendA / recvA (smgpu_halo_l_doubles per slot in use)  */
    int32_t useExchangeStream;    /* 0: the host enqueues its exchanges on the engine's stream (in order).       */
    void* exchangeStream;         /* 1: the host enqueues them on THIS hipStream_t (NULL = the null stream); the
                                     engine orders its own stream against it with events inside
                                     smgpu_iter_begin/mid/end, so the exchange runs next to the kernels of
                                     smgpu_iter_interior / smgpu_iter_ahead and the compute queue does not idle */
} smgpu_halo_desc;
int smgpu_halo_configure(smgpu_handle* h, const smgpu_halo_desc* d);
/* ---- peer-store transport: the ranks of one node move the shared-point records THEMSELVES -------------------------------
 * Instead of the host enqueuing an exchange between smgpu_iter_begin / mid / end (MPI, RCCL send / recv groups), the kernels
 * that pack exchange A / L / F store every record straight into the peer's receive slot over xGMI (the peers' receive
 * buffers are mapped into this process: hipIpc) and raise a flag word at the peer; the first kernel that consumes the records
 * waits for its peers' flags.  pack = send, no collective kernel, no host call.  The host
 *   1. allocates recvA / recvL / recvF and one flag array (uint32[2 * 64], zero) with smgpu_push_alloc and passes the
 *      receive buffers to smgpu_halo_configure as usual (useExchangeStream = 0);
 *   2. hands the 64-byte handles to its peers (any channel) and maps theirs with smgpu_push_open;
 *   3. calls smgpu_halo_set_push on every rank, then iterates WITHOUT moving anything between the smgpu_iter_* calls.
 * peers = the ranks this rank shares points with, ascending (the order of the send slot groups); remoteBase[o] = first slot,
 * in peer o's receive numbering, of this rank's records; myIndexAtPeer[o] = this rank's position among peer o's peers.
 * All ranks must use the same transport.  A record that does not arrive within two seconds raises an error at the next
 * host read-back (smgpu_last_error).  d = NULL switches back to host-driven exchanges. */
typedef struct smgpu_push_desc {
    int32_t nPeers;
    const int32_t* peerCount;       /* [nPeers] slots per peer (sum = nSend)                              */
    const int32_t* remoteBase;      /* [nPeers]                                                           */
    const int32_t* myIndexAtPeer;   /* [nPeers]                                                           */
    void* const* peerRecvA;         /* [nPeers] the peers' buffers, mapped                                */
    void* const* peerRecvL;         /* [nPeers] (entries may be NULL while neither layers nor boundary smoothing is on) */
    void* const* peerRecvF;         /* [nPeers]                                                           */
    void* const* peerFlags;         /* [nPeers] the peers' flag arrays, mapped                            */
    void* localFlags;               /* this rank's flag array                                             */
} smgpu_push_desc;
int smgpu_halo_set_push(smgpu_handle* h, const smgpu_push_desc* d);
int smgpu_push_alloc(int32_t device, size_t bytes, void** ptr, void* ipcHandle64);   /* uncached device memory + its IPC handle */
int smgpu_push_open(int32_t device, const void* ipcHandle64, void** ptr);            /* map a peer's allocation               */
int smgpu_push_close(void* ptr);
int smgpu_push_free(void* ptr);

/* change useExchangeStream / exchangeStream of a configured halo (e.g. to time both arrangements on the target) */
int smgpu_halo_set_exchange_stream(smgpu_handle* h, int32_t useExchangeStream, void* exchangeStream);
/* the hipStream_t the engine launches on (its own, or the caller's when useCallerStream was set) */
int smgpu_get_stream(smgpu_handle* h, void** stream);
/* optional: smgpu_iter_end additionally writes the iteration's {residual, nFrozenPoints} to record (n mod capacity) of
 * this device array of 2*capacity doubles, n = number of smgpu_iter_end calls since this call -- a run that cannot
 * stop early (relTol <= 0) then needs no per-iteration host action on localStats.  history = NULL switches it off. */
int smgpu_halo_set_stats_history(smgpu_handle* h, void* history, int32_t capacity);
int smgpu_iter_begin(smgpu_handle* h);   /* geometry + local partial sums / closest points -> sendA */
int smgpu_iter_interior(smgpu_handle* h);/* optional, between begin and mid: everything that does not need
                                            recvA (points away from the shared ones) -- lets the host overlap
                                            exchange A with compute                                         */
int smgpu_iter_mid(smgpu_handle* h);     /* combine recvA, proposal, constraints -> sendF           */
int smgpu_iter_ahead(smgpu_handle* h);   /* optional, between mid and end: next iteration's geometry away from
                                            the shared points -- overlaps exchange F (constraints off)      */
int smgpu_iter_end(smgpu_handle* h);     /* or recvF, restore, residual -> localStats; movePoints   */

/* ---- optional boundary layer treatment (prismatic layers on selected patches) -------------------------------
 * Replaces SM.C:2186-2221 (set-up: point classification BPS.C:296-340,397-403; calculatePointHopsToBoundary,
 * calculateBoundaryPointNormals, propagateOuterNeighInfo, OBB.C = src/orthogonalBoundaryBlending.C) and, inside
 * every later iteration, SM.C:2266 + 2283-2305 (updateNeighCoords, blendWithOrthogonalPoints, second step clamp).
 * Patches as in polyMesh/boundary: face ranges in file order.  Call after smgpu_create (the set-up uses the
 * coordinates the engine holds) and before iterating.  With a halo (smgpu_halo_configure) use the step-wise form below.
 * *enabled = the reference's doLayerTreatment (a layer patch is selected and layerMaxBlendingFraction > SMALL). */
typedef struct smgpu_layer_desc {
    int32_t nPatches;
    const int32_t* patchStart;     /* [nPatches] first face                                    */
    const int32_t* patchSize;      /* [nPatches] number of faces                               */
    const uint8_t* patchKind;      /* [nPatches] 0 ordinary, 1 processor, 2 empty (OBB.C:156-159) */
    const uint8_t* isLayerPatch;   /* [nPatches] selected by -layerPatches (SM.C:1823)          */
    double layerMaxBlendingFraction;   /* SM.C:1892, default 0.3                                */
    double layerEdgeLength;            /* SM.C:1895, default minEdgeLength                      */
    double layerExpansionRatio;        /* SM.C:1898, default 1.3                                */
    int32_t minLayers, maxLayers;      /* SM.C:1901-1905, defaults 1 and 4                      */
} smgpu_layer_desc;
int smgpu_set_layers(smgpu_handle* h, const smgpu_layer_desc* d, int32_t* enabled);

/* The same set-up in steps, for runs with a halo (-parallel): between the steps the host performs the reference's
 * syncTools::syncPointList calls over the shared points (values in the order of smgpu_halo_desc.sharedLocal, exchanged
 * and combined by the host like exchange A).  Sequence (SM.C:2215-2221):
 *   smgpu_layers_begin                                         -> *maxIter = maxLayers + 1
 *   maxIter x { step HOPS_SWEEP;  get HOPS, combine with max over the sharers (OBB.C:124-130), set HOPS }
 *   step NORMALS_ACCUMULATE;  get NORMALS_COUNT, sum over the sharers in ascending rank order (OBB.C:184-198), set
 *   step NORMALS_FINISH
 *   for iter = 1..maxIter { step PROPAGATE_SWEEP(iter);  get NORMALS, every sharer folds the others' values onto its own
 *                           in ascending rank order keeping the larger magnitude, ties keep (OBB.C:359-365), set }
 *   step FINISH
 * Every later iteration additionally exchanges 6 doubles per shared point (smgpu_halo_desc.sendL / recvL: the local
 * normal and the outer neighbour's coordinates; plusEq OBB.C:184-198 and minMagSqr OBB.C:490-496) next to exchange A. */
enum { SMGPU_LAYERS_HOPS_SWEEP = 0, SMGPU_LAYERS_NORMALS_ACCUMULATE = 1, SMGPU_LAYERS_NORMALS_FINISH = 2,
       SMGPU_LAYERS_PROPAGATE_SWEEP = 3, SMGPU_LAYERS_FINISH = 4 };
enum { SMGPU_LAYERS_F_HOPS = 0,            /* 1 double per shared point (the hop count or -1)        */
       SMGPU_LAYERS_F_NORMALS_COUNT = 1,   /* 4 doubles: normal, number of boundary faces            */
       SMGPU_LAYERS_F_NORMALS = 2 };       /* 3 doubles: normal                                      */
/* One record per shared point: [0:3] local normal, [3:6] outer neighbour coordinates (layers), [6] local number of boundary
 * faces, [7:10] inner neighbour coordinates, [10:13] local feature edge projection sum, [13] its count (boundary point
 * smoothing; zero / UNDEF when that is off).  Exchanged whenever the layer treatment or the boundary point smoothing is on. */
#define SMGPU_HALO_L_DOUBLES 14
/* The record in use is shorter while only the layer treatment needs it: the first SMGPU_HALO_L_LAYERS doubles, records packed
 * back to back from the start of sendL / recvL (which are sized for SMGPU_HALO_L_DOUBLES per slot).  smgpu_halo_l_doubles tells
 * the host how many doubles per slot to exchange; it changes when the boundary point smoothing is set up. */
#define SMGPU_HALO_L_LAYERS 6
int smgpu_halo_l_doubles(smgpu_handle* h, int32_t* doublesPerSlot);
int smgpu_layers_begin(smgpu_handle* h, const smgpu_layer_desc* d, int32_t* enabled, int32_t* maxIter);
int smgpu_layers_step(smgpu_handle* h, int32_t step, int32_t arg);
int smgpu_layers_shared(smgpu_handle* h, int32_t field, int32_t set, double* values);

/* ---- optional boundary point smoothing (projection of boundary points to feature edges and target surfaces) --------
 * Replaces, for this feature, the set-up SM.C:2080-2253 (edge mesh sanity checks BPS.C:20-79, target edge strings
 * BPS.C:446-587, classifyBoundaryPoints BPS.C:269-441, hop counts to the smoothing patches OBB.C:52-133, inner neighbour
 * map OBB.C:396-459, target strings of the feature edge points SM.C:2234-2249) and, inside every later iteration,
 * SM.C:2266 (calculateBoundaryPointNormals OBB.C:141-233), centroidalSmoothing of the boundary points too (SM.C:116),
 * SM.C:2307-2357 (projectBoundaryPointsToEdgesAndSurfaces BPS.C:843-945, projectPrismaticInternalPointsToSurfaces
 * OBB.C:573-631, third step clamp)  (BPS.C = src/boundaryPointSmoothing.C, OBB.C = src/orthogonalBoundaryBlending.C).
 * Inputs are the contents of constant/geometry/{initEdges,targetEdges,targetSurfaces}.obj (SM.C:1924-1926) as flat
 * arrays and, optionally, the isCornerPoint / isFeatureEdgePoint lists a previous run wrote (SM.C:2039-2077).
 * OpenFOAM's octree line query is replaced by a bounding volume hierarchy; semantics in csrc/kernels_boundary.hpp.
 * Call after smgpu_create and, when both are used, after smgpu_set_layers; before iterating.  With a halo use the
 * step-wise form below.
 * info->enabled = the reference's doBoundarySmoothing (SM.C:2080-2093). */
typedef struct smgpu_boundary_desc {
    int32_t nPatches;
    const int32_t* patchStart;         /* [nPatches] first face                                              */
    const int32_t* patchSize;          /* [nPatches] number of faces                                         */
    const uint8_t* patchKind;          /* [nPatches] 0 ordinary, 1 processor, 2 empty                        */
    const uint8_t* isSmoothingPatch;   /* [nPatches] selected by -smoothingPatches (default all, SM.C:1837)  */
    int32_t nInitEdgePoints;   const double* initEdgePoints;     /* [3 n] initEdges.obj                      */
    int32_t nInitEdges;        const int32_t* initEdges;         /* [2 n]                                    */
    int32_t nTargetEdgePoints; const double* targetEdgePoints;   /* targetEdges.obj; 0 edges = use initEdges */
    int32_t nTargetEdges;      const int32_t* targetEdges;
    int32_t nSurfacePoints;    const double* surfacePoints;      /* [3 n] targetSurfaces.obj                 */
    int32_t nSurfaceTriangles; const int32_t* surfaceTriangles;  /* [3 n]                                    */
    const int32_t* isCornerPointIO;        /* [nPoints] or NULL                                              */
    const int32_t* isFeatureEdgePointIO;   /* [nPoints] or NULL                                              */
    double distanceTolerance;                  /* SM.C:1921: REL_TOL * min(mesh min edge length, layerEdgeLength) */
    double internalSmoothingBlendingFraction;  /* SM.C:1907, default 0                                       */
} smgpu_boundary_desc;
typedef struct smgpu_boundary_info {
    int32_t enabled;
    int32_t nCornerPoints, nFeatureEdgePoints, nSmoothingSurfacePoints, nFrozenSurfacePoints;   /* BPS.C:423-438 */
    int32_t nTargetEdgeStrings;                                                                /* SM.C:2171      */
} smgpu_boundary_info;
int smgpu_set_boundary_smoothing(smgpu_handle* h, const smgpu_boundary_desc* d, smgpu_boundary_info* info);
/* The same set-up in steps, for runs with a halo (-parallel; configure the halo and, if used, the layers first).  The host
 * performs the reference's reductions and syncTools::syncPointList calls between the steps (SM.C:1528-1538, 2218-2219):
 *   smgpu_boundary_stats on every rank; minimum of the edge lengths, bounding box over the ranks,
 *                                       perimeter = (max x - min x) + (max y - min y) + (max z + min z)   [SM.C:1538 as written]
 *   smgpu_boundary_begin(reduced values) on every rank
 *   2 x { step HOPS_SWEEP;  get F_HOPS, combine with max over the sharers (OBB.C:124-130), set F_HOPS }
 *   step TABLES
 *   step NORMALS_ACCUMULATE;  get F_NORMALS_COUNT, sum over the sharers in ascending rank order (OBB.C:184-198), set;
 *   step NORMALS_FINISH                      (both are no-ops when the layer set-up has produced the normals already)
 * Every later iteration the boundary point smoothing fields travel in the sendL / recvL records (SMGPU_HALO_L_DOUBLES). */
enum { SMGPU_BOUNDARY_HOPS_SWEEP = 0, SMGPU_BOUNDARY_TABLES = 1, SMGPU_BOUNDARY_NORMALS_ACCUMULATE = 2, SMGPU_BOUNDARY_NORMALS_FINISH = 3 };
enum { SMGPU_BOUNDARY_F_HOPS = 0,            /* 1 double per shared point (the hop count or -1)         */
       SMGPU_BOUNDARY_F_NORMALS_COUNT = 1 }; /* 4 doubles: local normal sum, local number of boundary faces */
int smgpu_boundary_stats(smgpu_handle* h, double* minEdgeLength, double* boundingBox /* [6]: min x, max x, min y, ... */);
int smgpu_boundary_begin(smgpu_handle* h, const smgpu_boundary_desc* d, double minEdgeLengthGlobal, double perimeterGlobal,
                         smgpu_boundary_info* info);
int smgpu_boundary_step(smgpu_handle* h, int32_t step);
int smgpu_boundary_shared(smgpu_handle* h, int32_t field, int32_t set, double* values);
/* the classification to persist as <time>/isCornerPoint and <time>/isFeatureEdgePoint (labelIOLists, SM.C:2039-2064) */
int smgpu_get_boundary_classification(smgpu_handle* h, int32_t* isCornerPoint, int32_t* isFeatureEdgePoint);
/* parity access, host only: the string index of every edge of an edge mesh (findEdgeMeshStrings BPS.C:557-587) */
int smgpu_debug_edge_strings(int32_t nPoints, int32_t nEdges, const int32_t* edges, int32_t* strings, int32_t* nStrings);
/* parity access: nearest intersections of n segments (6 doubles each: start, end) with the target surface */
int smgpu_debug_find_line(smgpu_handle* h, int32_t n, const double* segments, double* hitPoints, int32_t* hit);

/* nEngines engines compute on this handle's device at the same time (ranks sharing a GPU in a debugging run, the sub-domains of
 * one process): the persistent launch of the face-angle walk replay, whose workgroups all have to be resident at once, takes
 * 1/nEngines of its default size.  No reference counterpart (the reference runs one MPI rank per core).  Results do not
 * depend on it. */
int smgpu_set_device_share(smgpu_handle* h, int32_t nEngines);

/* The replay form of the face-angle freeze walk (SM.C:1347-1434) in use: -1 not decided yet, 0 one wave over the flag array
 * (few points outside the good angle range), 1 host replay (SMGPU_WALK=host), 2 compaction + causal fixed point (many); and how
 * often the automatic choice has changed since smgpu_set_params -- it follows the number of points outside the good range as
 * the run goes (results never depend on it); *lastCount = that number for the last iteration the GPU has closed (-1: none). */
int smgpu_debug_walk_mode(smgpu_handle* h, int32_t* mode, int32_t* switches, int32_t* lastCount);
/* how the LAST smgpu_iter_begin / mid / end went out (multi-rank): multiRole = geometry + pack and combine + smoothing + packF as
 * the two multi-role launches on tiles of the shared points (constraints off; 0 = one kernel per step), flagged = the host's
 * exchanges on the exchange stream ordered by flag words next to those launches, fixInside = k_shared_fix's work as a role of
 * the smoothing launch (peer-store transport) */
/* FNV-1a checksums of every array of the addressing in a fixed order (SMGPU_TOPO_CHECKSUMS words; [0] = sizes and maxima): the
 * engine's (built on the device where the mesh allows, csrc/topology_dev.hip) against smgpu_topology_checksums of the host build */
#define SMGPU_TOPO_CHECKSUMS 64
int smgpu_debug_addressing_checksums(smgpu_handle* h, uint64_t* out /* [SMGPU_TOPO_CHECKSUMS] */);
/* the same for the geometry tile tables as the kernels read them (device build, csrc/tiles_dev.hip, against SMGPU_DEVICE_TILES=0) */
int smgpu_debug_tile_checksums(smgpu_handle* h, uint64_t* out /* [SMGPU_TOPO_CHECKSUMS] */);
int smgpu_debug_halo_mode(smgpu_handle* h, int32_t* multiRole, int32_t* flagged, int32_t* fixInside);
/* the tile counts the multi-role launches are split on (smgpu_halo_configure; all 0 on the direct-gather kernels): geometry tiles
 * with / without a shared point, regular smoothing tiles, tiles of the shared points only */
int smgpu_debug_halo_tiles(smgpu_handle* h, int32_t* geomShared, int32_t* geomInterior, int32_t* smoothTiles, int32_t* sharedPointTiles);

/* self-test of the geometry kernel's range-tested square root / division fast paths (csrc/fpexact.hpp) against the plain
 * IEEE operators on n generated arguments (random, zeros, denormals, inf / nan, both ends of the exponent range) on the
 * given device; *mismatches = number of results whose bits differ (nan == nan).  0 is the only acceptable count. */
int smgpu_debug_selftest_fpexact(int32_t device, uint64_t seed, int64_t n, int64_t* mismatches);

/* ---- debug / parity access (device -> host copy of an internal field) -----------------------
 * name: "cellCentres" [3C], "faceCentres" [3F], "faceAreas" [3F], "newPoints" [3P] (proposal of the
 * last iteration before restore), "isFrozenPoint" [P], "edgeMinAngle"/"edgeMaxAngle" [E],
 * "pointMinAngle"/"pointMaxAngle" [P].  Values are converted to double.  Returns the element
 * count through *n; out may be NULL to query the size.
 * "eaMaybe" [P], "faMaybe" [P]: the verdicts of the f32 filters in front of the two angle evaluators
 * (csrc/kernels_filter.hpp), 0 = GOOD for sure, 1 = left to the exact kernel ("faMaybe": the point
 * has an edge the face-angle filter could not decide; the mark is compared with the pass's tag, as for
 * "faActive").  They describe the latest constraint pass and are meant to be read after
 * smgpu_debug_propose under SMGPU_DEBUG_FILTERED=1; if that pass did not run the filter in question
 * (debug_propose without that variable, SMGPU_FILTER=0, the constraint off) the call fails with a
 * message instead of returning the bytes of an earlier pass. */
int smgpu_debug_get_field(smgpu_handle* h, const char* name, double* out, int64_t* n);
/* kind: pointCells, pointPoints, pointFaces, pointEdges, edgeFaces, edgeCells, edges (2/row).
 * offsets/values may be NULL to query nnz. */
int smgpu_debug_get_addressing(smgpu_handle* h, const char* kind, int32_t* offsets, int32_t* values, int64_t* nnz);
/* Run one iteration up to (not including) restore/movePoints so "newPoints"/"isFrozenPoint"
 * can be compared with the oracle's phaseA/phaseB. */
int smgpu_debug_propose(smgpu_handle* h);


/* ---- host-only addressing build (no device needed; used by the CPU test-suite and hosts that
 * want the derived lists, e.g. to compute getMeshStats defaults before choosing a device) ------- */
typedef struct smgpu_topology smgpu_topology;
int smgpu_topology_create(const smgpu_mesh_desc* desc, smgpu_topology** out);
int smgpu_topology_get(smgpu_topology* t, const char* kind, int32_t* offsets, int32_t* values, int64_t* nnz);
int smgpu_topology_num_edges(smgpu_topology* t, int32_t* nEdges);
int smgpu_topology_checksums(smgpu_topology* t, uint64_t* out /* [SMGPU_TOPO_CHECKSUMS], see smgpu_debug_addressing_checksums */);
int smgpu_topology_destroy(smgpu_topology* t);

#ifdef __cplusplus
}
#endif
#endif /* SMGPU_H */
