// kernels_quality.hpp -- mesh quality report of the current points (smgpu_mesh_quality / smgpu_quality_field and, for a sub-domain
// of a decomposed mesh, smgpu_quality_coupled_*: include/smgpu.h).
//
// Inputs are the loop's own geometry: face centres / area vectors by face id and cell centres by cell id, as the geometry
// kernel publishes them for ptsCur (runGeometry with writeFaces).  Definitions: DESIGN.md "Mesh quality" (after OpenFOAM
// primitiveMeshCheck).  Three passes, no float atomics: a face pass (one lane per face, polyMesh order) and a cell pass (one lane
// per cell) leave one partial record per workgroup; k_quality_final reduces the two slabs in a fixed order into one
// smgpu_quality (or, for a sub-domain, one smgpu_quality_part).  The face pass and the face flag pass are one kernel template
// each: the serial and the coupled report are its Coupled = false / true instantiations, and differ in what qNeighbour returns.
// Every reduction is a fixed xor butterfly inside the wave, the waves of a workgroup in wave order, and the workgroup records in
// a fixed stride order: the report is bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smgpu.h"
#include "kernels.hpp"
#include "vec3.hpp"
#include "smacos.hpp"

namespace smgpu {

constexpr int kQualityBlock = 256;
constexpr int kQualityNoId = 0x7fffffff;   // the id of an empty max / min (lowest-id tie rule: never wins a tie)

// partial record of the face pass (one per workgroup, then the final reduction's accumulator)
struct QFace {
    double maxNO, sumTh, maxSk, minA, maxA;
    int maxNOId, maxSkId;
    long long nSev, nErr, nSkew, nWrong, nZero;
};
// ... and of the cell pass
struct QCell {
    double minV, maxV, sumV, maxOpen, maxAR;
    int minVId;
    long long nNonPos, nOpen, nHigh;
};

template <class A> __device__ __forceinline__ A qEmpty();
template <> __device__ __forceinline__ QFace qEmpty<QFace>() {
    QFace a;
    a.maxNO = -__builtin_inf(); a.sumTh = 0.0; a.maxSk = -__builtin_inf(); a.minA = __builtin_inf(); a.maxA = -__builtin_inf();
    a.maxNOId = kQualityNoId; a.maxSkId = kQualityNoId;
    a.nSev = a.nErr = a.nSkew = a.nWrong = a.nZero = 0;
    return a;
}
template <> __device__ __forceinline__ QCell qEmpty<QCell>() {
    QCell a;
    a.minV = __builtin_inf(); a.maxV = -__builtin_inf(); a.sumV = 0.0; a.maxOpen = -__builtin_inf(); a.maxAR = -__builtin_inf();
    a.minVId = kQualityNoId;
    a.nNonPos = a.nOpen = a.nHigh = 0;
    return a;
}
// larger value wins, a tie goes to the lower id (an order-independent rule: the result does not depend on the reduction tree)
__device__ __forceinline__ void qMaxId(double& v, int& id, double ov, int oid) {
    if (ov > v || (ov == v && oid < id)) { v = ov; id = oid; }
}
__device__ __forceinline__ void qMinId(double& v, int& id, double ov, int oid) {
    if (ov < v || (ov == v && oid < id)) { v = ov; id = oid; }
}
__device__ __forceinline__ void qCombine(QFace& a, const QFace& b) {
    qMaxId(a.maxNO, a.maxNOId, b.maxNO, b.maxNOId);
    a.sumTh += b.sumTh;
    qMaxId(a.maxSk, a.maxSkId, b.maxSk, b.maxSkId);
    a.minA = fmin(a.minA, b.minA); a.maxA = fmax(a.maxA, b.maxA);
    a.nSev += b.nSev; a.nErr += b.nErr; a.nSkew += b.nSkew; a.nWrong += b.nWrong; a.nZero += b.nZero;
}
__device__ __forceinline__ void qCombine(QCell& a, const QCell& b) {
    qMinId(a.minV, a.minVId, b.minV, b.minVId);
    a.maxV = fmax(a.maxV, b.maxV);
    a.sumV += b.sumV;
    a.maxOpen = fmax(a.maxOpen, b.maxOpen); a.maxAR = fmax(a.maxAR, b.maxAR);
    a.nNonPos += b.nNonPos; a.nOpen += b.nOpen; a.nHigh += b.nHigh;
}
__device__ __forceinline__ QFace qShfl(const QFace& a, int o) {
    QFace r;
    r.maxNO = __shfl_xor(a.maxNO, o, 64); r.sumTh = __shfl_xor(a.sumTh, o, 64); r.maxSk = __shfl_xor(a.maxSk, o, 64);
    r.minA = __shfl_xor(a.minA, o, 64); r.maxA = __shfl_xor(a.maxA, o, 64);
    r.maxNOId = __shfl_xor(a.maxNOId, o, 64); r.maxSkId = __shfl_xor(a.maxSkId, o, 64);
    r.nSev = __shfl_xor(a.nSev, o, 64); r.nErr = __shfl_xor(a.nErr, o, 64); r.nSkew = __shfl_xor(a.nSkew, o, 64);
    r.nWrong = __shfl_xor(a.nWrong, o, 64); r.nZero = __shfl_xor(a.nZero, o, 64);
    return r;
}
__device__ __forceinline__ QCell qShfl(const QCell& a, int o) {
    QCell r;
    r.minV = __shfl_xor(a.minV, o, 64); r.maxV = __shfl_xor(a.maxV, o, 64); r.sumV = __shfl_xor(a.sumV, o, 64);
    r.maxOpen = __shfl_xor(a.maxOpen, o, 64); r.maxAR = __shfl_xor(a.maxAR, o, 64);
    r.minVId = __shfl_xor(a.minVId, o, 64);
    r.nNonPos = __shfl_xor(a.nNonPos, o, 64); r.nOpen = __shfl_xor(a.nOpen, o, 64); r.nHigh = __shfl_xor(a.nHigh, o, 64);
    return r;
}
// workgroup reduction in a fixed order: xor butterfly in each wave (a + b and b + a are the same IEEE sum, so every lane ends
// with the same bits), then the waves' records in wave order.  The result is valid in thread 0.
template <class A>
__device__ __forceinline__ A qBlockReduce(A v, A* sh /* [kQualityBlock / 64] in LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const A w = qShfl(v, o);
        qCombine(v, w);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = sh[0];
        for (int w = 1; w < kQualityBlock / 64; ++w) qCombine(v, sh[w]);
    }
    return v;
}

// Each workgroup takes kQualityPer * kQualityBlock consecutive elements, lane t the elements t, t + 256, ... (coalesced), so that
// the final reduction folds kQualityPer times fewer records (one workgroup folding one record per 256 elements took 0.7 ms on the
// 10 M-cell mesh: profiles/quality/README.md)
constexpr int kQualityPer = 8;
__host__ __device__ constexpr int qualityGrid(int n) { return (int)(((long long)n + kQualityPer * kQualityBlock - 1) / (kQualityPer * kQualityBlock)); }

// the workgroup's elements of [0, n) in lane order: each(i)
template <class Each>
__device__ __forceinline__ void qEach(int n, Each each) {
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int i = base + k * kQualityBlock;
        if (i >= n) break;
        each(i);
    }
}
// a reducing pass: one(i, e) fills the record e of element i; the lane folds its elements in order, the workgroup reduces, and
// part[blockIdx.x] takes the workgroup's record
template <class A, class One>
__device__ __forceinline__ void qPass(int n, A* __restrict__ part, One one) {
    __shared__ A sh[kQualityBlock / 64];
    A a = qEmpty<A>();
    qEach(n, [&](int i) {
        A e = qEmpty<A>();
        one(i, e);
        qCombine(a, e);
    });
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
// the final reduction's fold of one slab: thread t folds the records t, t + 256, ... in that order, then the workgroup reduction
// (valid in thread 0)
template <class A>
__device__ __forceinline__ A qFold(const A* __restrict__ part, int nB) {
    __shared__ A sh[kQualityBlock / 64];
    A a = qEmpty<A>();
    for (int i = threadIdx.x; i < nB; i += kQualityBlock) qCombine(a, part[i]);
    return qBlockReduce(a, sh);
}

// owner / neighbour of every face from the cell -> face rows (bit 31 = the cell is the face's neighbour): the addressing the
// engine holds on the device, so the first report uploads nothing.  Each face has one owner and at most one neighbour: plain
// stores, no race.
__global__ void __launch_bounds__(kQualityBlock) k_quality_owners(MeshView m, int* __restrict__ own, int* __restrict__ nei) {
    const int c = blockIdx.x * kQualityBlock + threadIdx.x;
    if (c >= m.nCells) return;
    for (int j = m.cfOff[c]; j < m.cfOff[c + 1]; ++j) {
        const int e = m.cfVal[j];
        const int f = e & 0x7fffffff;
        if (e < 0) { if (f < m.nInternalFaces) nei[f] = c; }
        else if (f < m.nFaces) own[f] = c;
    }
}

struct QualityThresholds { double cosNonOrth, skew, closed, aspect; };

constexpr double kRadToDeg = 180.0 / SMGPU_PI;

// ---- the neighbour side of a face ------------------------------------------------------------------------------------------
// A processor face of a decomposed mesh (smgpu_quality_coupled_*, DESIGN.md "Mesh quality", 10.4 and 10.8) is an internal face
// of the global mesh: it takes the internal-face branch of every criterion with the neighbour rank's cell centre and volume,
// which the host has moved into recvCc / recvVc.  slot[f - nInternalFaces] is the array smgpu_quality_coupled_pack builds: -1 on
// a physical boundary face, else the face's place in recvCc / recvVc (patch order), | kQualityNotCounted on the side with
// myRank > neighbRank: the record counts the face on the other side only, the per-face fields carry it on both.  The kernels of
// this file read it here only; the coupled geometry and motion kernels decode it themselves.
constexpr int kQualitySlotMask = 0x3fffffff;
constexpr int kQualityNotCounted = 0x40000000;
template <bool Coupled> struct QCoupling {};                   // the serial kernels carry no coupling
template <> struct QCoupling<true> { const int* __restrict__ slot; const double* __restrict__ recvCc; const double* __restrict__ recvVc; };

// cc: where the neighbour's cell centre is, valid where `internal`
struct QNeighbour { bool internal, counted; const double* cc; };
template <bool Coupled>
__device__ __forceinline__ QNeighbour qNeighbour(const MeshView& m, const double* __restrict__ cellCtr, const int* __restrict__ nei, const QCoupling<Coupled>& cp, int f) {
    if (f < m.nInternalFaces) {
        const int n = nei[f];
        return QNeighbour{true, true, cellCtr + 3 * (size_t)n};
    }
    if constexpr (Coupled) {
        const int sl = cp.slot[f - m.nInternalFaces];
        if (sl >= 0) {
            const int k = sl & kQualitySlotMask;
            return QNeighbour{true, !(sl & kQualityNotCounted), cp.recvCc + 3 * (size_t)k};
        }
    }
    return QNeighbour{false, true, nullptr};
}
__device__ __forceinline__ V3 qNeighbourCentre(const QNeighbour& nb) { return nb.internal ? v3(nb.cc[0], nb.cc[1], nb.cc[2]) : v3(0, 0, 0); }

// face pass: non-orthogonality (internal faces), skewness, both face pyramids, face area of face f.  outNO / outSkew: optional
// per-face fields (smgpu_quality_field), NULL for the report.
// one face with owner centre CO and, where `internal`, neighbour centre CN
__device__ __forceinline__ void qFaceCore(const MeshView& m, const double* __restrict__ pts, const V3 Cf, const V3 Sf, const V3 CO, bool internal,
                                          const V3 CN, const QualityThresholds& thr, int f, QFace& a, double* __restrict__ outNO,
                                          double* __restrict__ outSkew) {
    const double magSf = mag(Sf);
    a.minA = magSf; a.maxA = magSf;
    a.nZero = (magSf <= SMGPU_VSMALL) ? 1 : 0;
    const V3 Cpf = Cf - CO;
    const double pO = dot(Sf, Cpf);
    bool wrong = pO <= 0.0;
    V3 d;
    double theta = 0.0;
    if (internal) {
        d = CN - CO;
        const double ortho = dot(d, Sf) / (mag(d) * magSf + SMGPU_VSMALL);
        const double oc = fmin(fmax(ortho, -1.0), 1.0);
        theta = smacos::acosX(oc) * kRadToDeg;
        a.maxNO = theta; a.maxNOId = f;
        a.sumTh = theta;
        a.nSev = (ortho > 0.0 && ortho < thr.cosNonOrth) ? 1 : 0;
        a.nErr = (ortho <= 0.0) ? 1 : 0;
        const double pN = dot(Sf, CN - Cf);
        wrong = wrong || pN <= 0.0;
    } else {
        const V3 n = Sf / (magSf + SMGPU_ROOTVSMALL);
        d = dot(n, Cpf) * n;
    }
    a.nWrong = wrong ? 1 : 0;
    // skewness
    const V3 sv = Cpf - (dot(Sf, Cpf) / (dot(Sf, d) + SMGPU_ROOTVSMALL)) * d;
    const double magSv = mag(sv);
    const V3 sHat = sv / (magSv + SMGPU_ROOTVSMALL);
    double fd = 0.2 * mag(d) + SMGPU_ROOTVSMALL;
    for (int j = m.faceOff[f]; j < m.faceOff[f + 1]; ++j) fd = fmax(fd, fabs(dot(sHat, ldv(pts, m.facePts[j]) - Cf)));
    const double skew = magSv / fd;
    a.maxSk = skew; a.maxSkId = f;
    a.nSkew = (skew > thr.skew) ? 1 : 0;
    if (outNO) outNO[f] = theta;
    if (outSkew) outSkew[f] = skew;
}
template <bool Coupled>
__device__ __forceinline__ void qFaceOne(const MeshView& m, const double* __restrict__ pts, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                         const double* __restrict__ cellCtr, const int* __restrict__ own, const int* __restrict__ nei,
                                         const QCoupling<Coupled>& cp, const QualityThresholds& thr, int f, QFace& a, double* __restrict__ outNO,
                                         double* __restrict__ outSkew) {
    const QNeighbour nb = qNeighbour(m, cellCtr, nei, cp, f);
    qFaceCore(m, pts, ldv(fCtr, f), ldv(fArea, f), ldv(cellCtr, own[f]), nb.internal, qNeighbourCentre(nb), thr, f, a, outNO, outSkew);
    if (!nb.counted) a = qEmpty<QFace>();
}
template <bool Coupled>
__global__ void __launch_bounds__(kQualityBlock) k_quality_faces(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                  const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                  const int* __restrict__ own, const int* __restrict__ nei, QCoupling<Coupled> cp,
                                                                  QualityThresholds thr, QFace* __restrict__ part, double* __restrict__ outNO,
                                                                  double* __restrict__ outSkew) {
    qPass(m.nFaces, part, [&](int f, QFace& e) { qFaceOne(m, pts, fCtr, fArea, cellCtr, own, nei, cp, thr, f, e, outNO, outSkew); });
}

// the signed volume of cell c: the estimated centre (mean of the face centres), then a third of the signed face pyramids, faces in
// the cell's geometry order (cfOff / cfVal), sign -1 on the neighbour side.  extra(flipped, f, Sf): the caller's own sums over
// the same faces, each its own chain
template <class Extra>
__device__ __forceinline__ double qCellVolume(const MeshView& m, const double* __restrict__ fCtr, const double* __restrict__ fArea, int c, Extra extra) {
    const int b = m.cfOff[c], e = m.cfOff[c + 1];
    V3 cEst = v3(0, 0, 0);
    for (int j = b; j < e; ++j) cEst = cEst + ldv(fCtr, m.cfVal[j] & 0x7fffffff);
    cEst = cEst / (double)(e - b);
    double pyr = 0.0;
    for (int j = b; j < e; ++j) {
        const int ev = m.cfVal[j];
        const int f = ev & 0x7fffffff;
        const V3 Sf = ldv(fArea, f);
        double p = dot(Sf, ldv(fCtr, f) - cEst);
        if (ev < 0) p = -p;
        extra(ev < 0, f, Sf);
        pyr += p;
    }
    return (1.0 / 3.0) * pyr;
}

// cell pass: signed volume, openness, aspect ratio of cell c.  outV / outOpen / outAR: optional per-cell fields, NULL for the report.
__device__ __forceinline__ void qCellOne(const MeshView& m, const double* __restrict__ fCtr, const double* __restrict__ fArea, const QualityThresholds& thr,
                                         int c, QCell& a, double* __restrict__ outV, double* __restrict__ outOpen, double* __restrict__ outAR) {
    {
        V3 sumS = v3(0, 0, 0), M = v3(0, 0, 0);
        const double V = qCellVolume(m, fCtr, fArea, c, [&](bool flipped, int, const V3& Sf) {
            if (flipped) sumS = sumS - Sf;
            else sumS = sumS + Sf;
            M = M + v3(fabs(Sf.x), fabs(Sf.y), fabs(Sf.z));
        });
        const double open = fmax(fmax(fabs(sumS.x) / (M.x + SMGPU_ROOTVSMALL), fabs(sumS.y) / (M.y + SMGPU_ROOTVSMALL)),
                                 fabs(sumS.z) / (M.z + SMGPU_ROOTVSMALL));
        const double maxM = fmax(fmax(M.x, M.y), M.z), minM = fmin(fmin(M.x, M.y), M.z);
        const double ar = fmax(maxM / (minM + SMGPU_ROOTVSMALL),
                               ((1.0 / 6.0) * ((M.x + M.y) + M.z)) / pow(fmax(V, SMGPU_ROOTVSMALL), 2.0 / 3.0));
        a.minV = V; a.minVId = c; a.maxV = V; a.sumV = V;
        a.nNonPos = (V <= SMGPU_VSMALL) ? 1 : 0;
        a.maxOpen = open; a.nOpen = (open > thr.closed) ? 1 : 0;
        a.maxAR = ar; a.nHigh = (ar > thr.aspect) ? 1 : 0;
        if (outV) outV[c] = V;
        if (outOpen) outOpen[c] = open;
        if (outAR) outAR[c] = ar;
    }
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_cells(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                  QualityThresholds thr, QCell* __restrict__ part, double* __restrict__ outV,
                                                                  double* __restrict__ outOpen, double* __restrict__ outAR) {
    qPass(m.nCells, part, [&](int c, QCell& e) { qCellOne(m, fCtr, fArea, thr, c, e, outV, outOpen, outAR); });
}

// the serial report of the folded record: the average in place of the sum
__device__ __forceinline__ void qFinish(const smgpu_quality_part& q, smgpu_quality_part* __restrict__ out) { *out = q; }
__device__ __forceinline__ void qFinish(const smgpu_quality_part& q, smgpu_quality* __restrict__ out) {
    smgpu_quality r;
    r.nCells = q.nCells; r.nFaces = q.nFaces; r.nInternalFaces = q.nInternalFaces;
    r.minVolume = q.minVolume; r.maxVolume = q.maxVolume; r.totalVolume = q.totalVolume;
    r.nNonPositiveVolume = q.nNonPositiveVolume; r.minVolumeCell = q.minVolumeCell;
    r.minFaceArea = q.minFaceArea; r.maxFaceArea = q.maxFaceArea; r.nZeroAreaFaces = q.nZeroAreaFaces;
    r.maxNonOrth = q.maxNonOrth; r.avgNonOrth = q.nInternalFaces > 0 ? q.sumNonOrth / (double)q.nInternalFaces : 0.0;
    r.nSevereNonOrth = q.nSevereNonOrth; r.nErrorNonOrth = q.nErrorNonOrth; r.maxNonOrthFace = q.maxNonOrthFace;
    r.maxSkewness = q.maxSkewness; r.nSkewFaces = q.nSkewFaces; r.maxSkewFace = q.maxSkewFace;
    r.nWrongOrientedFaces = q.nWrongOrientedFaces;
    r.maxOpenness = q.maxOpenness; r.nOpenCells = q.nOpenCells;
    r.maxAspectRatio = q.maxAspectRatio; r.nHighAspectCells = q.nHighAspectCells;
    *out = r;
}
// one workgroup folds the two slabs into the record of sums and denominators.  Out = smgpu_quality_part: the per-rank record of a
// decomposed mesh (nFaces / nInternalFaces are the counted ones); Out = smgpu_quality: the serial report
template <class Out>
__global__ void __launch_bounds__(kQualityBlock) k_quality_final(const QFace* __restrict__ fPart, int nFB, const QCell* __restrict__ cPart, int nCB,
                                                                  int nCells, int nFaces, int nInternalFaces, Out* __restrict__ out) {
    const QFace a = qFold(fPart, nFB);
    const QCell b = qFold(cPart, nCB);
    if (threadIdx.x != 0) return;
    smgpu_quality_part q;
    q.nCells = nCells; q.nFaces = nFaces; q.nInternalFaces = nInternalFaces;
    const bool anyCell = nCells > 0, anyFace = nFaces > 0, anyInternal = nInternalFaces > 0;
    q.minVolume = anyCell ? b.minV : 0.0; q.maxVolume = anyCell ? b.maxV : 0.0; q.totalVolume = b.sumV;
    q.nNonPositiveVolume = b.nNonPos; q.minVolumeCell = anyCell ? b.minVId : -1;
    q.minFaceArea = anyFace ? a.minA : 0.0; q.maxFaceArea = anyFace ? a.maxA : 0.0; q.nZeroAreaFaces = a.nZero;
    q.maxNonOrth = anyInternal ? a.maxNO : 0.0; q.sumNonOrth = a.sumTh;
    q.nSevereNonOrth = a.nSev; q.nErrorNonOrth = a.nErr; q.maxNonOrthFace = anyInternal ? a.maxNOId : -1;
    q.maxSkewness = anyFace ? a.maxSk : 0.0; q.nSkewFaces = a.nSkew; q.maxSkewFace = anyFace ? a.maxSkId : -1;
    q.nWrongOrientedFaces = a.nWrong;
    q.maxOpenness = anyCell ? b.maxOpen : 0.0; q.nOpenCells = b.nOpen;
    q.maxAspectRatio = anyCell ? b.maxAR : 0.0; q.nHighAspectCells = b.nHigh;
    qFinish(q, out);
}

// the owner cell centre of every processor face, in patch order: what the neighbour rank needs as its C_N
__global__ void __launch_bounds__(kQualityBlock) k_quality_pack(const int* __restrict__ own, const double* __restrict__ cellCtr,
                                                                 const int* __restrict__ procFace, int nProc, double* __restrict__ sendCc) {
    const int i = blockIdx.x * kQualityBlock + threadIdx.x;
    if (i >= nProc) return;
    const V3 c = ldv(cellCtr, own[procFace[i]]);
    sendCc[3 * (size_t)i] = c.x; sendCc[3 * (size_t)i + 1] = c.y; sendCc[3 * (size_t)i + 2] = c.z;
}

// ---- the failing elements as sets (smgpu_quality_sets / _coupled_sets, DESIGN.md "Mesh quality", 10.5) ------------------------
// Three steps, no atomics:
//   1. flag passes (the report's face / cell passes with the same qFaceOne / qCellOne records): one mask byte per
//      element (bit s = member of set s of its kind), and per workgroup the member count of every set: cnt[row(s) + block];
//   2. k_quality_set_scan: one exclusive scan of cnt in its flat order.  Rows go set by set (the 4 face sets over the face
//      workgroups, then the 3 cell sets over the cell workgroups), so the scan is at once each workgroup's offset inside its
//      set and the set's offset inside the concatenated output;
//   3. k_quality_set_scatter: each workgroup walks its 2048 elements in 256-element rounds; a wave ranks its members with a
//      64-bit ballot, the waves' totals go through LDS in wave order.  Ids come out ascending.
// qFlagPass, the scan and the scatter also serve the sets of the -allGeometry checks and of the motion criteria (10.9), whose flag
// passes are in kernels_quality_geom.hpp and kernels_quality_motion.hpp: scan and scatter are templates over the set layout.
constexpr int kQualityFaceSets = 4;   // nonOrthoFaces, skewFaces, wrongOrientedFaces, zeroAreaFaces
constexpr int kQualityCellSets = 3;   // zeroVolumeCells, nonClosedCells, highAspectRatioCells

__device__ __forceinline__ unsigned qFaceBits(const QFace& e) {
    return ((e.nSev | e.nErr) ? 1u : 0u) | (e.nSkew ? 2u : 0u) | (e.nWrong ? 4u : 0u) | (e.nZero ? 8u : 0u);
}
__device__ __forceinline__ unsigned qCellBits(const QCell& e) {
    return (e.nNonPos ? 1u : 0u) | (e.nOpen ? 2u : 0u) | (e.nHigh ? 4u : 0u);
}
// the member counts of the workgroup's rounds (bits of each round's elements), set by set, into cnt[s * nB + blockIdx.x]
template <int NS>
__device__ __forceinline__ void qSetCountStore(const int (&waveCnt)[NS], int* __restrict__ sh /* [NS][4] */, int* __restrict__ cnt, int nB) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int s = 0; s < NS; ++s) sh[s * (kQualityBlock / 64) + w] = waveCnt[s];
    __syncthreads();
    if (threadIdx.x < NS) {
        int t = 0;
        for (int v = 0; v < kQualityBlock / 64; ++v) t += sh[threadIdx.x * (kQualityBlock / 64) + v];
        cnt[(size_t)threadIdx.x * nB + blockIdx.x] = t;
    }
}

// a flag pass: bitsOf(i) gives the mask byte of element i (a face the neighbour rank counts is in no set here).  Not qEach: a
// lane past the end must not leave the loop, every lane of the wave has to reach the ballots of every round
template <int NS, class Bits>
__device__ __forceinline__ void qFlagPass(int n, uint8_t* __restrict__ mask, int* __restrict__ cnt, Bits bitsOf) {
    __shared__ int sh[NS * (kQualityBlock / 64)];
    int wc[NS] = {};
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int i = base + k * kQualityBlock;
        unsigned bits = 0;
        if (i < n) {
            bits = bitsOf(i);
            mask[i] = (uint8_t)bits;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) wc[s] += __popcll(__ballot((bits >> s) & 1u));
    }
    qSetCountStore(wc, sh, cnt, gridDim.x);
}
template <bool Coupled>
__global__ void __launch_bounds__(kQualityBlock) k_quality_face_flags(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                       const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                       const int* __restrict__ own, const int* __restrict__ nei, QCoupling<Coupled> cp,
                                                                       QualityThresholds thr, uint8_t* __restrict__ mask, int* __restrict__ cnt) {
    qFlagPass<kQualityFaceSets>(m.nFaces, mask, cnt, [&](int f) {
        QFace e = qEmpty<QFace>();
        qFaceOne(m, pts, fCtr, fArea, cellCtr, own, nei, cp, thr, f, e, nullptr, nullptr);
        return qFaceBits(e);
    });
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_cell_flags(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                       QualityThresholds thr, uint8_t* __restrict__ mask, int* __restrict__ cnt) {
    qFlagPass<kQualityCellSets>(m.nCells, mask, cnt, [&](int c) {
        QCell e = qEmpty<QCell>();
        qCellOne(m, fCtr, fArea, thr, c, e, nullptr, nullptr, nullptr);
        return qCellBits(e);
    });
}

// one workgroup of 1024: exclusive scan of cnt[0, n) into off[0, n] (off[n] = the total), tile by tile in index order; then the
// set sizes: counts[s] = off[rowEnd(s)] - off[rowStart(s)].  <NF, NC>: the set layout, NF face sets over the face workgroups
// then NC cell sets over the cell workgroups -- <4, 3> for the report of this file, <4, 1> for the -allGeometry checks and
// <4, 0> for the motion criteria (with NC = 0 there are no cell rows and nCB is 0)
constexpr int kQualityScanBlock = 1024;
template <int NF, int NC>
__global__ void __launch_bounds__(kQualityScanBlock) k_quality_set_scan(const int* __restrict__ cnt, int n, int nFB, int nCB,
                                                                         long long* __restrict__ off, long long* __restrict__ counts) {
    __shared__ long long shW[kQualityScanBlock / 64];
    __shared__ long long shCarry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) shCarry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += kQualityScanBlock) {
        const int i = t0 + threadIdx.x;
        const long long v = i < n ? (long long)cnt[i] : 0;
        long long x = v;                               // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) shW[w] = x;
        __syncthreads();
        long long before = shCarry;
        for (int u = 0; u < w; ++u) before += shW[u];
        if (i < n) off[i] = before + x - v;
        __syncthreads();                               // every thread has read shCarry and shW
        if (threadIdx.x == kQualityScanBlock - 1) shCarry = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = shCarry;
    __syncthreads();
    if (threadIdx.x < NF + NC) {
        const int s = threadIdx.x;
        const int b = s < NF ? s * nFB : NF * nFB + (s - NF) * nCB;
        const int e = b + (s < NF ? nFB : nCB);
        counts[s] = off[e] - off[b];
    }
}

// workgroups [0, nFB) take the face sets of face workgroup b, the rest the cell sets of cell workgroup b - nFB (mask[nFaces + c]).
// A member's place: the scan's offset of (set, workgroup), plus the members of the earlier rounds, of the earlier waves of this
// round, and of the lower lanes of its wave.  pos < total always holds (the masks are the ones counted); it is checked anyway.
// <NF, NC> as k_quality_set_scan; with NC = 0 the grid is the nFB face workgroups and the mask holds nFaces bytes only.
template <int NF, int NC>
__global__ void __launch_bounds__(kQualityBlock) k_quality_set_scatter(const uint8_t* __restrict__ mask, int nFaces, int nCells, int nFB, int nCB,
                                                                        const long long* __restrict__ off, int* __restrict__ ids, long long total) {
    static_assert(NC <= NF && NF <= 8, "a cell workgroup uses the face sets' slots; one mask byte per element");
    __shared__ int sh[2][NF][kQualityBlock / 64];
    const bool faces = (int)blockIdx.x < nFB;
    const int b = faces ? (int)blockIdx.x : (int)blockIdx.x - nFB;
    const int n = faces ? nFaces : nCells;
    const int ns = faces ? NF : NC;
    const uint8_t* mk = faces ? mask : mask + nFaces;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    long long run[NF];
    for (int s = 0; s < NF; ++s)
        run[s] = s < ns ? off[faces ? s * nFB + b : NF * nFB + s * nCB + b] : 0;
    for (int k = 0; k < kQualityPer; ++k) {
        const int i0 = b * (kQualityPer * kQualityBlock) + k * kQualityBlock;
        if (i0 >= n) break;                            // uniform in the workgroup
        const int i = i0 + threadIdx.x;
        const unsigned bits = i < n ? mk[i] : 0u;
        const int buf = k & 1;                         // two LDS buffers: round k + 1 writes while no wave still reads round k's
        unsigned long long bal[NF];
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            bal[s] = __ballot((bits >> s) & 1u);
            if (lane == 0) sh[buf][s][w] = __popcll(bal[s]);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            if (s >= ns) break;
            int before = 0, all = 0;
            for (int v = 0; v < kQualityBlock / 64; ++v) {
                const int c = sh[buf][s][v];
                if (v < w) before += c;
                all += c;
            }
            if ((bits >> s) & 1u) {
                const long long pos = run[s] + before + __popcll(bal[s] & below);
                if (pos < total) ids[pos] = i;
            }
            run[s] += all;
        }
    }
}

}  // namespace smgpu
