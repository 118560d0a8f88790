// kernels_quality_motion.hpp -- the motion criteria of the quality report (smgpu_mesh_quality_motion / smgpu_quality_motion_field:
// include/smgpu.h): the meshQualityDict checks that the reports of kernels_quality.hpp and kernels_quality_geom.hpp do not cover --
// face-centre tet quality, base-point tet quality (the decomposition particle tracking uses), face twist, triangle twist.
// Definitions: DESIGN.md "Mesh quality", 10.7.
//
// Same inputs and the same layout as kernels_quality.hpp: face centres by face id and cell centres by cell id as the loop's
// geometry launch publishes them, kQualityBlock threads, kQualityPer faces per lane (lane t the faces t, t + 256, ...), one partial
// record per workgroup, one folding workgroup at the end, no float atomics.  A face pass only: every criterion is per face.
// For a sub-domain of a decomposed mesh (smgpu_quality_coupled_motion_*) k_quality_motion_faces_coupled runs: a
// processor face takes the internal-face branch of the tets and the twist with the neighbour rank's cell centre.  The serial and
// the coupled face pass stay a pair, with their own pass loops: one shared body changed the register allocation and cost 2 % of
// kernel time (profiles/quality/README.md), so they are the functions that were measured.
// The findings as sets (smgpu_quality_motion_sets / _coupled_motion_sets): the flag pass at the end of this file.
#pragma once
#include "kernels_quality.hpp"

namespace smgpu {

// partial record of the face pass
struct QMFace {
    double minTet, sumTet, minBase, minTw, sumTw, minTri, sumTri;
    int minTetId, minBaseId, minTwId, minTriId;
    long long nLowTet, nNoBase, nTw, nLowTw, nLowTri;
};

template <> __device__ __forceinline__ QMFace qEmpty<QMFace>() {
    QMFace a;
    a.minTet = a.minBase = a.minTw = a.minTri = __builtin_inf();
    a.sumTet = a.sumTw = a.sumTri = 0.0;
    a.minTetId = a.minBaseId = a.minTwId = a.minTriId = kQualityNoId;
    a.nLowTet = a.nNoBase = a.nTw = a.nLowTw = a.nLowTri = 0;
    return a;
}
__device__ __forceinline__ void qCombine(QMFace& a, const QMFace& b) {
    qMinId(a.minTet, a.minTetId, b.minTet, b.minTetId);
    qMinId(a.minBase, a.minBaseId, b.minBase, b.minBaseId);
    qMinId(a.minTw, a.minTwId, b.minTw, b.minTwId);
    qMinId(a.minTri, a.minTriId, b.minTri, b.minTriId);
    a.sumTet += b.sumTet; a.sumTw += b.sumTw; a.sumTri += b.sumTri;
    a.nLowTet += b.nLowTet; a.nNoBase += b.nNoBase; a.nTw += b.nTw; a.nLowTw += b.nLowTw; a.nLowTri += b.nLowTri;
}
__device__ __forceinline__ QMFace qShfl(const QMFace& a, int o) {
    QMFace r;
    r.minTet = __shfl_xor(a.minTet, o, 64); r.sumTet = __shfl_xor(a.sumTet, o, 64); r.minBase = __shfl_xor(a.minBase, o, 64);
    r.minTw = __shfl_xor(a.minTw, o, 64); r.sumTw = __shfl_xor(a.sumTw, o, 64);
    r.minTri = __shfl_xor(a.minTri, o, 64); r.sumTri = __shfl_xor(a.sumTri, o, 64);
    r.minTetId = __shfl_xor(a.minTetId, o, 64); r.minBaseId = __shfl_xor(a.minBaseId, o, 64);
    r.minTwId = __shfl_xor(a.minTwId, o, 64); r.minTriId = __shfl_xor(a.minTriId, o, 64);
    r.nLowTet = __shfl_xor(a.nLowTet, o, 64); r.nNoBase = __shfl_xor(a.nNoBase, o, 64); r.nTw = __shfl_xor(a.nTw, o, 64);
    r.nLowTw = __shfl_xor(a.nLowTw, o, 64); r.nLowTri = __shfl_xor(a.nLowTri, o, 64);
    return r;
}

// k: the host's 8.0 / (9.0 * sqrt(3.0)), the normalisation that gives a regular tetrahedron |q| = 1
struct QualityMotionThresholds { double tet, twist, triTwist, k; };

// tet quality q(a, b, c, d) with u = b - a, v = c - a and n = u x v given (the two sides of a face share them), d the apex:
// signed volume over the volume of the regular tetrahedron with the same circumradius
__device__ __forceinline__ double qmTetQ(const V3& a, const V3& u, const V3& v, const V3& n, const V3& d, double k) {
    const V3 w = d - a;
    const double D = dot(n, w);
    double R = SMGPU_GREAT;
    if (fabs(D) >= SMGPU_ROOTVSMALL) {
        const V3 num = (magSqr(w) * n + magSqr(v) * cross(w, u)) + magSqr(u) * cross(v, w);
        R = fmin(mag(num) / (2.0 * fabs(D)), SMGPU_GREAT);
    }
    return (D / 6.0) / (k * ((R * R) * R) + SMGPU_ROOTVSMALL);
}
// the smaller of the owner's and (internal faces) the neighbour's tet on the triangle (a, a + u, a + v): the signs make a valid
// tet positive on both sides
__device__ __forceinline__ double qmTetPair(const V3& a, const V3& u, const V3& v, const V3& CO, bool internal, const V3& CN, double k) {
    const V3 n = cross(u, v);
    double q = -qmTetQ(a, u, v, n, CO, k);
    if (internal) q = fmin(q, qmTetQ(a, u, v, n, CN, k));
    return q;
}

// Two walks over the face's points, read by id as the skewness loop does (no per-lane array of points).  The first reads each
// vertex once and gives the face-centre tets of both sides, the twist and the triangle twist: the first point and the first
// valid unit triangle normal are carried to close the cycle.  The second gives the base-point tets: for every base the fan
// (p_b, p_{b+k}, p_{b+k+1}), the edge p_{b+k+1} - p_b carried from one tet to the next.  out*: optional per-face fields.
__device__ __forceinline__ void qmFaceOne(const MeshView& m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                          const double* __restrict__ cellCtr, const int* __restrict__ own, const int* __restrict__ nei,
                                          const QualityMotionThresholds& thr, int f, QMFace& a, double* __restrict__ outTet,
                                          double* __restrict__ outBase, double* __restrict__ outTw, double* __restrict__ outTri) {
    const V3 Cf = ldv(fCtr, f);
    const bool internal = f < m.nInternalFaces;
    const V3 CO = ldv(cellCtr, own[f]);
    const V3 CN = internal ? ldv(cellCtr, nei[f]) : v3(0, 0, 0);
    const int jb = m.faceOff[f], nv = m.faceOff[f + 1] - jb;
    const bool summed = nv > 3;
    double tet = __builtin_inf(), tw = __builtin_inf(), tri = __builtin_inf();
    int nValid = 0;
    if (nv > 0) {
        const V3 dv = sel3(internal, CN, Cf) - CO;
        const V3 nHat = dv / (mag(dv) + SMGPU_VSMALL);
        const V3 p0 = ldv(pts, m.facePts[jb]);
        V3 cur = p0, hFirst = v3(0, 0, 0), hPrev = v3(0, 0, 0);
        for (int i = 0; i < nv; ++i) {
            const V3 nxt = (i + 1 < nv) ? ldv(pts, m.facePts[jb + i + 1]) : p0;
            const V3 u = nxt - cur, v = Cf - cur;
            tet = fmin(tet, qmTetPair(cur, u, v, CO, internal, CN, thr.k));
            if (summed) {
                const V3 t = 0.5 * cross(u, v);
                const double mt = mag(t);
                if (mt > SMGPU_VSMALL) {
                    const V3 h = t / mt;
                    tw = fmin(tw, dot(nHat, h));
                    if (nValid > 0) tri = fmin(tri, dot(hPrev, h));
                    else hFirst = h;
                    hPrev = h;
                    ++nValid;
                }
            }
            cur = nxt;
        }
        if (nValid >= 2) tri = fmin(tri, dot(hPrev, hFirst));
    }
    double base = __builtin_inf();
    for (int b = 0; b < nv; ++b) {
        const V3 pb = ldv(pts, m.facePts[jb + b]);
        int i = b + 1 < nv ? b + 1 : b + 1 - nv;
        V3 u = ldv(pts, m.facePts[jb + i]) - pb;
        double mb = __builtin_inf();
        for (int k = 1; k + 2 <= nv; ++k) {
            i = i + 1 < nv ? i + 1 : 0;
            const V3 v = ldv(pts, m.facePts[jb + i]) - pb;
            mb = fmin(mb, qmTetPair(pb, u, v, CO, internal, CN, thr.k));
            u = v;
        }
        if (b == 0 || mb > base) base = mb;
    }
    a.minTet = tet; a.minTetId = f; a.sumTet = tet; a.nLowTet = (tet < thr.tet) ? 1 : 0;
    a.minBase = base; a.minBaseId = f; a.nNoBase = (base < thr.tet) ? 1 : 0;
    if (nValid < 1) tw = 1.0;
    if (nValid < 2) tri = 1.0;
    if (summed) {
        a.minTw = tw; a.minTwId = f; a.sumTw = tw; a.nTw = 1; a.nLowTw = (tw < thr.twist) ? 1 : 0;
        a.minTri = tri; a.minTriId = f; a.sumTri = tri; a.nLowTri = (tri < thr.triTwist) ? 1 : 0;
    }
    if (outTet) outTet[f] = tet;
    if (outBase) outBase[f] = base;
    if (outTw) outTw[f] = tw;
    if (outTri) outTri[f] = tri;
}
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_faces(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                         const double* __restrict__ cellCtr, const int* __restrict__ own,
                                                                         const int* __restrict__ nei, QualityMotionThresholds thr,
                                                                         QMFace* __restrict__ part, double* __restrict__ outTet,
                                                                         double* __restrict__ outBase, double* __restrict__ outTw,
                                                                         double* __restrict__ outTri) {
    __shared__ QMFace sh[kQualityBlock / 64];
    QMFace a = qEmpty<QMFace>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QMFace e = qEmpty<QMFace>();
        qmFaceOne(m, pts, fCtr, cellCtr, own, nei, thr, f, e, outTet, outBase, outTw, outTri);
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// qmFaceOne with `internal` and C_N given by the caller, so that a processor face takes the internal-face branch of the tets
// and the twist with the neighbour rank's cell centre.  Its twin: the two walks, statement by statement; with
// internal = f < nInternalFaces and C_N = cellCtr[nei[f]] the same bits.  Keep the two alike.
__device__ __forceinline__ void qmFaceOneCoupled(const MeshView& m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                 const V3 CO, const bool internal, const V3 CN, const QualityMotionThresholds& thr, int f,
                                                 QMFace& a, double* __restrict__ outTet, double* __restrict__ outBase,
                                                 double* __restrict__ outTw, double* __restrict__ outTri) {
    const V3 Cf = ldv(fCtr, f);
    const int jb = m.faceOff[f], nv = m.faceOff[f + 1] - jb;
    const bool summed = nv > 3;
    double tet = __builtin_inf(), tw = __builtin_inf(), tri = __builtin_inf();
    int nValid = 0;
    if (nv > 0) {
        const V3 dv = sel3(internal, CN, Cf) - CO;
        const V3 nHat = dv / (mag(dv) + SMGPU_VSMALL);
        const V3 p0 = ldv(pts, m.facePts[jb]);
        V3 cur = p0, hFirst = v3(0, 0, 0), hPrev = v3(0, 0, 0);
        for (int i = 0; i < nv; ++i) {
            const V3 nxt = (i + 1 < nv) ? ldv(pts, m.facePts[jb + i + 1]) : p0;
            const V3 u = nxt - cur, v = Cf - cur;
            tet = fmin(tet, qmTetPair(cur, u, v, CO, internal, CN, thr.k));
            if (summed) {
                const V3 t = 0.5 * cross(u, v);
                const double mt = mag(t);
                if (mt > SMGPU_VSMALL) {
                    const V3 h = t / mt;
                    tw = fmin(tw, dot(nHat, h));
                    if (nValid > 0) tri = fmin(tri, dot(hPrev, h));
                    else hFirst = h;
                    hPrev = h;
                    ++nValid;
                }
            }
            cur = nxt;
        }
        if (nValid >= 2) tri = fmin(tri, dot(hPrev, hFirst));
    }
    double base = __builtin_inf();
    for (int b = 0; b < nv; ++b) {
        const V3 pb = ldv(pts, m.facePts[jb + b]);
        int i = b + 1 < nv ? b + 1 : b + 1 - nv;
        V3 u = ldv(pts, m.facePts[jb + i]) - pb;
        double mb = __builtin_inf();
        for (int k = 1; k + 2 <= nv; ++k) {
            i = i + 1 < nv ? i + 1 : 0;
            const V3 v = ldv(pts, m.facePts[jb + i]) - pb;
            mb = fmin(mb, qmTetPair(pb, u, v, CO, internal, CN, thr.k));
            u = v;
        }
        if (b == 0 || mb > base) base = mb;
    }
    a.minTet = tet; a.minTetId = f; a.sumTet = tet; a.nLowTet = (tet < thr.tet) ? 1 : 0;
    a.minBase = base; a.minBaseId = f; a.nNoBase = (base < thr.tet) ? 1 : 0;
    if (nValid < 1) tw = 1.0;
    if (nValid < 2) tri = 1.0;
    if (summed) {
        a.minTw = tw; a.minTwId = f; a.sumTw = tw; a.nTw = 1; a.nLowTw = (tw < thr.twist) ? 1 : 0;
        a.minTri = tri; a.minTriId = f; a.sumTri = tri; a.nLowTri = (tri < thr.triTwist) ? 1 : 0;
    }
    if (outTet) outTet[f] = tet;
    if (outBase) outBase[f] = base;
    if (outTw) outTw[f] = tw;
    if (outTri) outTri[f] = tri;
}
// k_quality_motion_faces with processor faces: one body for the three kinds of face, the slot only selects where C_N comes
// from (148 VGPR where k_quality_motion_faces holds 146, both three waves per SIMD)
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_faces_coupled(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                                 const double* __restrict__ cellCtr, const int* __restrict__ own,
                                                                                 const int* __restrict__ nei, const int* __restrict__ slot,
                                                                                 const double* __restrict__ recvCc, QualityMotionThresholds thr,
                                                                                 QMFace* __restrict__ part, double* __restrict__ outTet,
                                                                                 double* __restrict__ outBase, double* __restrict__ outTw,
                                                                                 double* __restrict__ outTri) {
    __shared__ QMFace sh[kQualityBlock / 64];
    QMFace a = qEmpty<QMFace>();
    const int base = blockIdx.x * (kQualityPer * kQualityBlock) + threadIdx.x;
    for (int k = 0; k < kQualityPer; ++k) {
        const int f = base + k * kQualityBlock;
        if (f >= m.nFaces) break;
        QMFace e = qEmpty<QMFace>();
        const int sl = f < m.nInternalFaces ? -1 : slot[f - m.nInternalFaces];
        // C_N by address: the neighbour cell's row of cellCtr, the slot's row of recvCc, or (physical patch, unused) the owner's row
        const double* cnAt = f < m.nInternalFaces ? cellCtr + 3 * (size_t)nei[f]
                                                  : (sl >= 0 ? recvCc + 3 * (size_t)(sl & kQualitySlotMask) : cellCtr + 3 * (size_t)own[f]);
        const bool internal = f < m.nInternalFaces || sl >= 0;
        const V3 CN = internal ? v3(cnAt[0], cnAt[1], cnAt[2]) : v3(0, 0, 0);
        qmFaceOneCoupled(m, pts, fCtr, ldv(cellCtr, own[f]), internal, CN, thr, f, e, outTet, outBase, outTw, outTri);
        if (sl >= 0 && (sl & kQualityNotCounted)) e = qEmpty<QMFace>();
        qCombine(a, e);
    }
    a = qBlockReduce(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// the serial report of the folded record: the averages in place of the sums
__device__ __forceinline__ void qFinish(const smgpu_quality_motion_part& q, smgpu_quality_motion_part* __restrict__ out) { *out = q; }
__device__ __forceinline__ void qFinish(const smgpu_quality_motion_part& q, smgpu_quality_motion* __restrict__ out) {
    smgpu_quality_motion r;
    const bool anyFace = q.nFaces > 0, anyTw = q.nTwistFaces > 0;
    r.minTetQuality = q.minTetQuality; r.avgTetQuality = anyFace ? q.sumTetQuality / (double)q.nFaces : 1.0;
    r.nLowTetFaces = q.nLowTetFaces; r.minTetFace = q.minTetFace;
    r.minBaseTetQuality = q.minBaseTetQuality; r.nNoBasePointFaces = q.nNoBasePointFaces; r.minBaseTetFace = q.minBaseTetFace;
    r.minTwist = q.minTwist; r.avgTwist = anyTw ? q.sumTwist / (double)q.nTwistFaces : 1.0;
    r.nTwistFaces = q.nTwistFaces; r.nLowTwistFaces = q.nLowTwistFaces; r.minTwistFace = q.minTwistFace;
    r.minTriangleTwist = q.minTriangleTwist; r.avgTriangleTwist = anyTw ? q.sumTriangleTwist / (double)q.nTwistFaces : 1.0;
    r.nLowTriangleTwistFaces = q.nLowTriangleTwistFaces; r.minTriangleTwistFace = q.minTriangleTwistFace;
    *out = r;
}
// one workgroup folds the slab (qFold) into the record of sums and denominators.  Out = smgpu_quality_motion_part: the per-rank
// record (nFaces is the counted one); Out = smgpu_quality_motion: the serial report
template <class Out>
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_final(const QMFace* __restrict__ fPart, int nFB, int nFaces, Out* __restrict__ out) {
    const QMFace a = qFold(fPart, nFB);
    if (threadIdx.x != 0) return;
    smgpu_quality_motion_part q;
    q.nFaces = nFaces;
    const bool anyFace = nFaces > 0, anyTw = a.nTw > 0;
    q.minTetQuality = anyFace ? a.minTet : 1.0; q.sumTetQuality = a.sumTet;
    q.nLowTetFaces = a.nLowTet; q.minTetFace = anyFace ? a.minTetId : -1;
    q.minBaseTetQuality = anyFace ? a.minBase : 1.0; q.nNoBasePointFaces = a.nNoBase; q.minBaseTetFace = anyFace ? a.minBaseId : -1;
    q.minTwist = anyTw ? a.minTw : 1.0; q.sumTwist = a.sumTw;
    q.nTwistFaces = a.nTw; q.nLowTwistFaces = a.nLowTw; q.minTwistFace = anyTw ? a.minTwId : -1;
    q.minTriangleTwist = anyTw ? a.minTri : 1.0; q.sumTriangleTwist = a.sumTri;
    q.nLowTriangleTwistFaces = a.nLowTri; q.minTriangleTwistFace = anyTw ? a.minTriId : -1;
    qFinish(q, out);
}

// ---- the findings as sets (smgpu_quality_motion_sets / _coupled_motion_sets, DESIGN.md "Mesh quality", 10.9) --------------------
// The flag pass of kernels_quality.hpp (qFlagPass) over the bodies above, with null field outputs: a record's count members become
// the mask bits.  Face sets only: k_quality_set_scan / _scatter<4, 0>.  nTw, the twist denominator, is no set.
constexpr int kQualityMotionFaceSets = 4;   // lowQualityTetFaces, noBasePointFaces, twistedFaces, lowTriangleTwistFaces
__device__ __forceinline__ unsigned qmFaceBits(const QMFace& e) {
    return (e.nLowTet ? 1u : 0u) | (e.nNoBase ? 2u : 0u) | (e.nLowTw ? 4u : 0u) | (e.nLowTri ? 8u : 0u);
}
// Coupled: C_N and `internal` of a face as k_quality_motion_faces_coupled selects them (its twin, keep alike); no bits where the
// neighbour rank counts the face
template <bool Coupled>
__global__ void __launch_bounds__(kQualityBlock) k_quality_motion_face_flags(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                              const double* __restrict__ cellCtr, const int* __restrict__ own,
                                                                              const int* __restrict__ nei, QCoupling<Coupled> cp,
                                                                              QualityMotionThresholds thr, uint8_t* __restrict__ mask,
                                                                              int* __restrict__ cnt) {
    qFlagPass<kQualityMotionFaceSets>(m.nFaces, mask, cnt, [&](int f) {
        QMFace e = qEmpty<QMFace>();
        if constexpr (Coupled) {
            const int sl = f < m.nInternalFaces ? -1 : cp.slot[f - m.nInternalFaces];
            const double* cnAt = f < m.nInternalFaces ? cellCtr + 3 * (size_t)nei[f]
                                                      : (sl >= 0 ? cp.recvCc + 3 * (size_t)(sl & kQualitySlotMask) : cellCtr + 3 * (size_t)own[f]);
            const bool internal = f < m.nInternalFaces || sl >= 0;
            const V3 CN = internal ? v3(cnAt[0], cnAt[1], cnAt[2]) : v3(0, 0, 0);
            qmFaceOneCoupled(m, pts, fCtr, ldv(cellCtr, own[f]), internal, CN, thr, f, e, nullptr, nullptr, nullptr, nullptr);
            if (sl >= 0 && (sl & kQualityNotCounted)) e = qEmpty<QMFace>();
        } else {
            qmFaceOne(m, pts, fCtr, cellCtr, own, nei, thr, f, e, nullptr, nullptr, nullptr, nullptr);
        }
        return qmFaceBits(e);
    });
}

}  // namespace smgpu
