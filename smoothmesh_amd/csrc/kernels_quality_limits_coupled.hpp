// kernels_quality_limits_coupled.hpp -- the tet, twist, weight, ratio and determinant limits of kernels_quality_limits.hpp on a
// sub-domain of a decomposed mesh (smgpu_set_quality_constraint_limits_coupled: include/smgpu.h, DESIGN.md "Mesh quality", 10.17).
//
// The coupled evaluation of kernels_quality_constraint.hpp (10.15) with, per evaluation,
//   first half, behind k_qc_tile (or the direct geometry kernels), in front of the packs:
//     a. k_qc_cells_more_coupled, queued only when minVolRatio or minDeterminant is on: k_qc_cells_more ungated, the determinant
//        over the cell's internal and processor faces (the constraint's own slot table).  The byte it leaves in cellFlag waits for
//        k_qc_cells of the second half, underDetNow for the host's read of QcDev there;
//     b. k_quality_pack_volumes (kernels_quality_geom.hpp) of the constraint's own volumes into sendVc, only when minVolRatio is on;
//   second half, behind the host's move of Cc and Vc:
//     c. k_qc_faces_more_coupled in the place of k_qc_faces_coupled whenever a new face criterion is on: a processor face takes
//        the internal branch of every criterion with C_N from recvCc and V_N from recvVc, flags its owner only, and counts only on
//        the counted side;
//   and on closing k_qc_close_full in the place of k_qc_close.
// The serial and the coupled kernels stay pairs: the serial ones are the functions whose resources 10.16 lists, and they are left
// as they were compiled.  Keep each pair alike.  No float atomics; every store is a plain vector store.
#pragma once
#include "kernels_quality_limits.hpp"

namespace smgpu {

// k_qc_cells_more on a sub-domain: its twin, line by line, without the gate, with qgcCounts (kernels_quality_geom.hpp) where it
// tests "f < nInternalFaces" -- without processor faces the same bits.  exemptOut != NULL (enabling): as k_qc_cells_more.
template <bool Det>
__global__ void __launch_bounds__(kQcBlock) k_qc_cells_more_coupled(MeshView m, const double* __restrict__ fCtr, const double* __restrict__ fArea,
                                                                     const int* __restrict__ slot, QcMore lim, double* __restrict__ vol,
                                                                     const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                                     uint8_t* __restrict__ cellFlag, QcDev* __restrict__ d) {
    const int c = blockIdx.x * kQcBlock + threadIdx.x;
    bool bad = false;
    if (c < m.nCells) {
        const int b = m.cfOff[c], e = m.cfOff[c + 1];
        V3 cEst = v3(0, 0, 0);
        for (int j = b; j < e; ++j) cEst = cEst + ldv(fCtr, m.cfVal[j] & 0x7fffffff);
        cEst = cEst / (double)(e - b);
        double pyr = 0.0, sumA = 0.0;
        int nInt = 0;
        for (int j = b; j < e; ++j) {
            const int ev = m.cfVal[j];
            const int f = ev & 0x7fffffff;
            const V3 Sf = ldv(fArea, f);
            double p = dot(Sf, ldv(fCtr, f) - cEst);
            if (ev < 0) p = -p;
            pyr += p;
            if (Det && qgcCounts(m, slot, f)) { sumA += mag(Sf); ++nInt; }
        }
        vol[c] = (1.0 / 3.0) * pyr;
        if constexpr (Det) {
            double det = 0.0;
            const double avgA = nInt > 0 ? sumA / (double)nInt : 0.0;
            if (nInt > 0 && avgA >= SMGPU_ROOTVSMALL) {
                double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
                for (int j = b; j < e; ++j) {
                    const int f = m.cfVal[j] & 0x7fffffff;
                    if (!qgcCounts(m, slot, f)) continue;
                    const V3 s = ldv(fArea, f) / avgA;
                    xx += s.x * s.x; xy += s.x * s.y; xz += s.x * s.z;
                    yy += s.y * s.y; yz += s.y * s.z; zz += s.z * s.z;
                }
                det = fabs((xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)) / 8.0;
            }
            bad = det < lim.minDet;
            if (exemptOut) exemptOut[c] = bad ? 1 : 0;
            else {
                bad = bad && !exempt[c];
                if (bad) cellFlag[c] = 1;
            }
        }
    }
    if constexpr (Det) {
        const int nBad = __syncthreads_count(bad ? 1 : 0);
        if (nBad > 0 && threadIdx.x == 0) atomicAdd(&d->underDetNow, nBad);
    }
}

// k_qc_faces_more on a sub-domain: its twin, line by line, without the gate.  The slot is decoded as k_qc_faces_coupled decodes
// it; `internal` is "internal face of the global mesh", `inner` "both cells are this rank's".  A processor face: C_N from recvCc,
// V_N from recvVc, the flag on its owner only, the counts only where the slot is counted.  Lanes of internal and physical faces
// take k_qc_faces_more's path.  exemptOut != NULL (enabling): as k_qc_faces_more.
template <bool Walk, bool Ratio>
__global__ void __launch_bounds__(kQcBlock) k_qc_faces_more_coupled(MeshView m, const double* __restrict__ pts, const double* __restrict__ fCtr,
                                                                     const double* __restrict__ fArea, const double* __restrict__ cellCtr,
                                                                     const double* __restrict__ vol, const int* __restrict__ own, const int* __restrict__ nei,
                                                                     const int* __restrict__ slot, const double* __restrict__ recvCc,
                                                                     const double* __restrict__ recvVc, QcLimits lim, QcMore more,
                                                                     const uint8_t* __restrict__ exempt, uint8_t* __restrict__ exemptOut,
                                                                     uint8_t* __restrict__ cellFlag, QcDev* __restrict__ d) {
    const int f = blockIdx.x * kQcBlock + threadIdx.x;
    bool badNO = false, badSk = false, badTet = false, badTw = false, badTri = false, badW = false, badR = false, counted = true;
    if (f < m.nFaces) {
        const bool inner = f < m.nInternalFaces;
        const int sl = inner ? -1 : slot[f - m.nInternalFaces];
        const bool internal = inner || sl >= 0;
        counted = sl < 0 || !(sl & kQualityNotCounted);
        const int o = own[f], n = inner ? nei[f] : 0;
        const V3 Cf = ldv(fCtr, f), Sf = ldv(fArea, f), CO = ldv(cellCtr, o);
        const V3 CN = inner ? ldv(cellCtr, n) : (sl >= 0 ? ldv(recvCc, sl & kQualitySlotMask) : v3(0, 0, 0));
        const double magSf = mag(Sf);
        const V3 Cpf = Cf - CO;
        V3 dd;
        double ortho = 1.0;
        if (internal) {
            dd = CN - CO;
            ortho = dot(dd, Sf) / (mag(dd) * magSf + SMGPU_VSMALL);
        } else {
            const V3 nb = Sf / (magSf + SMGPU_ROOTVSMALL);
            dd = dot(nb, Cpf) * nb;
        }
        const V3 sv = Cpf - (dot(Sf, Cpf) / (dot(Sf, dd) + SMGPU_ROOTVSMALL)) * dd;
        const double magSv = mag(sv);
        const V3 sHat = sv / (magSv + SMGPU_ROOTVSMALL);
        double fd = 0.2 * mag(dd) + SMGPU_ROOTVSMALL;
        const int jb = m.faceOff[f], nv = m.faceOff[f + 1] - jb;
        if constexpr (Walk) {
            const bool summed = nv > 3;
            double tet = __builtin_inf(), tw = __builtin_inf(), tri = __builtin_inf();
            int nValid = 0;
            if (nv > 0) {
                const V3 dv = sel3(internal, CN, Cf) - CO;
                const V3 nHat = dv / (mag(dv) + SMGPU_VSMALL);
                const V3 p0 = ldv(pts, m.facePts[jb]);
                V3 cur = p0, hFirst = v3(0, 0, 0), hPrev = v3(0, 0, 0);
                for (int i = 0; i < nv; ++i) {
                    fd = fmax(fd, fabs(dot(sHat, cur - Cf)));
                    const V3 nxt = (i + 1 < nv) ? ldv(pts, m.facePts[jb + i + 1]) : p0;
                    const V3 u = nxt - cur, v = Cf - cur;
                    tet = fmin(tet, qmTetPair(cur, u, v, CO, internal, CN, more.k));
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
            if (nValid < 1) tw = 1.0;
            if (nValid < 2) tri = 1.0;
            badTet = more.tetOn && tet < more.minTet;
            badTw = summed && more.twistOn && tw < more.minTwist;
            badTri = summed && more.triOn && tri < more.minTri;
        } else {
            for (int j = jb; j < jb + nv; ++j) fd = fmax(fd, fabs(dot(sHat, ldv(pts, m.facePts[j]) - Cf)));
        }
        const double skew = magSv / fd;
        badNO = internal && lim.nonOrthoOn && ortho < lim.cosT;
        badSk = internal ? (lim.internalSkewOn && skew > lim.maxInternalSkew) : (lim.boundarySkewOn && skew > lim.maxBoundarySkew);
        if (internal) {
            const double dO = fabs(dot(Sf, Cpf)), dN = fabs(dot(Sf, CN - Cf));
            const double w = fmin(dO, dN) / ((dO + dN) + SMGPU_VSMALL);
            badW = more.weightOn && w < more.minWeight;
            if constexpr (Ratio) {
                const double vO = vol[o], vN = inner ? vol[n] : recvVc[sl & kQualitySlotMask];
                const double r = fmin(vO, vN) / (fmax(vO, vN) + SMGPU_VSMALL);
                badR = more.ratioOn && r < more.minRatio;
            }
        }
        const bool any = badNO || badSk || badTet || badTw || badTri || badW || badR;
        if (exemptOut) exemptOut[f] = any ? 1 : 0;
        else if (exempt[f]) badNO = badSk = badTet = badTw = badTri = badW = badR = false;
        else if (any) {
            cellFlag[o] = 1;
            if (inner) cellFlag[n] = 1;
        }
    }
    const bool any = badNO || badSk || badTet || badTw || badTri || badW || badR;
    const int nNO = __syncthreads_count((badNO && counted) ? 1 : 0), nSk = __syncthreads_count((badSk && counted) ? 1 : 0),
              nAny = __syncthreads_count((any && counted) ? 1 : 0);
    int nTet = 0, nTw = 0, nTri = 0, nW = 0, nR = 0;
    if (Walk && more.tetOn) nTet = __syncthreads_count((badTet && counted) ? 1 : 0);
    if (Walk && more.twistOn) nTw = __syncthreads_count((badTw && counted) ? 1 : 0);
    if (Walk && more.triOn) nTri = __syncthreads_count((badTri && counted) ? 1 : 0);
    if (more.weightOn) nW = __syncthreads_count((badW && counted) ? 1 : 0);
    if (Ratio && more.ratioOn) nR = __syncthreads_count((badR && counted) ? 1 : 0);
    if (threadIdx.x == 0) {
        if (nNO > 0) atomicAdd(&d->nonOrthoNow, nNO);
        if (nSk > 0) atomicAdd(&d->skewNow, nSk);
        if (nAny > 0) atomicAdd(&d->facesNow, nAny);
        if (nTet > 0) atomicAdd(&d->lowTetNow, nTet);
        if (nTw > 0) atomicAdd(&d->lowTwistNow, nTw);
        if (nTri > 0) atomicAdd(&d->lowTriNow, nTri);
        if (nW > 0) atomicAdd(&d->lowWeightNow, nW);
        if (nR > 0) atomicAdd(&d->lowRatioNow, nR);
    }
}

// k_qc_close's twin with the wider record: n, the rank's ten counts at k = 0 in the record's order from nBadCells on, without
// nPointsReverted (the applies': the slot was zeroed before the iteration's first pass).  One wave, lane 0, plain C++.
struct QcCounts { long long n[10]; };
__global__ void __launch_bounds__(64) k_qc_close_full(smgpu_quality_constraint_record_full* __restrict__ rec, long long number, int passes, int fullRevert,
                                                       QcCounts c) {
    if (threadIdx.x != 0) return;
    rec->iteration = number;
    rec->passes = passes;
    rec->fullRevert = fullRevert;
    rec->nBadCells = c.n[0];
    rec->nTangledCells = c.n[1];
    rec->nNonOrthoFaces = c.n[2];
    rec->nSkewFaces = c.n[3];
    rec->nLowTetFaces = c.n[4];
    rec->nLowTwistFaces = c.n[5];
    rec->nLowTriangleTwistFaces = c.n[6];
    rec->nLowWeightFaces = c.n[7];
    rec->nLowVolRatioFaces = c.n[8];
    rec->nUnderdeterminedCells = c.n[9];
}

}  // namespace smgpu
