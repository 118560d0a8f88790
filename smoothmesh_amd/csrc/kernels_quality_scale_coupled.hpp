// kernels_quality_scale_coupled.hpp -- the scaling passes of the quality constraint on a sub-domain of a decomposed mesh
// (smgpu_set_quality_constraint_scaling_coupled: include/smgpu.h, DESIGN.md "Mesh quality", 10.20).  10.19's scale field, with the
// one thing that crosses the ranks: the sweep of a SHARED point runs over its neighbours in the whole mesh, of which a rank's
// pointPoints row holds a part.  The host drives the passes (10.15), so nothing here is gated: k_qs_keep, k_qs_mark and k_qs_sweep
// (kernels_quality_scale.hpp) are launched as they are, with gate = NULL and the constraint's device words, whose clean word the
// coupled form leaves 0.  New here:
//   k_qsc_open      in front of every pass_end that changes points: the three counts of the accepted state start over (the serial
//                   form's k_qs_verdict does it);
//   k_qsc_partial   one lane per shared point and trip (grids capped as 10.19's): the left fold from 0.0 of the current field over
//                   the COUNTED entries of its row, in row order, into the constraint's own `part` and into the point's send
//                   slots (exchange S, one double per slot; the slots as k_halo_packA finds them: sendOff / sendSlots);
//   k_qsc_combine   one lane per shared point and trip, behind the all-points k_qs_sweep of the same sweep and behind the host's move of
//                   S: the left fold from 0.0 of the sharers' partial sums in ascending rank (combSlots, -1 this rank), one
//                   division by the point's degree in the whole mesh, 10.19's min rule on the OLD field, the store into the NEW
//                   one at the point -- it replaces what k_qs_sweep left there from the rank's row alone;
//   k_qsc_apply     k_qs_apply's body; nPointsReverted and nPointsScaled take a shared point on its master only (10.13's
//                   counted mask), minScale is the rank's own minimum;
//   k_qsc_close     k_qc_close's twin for the scaled record (keep them alike).
// Every sharer folds the same values in the same order, so the copies of a shared point's scale stay bit-identical.  No float
// atomics; every store is a plain vector store.
#pragma once
#include "kernels_quality_scale.hpp"

namespace smgpu {

__global__ void __launch_bounds__(64) k_qsc_open(smgpu_quality_constraint_record_scaled* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    rec->nPointsReverted = 0; rec->nPointsScaled = 0; rec->minScale = 1.0;
}

// rowOff: nShared + 1; rowPt: local ids of the counted neighbours.  A point without a send slot (none exists: every shared point
// has a sharer) stores its part only.
__global__ void __launch_bounds__(kQsBlock) k_qsc_partial(int nShared, const int* __restrict__ rowOff, const int* __restrict__ rowPt,
                                                           const double* __restrict__ in, double* __restrict__ part, const int* __restrict__ sendOff,
                                                           const int* __restrict__ sendSlots, double* __restrict__ sendS) {
    for (long long i = (long long)blockIdx.x * kQsBlock + threadIdx.x; i < nShared; i += (long long)gridDim.x * kQsBlock) {
        double sum = 0.0;
        for (int k = rowOff[i]; k < rowOff[i + 1]; ++k) sum += in[rowPt[k]];
        part[i] = sum;
        for (int k = sendOff[i]; k < sendOff[i + 1]; ++k) sendS[sendSlots[k]] = sum;
    }
}

// in: the field the sweep reads; out: the field it writes (never the same).  deg == 0 (a shared point without an edge anywhere):
// the value is kept, as 10.19 keeps that of an empty row.
__global__ void __launch_bounds__(kQsBlock) k_qsc_combine(int nShared, const int* __restrict__ sharedLocal, const int* __restrict__ combOff,
                                                           const int* __restrict__ combSlots, const double* __restrict__ part, const double* __restrict__ recvS,
                                                           const int* __restrict__ sharedDeg, const double* __restrict__ in, double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * kQsBlock + threadIdx.x; i < nShared; i += (long long)gridDim.x * kQsBlock) {
        const int p = sharedLocal[i], deg = sharedDeg[i];
        const double s = in[p];
        double v = s;
        if (deg > 0) {
            double sum = 0.0;
            for (int k = combOff[i]; k < combOff[i + 1]; ++k) {
                const int sl = combSlots[k];
                sum += sl < 0 ? part[i] : recvS[sl];
            }
            const double t = 0.5 * s + 0.5 * (sum / (double)deg);
            v = t < s ? t : s;
        }
        out[p] = v;
    }
}

// k_qs_apply with master-only counting (keep the bodies alike): sharedSlot[p] >= 0 names the point's entry of `counted` (one byte
// per shared point, 0 where a lower rank shares it), as k_tangle_apply_counted reads them
__global__ void __launch_bounds__(kQsBlock) k_qsc_apply(const double* __restrict__ x, const double* __restrict__ L, double* __restrict__ cur,
                                                         const double* __restrict__ scale, int nPoints, const int* __restrict__ sharedSlot,
                                                         const uint8_t* __restrict__ counted, smgpu_quality_constraint_record_scaled* __restrict__ rec) {
    const int tid = threadIdx.x;
    int reverted = 0, scaled = 0;
    unsigned long long minBits = kQsOneBits;
    for (long long p = (long long)blockIdx.x * kQsBlock + tid; p < nPoints; p += (long long)gridDim.x * kQsBlock) {
        const double s = scale[p];
        if (s < 1.0) {
            const V3 a = ldv(x, p), l = ldv(L, p);
            const V3 v = (s == 0.0) ? a : v3(a.x + s * (l.x - a.x), a.y + s * (l.y - a.y), a.z + s * (l.z - a.z));
            stv(cur, p, v);
            const int sl = sharedSlot ? sharedSlot[p] : -1;
            const bool moved = (l.x != a.x || l.y != a.y || l.z != a.z) && (sl < 0 || counted[sl]);
            reverted += (moved && v.x == a.x && v.y == a.y && v.z == a.z) ? 1 : 0;
            scaled += (moved && s > 0.0) ? 1 : 0;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
            minBits = bits < minBits ? bits : minBits;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        reverted += __shfl_xor(reverted, o, 64);
        scaled += __shfl_xor(scaled, o, 64);
        const unsigned long long other = __shfl_xor(minBits, o, 64);
        minBits = other < minBits ? other : minBits;
    }
    __shared__ int waveReverted[kQsBlock / 64], waveScaled[kQsBlock / 64];
    __shared__ unsigned long long waveMin[kQsBlock / 64];
    if ((tid & 63) == 0) { waveReverted[tid >> 6] = reverted; waveScaled[tid >> 6] = scaled; waveMin[tid >> 6] = minBits; }
    __syncthreads();
    if (tid == 0) {
        int nR = 0, nS = 0;
        unsigned long long mn = kQsOneBits;
        for (int w = 0; w < kQsBlock / 64; ++w) { nR += waveReverted[w]; nS += waveScaled[w]; mn = waveMin[w] < mn ? waveMin[w] : mn; }
        if (nR > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsReverted), (unsigned long long)nR);
        if (nS > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nPointsScaled), (unsigned long long)nS);
        if (mn < kQsOneBits) atomicMin(reinterpret_cast<unsigned long long*>(&rec->minScale), mn);
    }
}

// k_qc_close's twin: the head through the same words, then the marked passes that scaled; an iteration without a marked pass has
// minScale 1.0 (the slot was zeroed), every other one what the last k_qsc_apply left
__global__ void __launch_bounds__(64) k_qsc_close(smgpu_quality_constraint_record_scaled* __restrict__ rec, long long number, int passes, int fullRevert,
                                                   QcCounts c, int nScalePasses, int clean) {
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
    rec->nConcaveFaces = c.n[10];
    rec->nWarpedFaces = c.n[11];
    rec->nSmallAreaFaces = c.n[12];
    rec->nSmallVolumeCells = c.n[13];
    rec->nScalePasses = nScalePasses;
    if (clean) rec->minScale = 1.0;
}

}  // namespace smgpu
