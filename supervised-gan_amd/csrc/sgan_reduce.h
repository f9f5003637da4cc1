// What the loss kernels share (sgan_ew.hip, sgan_factd.hip, sgan_seghead.hip): the fp64 workgroup sum, the one cross-workgroup
// hand-off of the library outside the conv kernels, and the sigmoid / BCE arithmetic.  Device helpers, and the host's ceiling divide for the grids; DESIGN.md §R12.
#pragma once
#include "sgan_common.h"

static inline int sg_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float sg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// torch's BCELoss term: both logs clamped at -100
__device__ __forceinline__ float sg_bce_term(float p, float t) {
    const float lp = fmaxf(logf(p), -100.f);
    const float lq = fmaxf(log1pf(-p), -100.f);
    return -(t * lp + (1.f - t) * lq);
}

// torch's d BCE / d p = (p - t) / max((1 - p) p, 1e-12).  A caller that scales the numerator before it divides
// (w * (p - t) / den) takes the denominator alone: the order of the roundings is part of its result.
__device__ __forceinline__ float sg_bce_dden(float p) { return fmaxf((1.f - p) * p, 1e-12f); }
__device__ __forceinline__ float sg_bce_dterm(float p, float t) { return (p - t) / sg_bce_dden(p); }

// sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ double sg_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Sum over a workgroup of NW waves, in every thread, in a fixed order: (w0 + w1) + (w2 + w3) for four waves, 0 + w0 + w1 + ... for any
// other count.  `red`: NW doubles of LDS; a second call may reuse them only behind a barrier of the caller's.
template <int NW>
__device__ __forceinline__ double sg_block_sum(double acc, double* red) {
    acc = sg_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    SG_SYNC();
    if constexpr (NW == 4) {
        return (red[0] + red[1]) + (red[2] + red[3]);
    } else {
        double t = 0.0;
        for (int i = 0; i < NW; ++i) t += red[i];
        return t;
    }
}

// The hand-off.  Producer, every workgroup: thread 0 stores the workgroup's partial in its slot, fences (release: the slot is out
// before the ticket is taken) and takes a ticket.  True in every thread of the workgroup whose ticket was `expected`, the last to
// arrive: gridDim.x - 1, or BLOCKS * n - 1 on the (BLOCKS, n) grids.  Consumer, that workgroup: every thread that reads slots issues
// __threadfence() (acquire) and then reads them with sg_slot_load; whoever finishes stores 0 to the ticket for the next launch.
__device__ __forceinline__ bool sg_publish_last(double sum, double* slot, unsigned* ticket, unsigned expected, int* last_lds) {
    if (threadIdx.x == 0) {
        *slot = sum;
        __threadfence();
        *last_lds = atomicAdd(ticket, 1u) == expected;
    }
    SG_SYNC();
    return *last_lds != 0;
}

// another workgroup's slot, behind the consumer's fence: read at agent scope, never from a line this CU cached earlier
__device__ __forceinline__ double sg_slot_load(const double* slot) {
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Finish of the multi-term losses, run by the first wave of the last workgroup behind its fence: lane t < n sums the BLOCKS slots of
// term t in order, writes the mean to each[t] and weights it; the n <= 8 weighted means sit in lanes 0..7 and meet in a 3-step butterfly.
template <int BLOCKS>
__device__ __forceinline__ void sg_finish_terms(const double* part, bool has_term, double npix, float weight, float* each, float* total,
                                                unsigned* ticket) {
    const int t = threadIdx.x;
    double w = 0.0;
    if (has_term) {
        double sum = 0.0;
        for (int b = 0; b < BLOCKS; ++b) sum += sg_slot_load(&part[t * BLOCKS + b]);
        const float m = (float)(sum / npix);
        each[t] = m;
        w = (double)weight * (double)m;
    }
    for (int off = 4; off > 0; off >>= 1) w += __shfl_xor(w, off);
    if (t == 0) {
        total[0] = (float)w;
        ticket[0] = 0u;
    }
}
