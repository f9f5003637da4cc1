// What the patch-descriptor scores share (sgan_swd.hip, sgan_prd.hip): the descriptor geometry and the one normalisation both apply on
// load, so that the two files cannot drift apart.  DESIGN.md §R26, §R27.
#pragma once
#include "sgan_common.h"

#define SG_SWD_PATCH 7
#define SG_SWD_TAPS 49          // values of one channel of a descriptor
#define SG_SWD_MAX_N 16384

static inline int sg_swd_channels(int32_t K) { return (K == 49 || K == 98 || K == 147) ? K / SG_SWD_TAPS : 0; }

// mean and 1 / std of channel c from (sum, sum of squares, count) exactly as util.swd_stats_from_sums: no contraction anywhere
__device__ __forceinline__ void sg_swd_norm(const double* stats, int C, int c, double count, float& m32, float& r32) {
    const double mean = __ddiv_rn(stats[c], count);
    double var = __dsub_rn(__ddiv_rn(stats[C + c], count), __dmul_rn(mean, mean));
    if (!(var > 0.0)) var = 0.0;
    const double sd = __dsqrt_rn(var);
    m32 = (float)mean;
    r32 = sd == 0.0 ? 0.f : (float)__ddiv_rn(1.0, sd);
}

// util.swd_normalise_ref: float32(float32(x - m32) * r32)
__device__ __forceinline__ float sg_swd_normalise(float x, float m32, float r32) { return __fmul_rn(__fsub_rn(x, m32), r32); }
