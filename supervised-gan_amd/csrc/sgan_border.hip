// The border term of the U-Net loss on the device (include/sgan_hip.h, "border weight"): for every wall pixel of a label map in
// sgan_ccl_label's form the squared distances to the nearest and to the second-nearest DISTINCT cell within a radius R, and from them
//     bmap(p) = w0 exp(-(d1 + d2)^2 / (2 sigma^2)).
// The distances are exact integers and do not depend on the order candidates are met in, so the planes repeat to the bit.
//
// One launch whose grid depends on (H, W) and whose LDS on R.  A workgroup of 256 threads owns a 32 x 32 core and holds the labels of
// the core and an R-pixel halo in LDS ((32 + 2 R)^2 int32, 36 KB at R = 32; outside the image = wall).  A thread takes four core
// pixels, 8 rows apart, so each 32-lane half of a wave holds one row of 32 consecutive pixels: a 4-byte LDS read is banked per half
// (32 banks), so the 32 consecutive dwords a half reads for one offset are conflict-free whatever the row stride.  Only wall
// pixels search: the rows of the disc in the order dy = 0, -1, +1, -2, +2, ..., every column of a row.  A candidate (d, L) meets the
// running pair (l1, d1), (l2, d2) of distinct labels, d1 <= d2:
//     L == l1: d1 = min(d1, d);   L == l2: d2 = min(d2, d), then the two swap if d2 < d1;   any other L is inserted where it sorts.
// A label that was pushed out of the pair comes back only with a smaller d, which is inserted like any other, so the pair ends as the
// two smallest per-label minima.  A row |dy| holds only d >= dy^2; once dy^2 > d2 in every searching lane of the wave no later row
// can change a pair, and the wave leaves the loop (one ballot per |dy|) -- on a cell map with thin walls after a few rows.
#include "sgan_common.h"

#define SG_BW_CORE 32
#define SG_BW_THREADS 256
#define SG_BW_MAX_R 32
#define SG_BW_ERR_LABELS 4      // a label < 0: the bit the other metric kernels raise for a label out of range
#define SG_BW_NONE 0x7fffffff

__global__ __launch_bounds__(SG_BW_THREADS) void sg_border_weight_kernel(const int32_t* __restrict__ L, int H, int W, int R, float w0, float sigma,
                                                                         int tiles_x, float* __restrict__ bmap, int32_t* __restrict__ d1sq,
                                                                         int32_t* __restrict__ d2sq, int32_t* dev_err) {
    extern __shared__ int32_t T[];      // (32 + 2 R)^2 labels, row stride S
    const int S = SG_BW_CORE + 2 * R;
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % tiles_x) * SG_BW_CORE, y0 = (int)(blockIdx.x / tiles_x) * SG_BW_CORE;
    bool bad = false;
    for (int p = tid; p < S * S; p += SG_BW_THREADS) {
        const int y = y0 - R + p / S, x = x0 - R + p % S;
        int32_t v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) v = L[(int64_t)y * W + x];
        if (v < 0) {
            bad = true;
            v = 0;
        }
        T[p] = v;
    }
    if (bad && dev_err) __hip_atomic_fetch_or(dev_err, SG_BW_ERR_LABELS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SG_SYNC();      // the core and its halo are in place; nothing writes T after this

    const int lx = tid % SG_BW_CORE;
    for (int k = 0; k < SG_BW_CORE * SG_BW_CORE / SG_BW_THREADS; ++k) {
        const int ly = tid / SG_BW_CORE + k * (SG_BW_THREADS / SG_BW_CORE);
        const int y = y0 + ly, x = x0 + lx;
        const bool inside = y < H && x < W;
        const int c = (ly + R) * S + lx + R;      // this pixel in T
        const bool wall = inside && T[c] == 0;
        int l1 = 0, l2 = 0, d1 = SG_BW_NONE, d2 = SG_BW_NONE;
        for (int a = 0; a <= R; ++a) {
            if (__ballot(wall && a * a <= d2) == 0ull) break;      // uniform over the wave
            if (!wall) continue;
            const int rem = R * R - a * a;
            int hw = (int)sqrtf((float)rem);      // floor(sqrt(rem)), corrected in integers
            while (hw * hw > rem) --hw;
            while ((hw + 1) * (hw + 1) <= rem) ++hw;
            for (int s = (a ? 0 : 1); s < 2; ++s) {
                const int row = c + (s ? a : -a) * S;
                for (int dx = -hw; dx <= hw; ++dx) {
                    const int lab = T[row + dx];
                    if (lab == 0) continue;
                    const int d = a * a + dx * dx;
                    if (lab == l1) {
                        d1 = d < d1 ? d : d1;
                    } else if (lab == l2) {
                        d2 = d < d2 ? d : d2;
                        if (d2 < d1) {
                            const int tl = l1, td = d1;
                            l1 = l2; d1 = d2;
                            l2 = tl; d2 = td;
                        }
                    } else if (d < d1) {
                        l2 = l1; d2 = d1;
                        l1 = lab; d1 = d;
                    } else if (d < d2) {
                        l2 = lab; d2 = d;
                    }
                }
            }
        }
        if (!inside) continue;
        const int64_t i = (int64_t)y * W + x;
        float b = 0.f;
        if (d2 != SG_BW_NONE) {      // two cells in range (d1 <= d2)
            const float sum = sqrtf((float)d1) + sqrtf((float)d2);
            b = w0 * expf(-(sum * sum) / (2.f * sigma * sigma));
        }
        bmap[i] = b;
        if (d1sq) d1sq[i] = d1 != SG_BW_NONE ? d1 : -1;
        if (d2sq) d2sq[i] = d2 != SG_BW_NONE ? d2 : -1;
    }
}

extern "C" int sgan_border_weight(const int32_t* labels, int32_t H, int32_t W, int32_t radius, float w0, float sigma, float* bmap,
                                  int32_t* d1sq, int32_t* d2sq, int32_t* dev_err, void* stream) {
    if (!labels || !bmap || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30) || radius < 1 || radius > SG_BW_MAX_R || !(sigma > 0.f)) return 1;
    const int tiles_x = (W + SG_BW_CORE - 1) / SG_BW_CORE, tiles_y = (H + SG_BW_CORE - 1) / SG_BW_CORE;      // tiles_x tiles_y < 2^21 + 2^26
    const int S = SG_BW_CORE + 2 * radius;
    hipLaunchKernelGGL(sg_border_weight_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(SG_BW_THREADS), (size_t)S * S * sizeof(int32_t),
                       (hipStream_t)stream, labels, H, W, radius, w0, sigma, tiles_x, bmap, d1sq, d2sq, dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_border_weight_kernel";
    return SGAN_OK;
}
