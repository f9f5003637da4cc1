// The exact squared Euclidean distance transform of a wall map and the boundary scores built on it (include/sgan_hip.h, "boundary
// scores").  dsq(y, x) = min over the wall pixels (y', x') of (y - y')^2 + (x - x')^2, an exact int32 that does not
// depend on the order candidates are met in, so the plane repeats to the bit.
//
// The separable algorithm.  Pass 1 finds, per column, the vertical distance g(y, x) to the nearest wall pixel of the column; pass 2
// takes, per row, dsq(y, x) = min over x' of (x - x')^2 + g(y, x')^2.
//
// Pass 1 is two launches over (column, segment of 32 rows); a thread owns one column of one segment, so loads and stores are
// coalesced across x and there are W H / 32 threads, not W.
//   mask:   the wall bits of the 32 rows as one uint32 per (segment, column), and the number of wall pixels added to a counter.
//   column: the carry -- the nearest wall row above the segment and the nearest below it -- is looked up in the masks of the other
//           segments, nearest first, until one is nonzero (at most H / 32 loads each way, one or two on a map with walls in every
//           segment); inside the segment the nearest wall row at or above / at or below row r comes from the segment's own mask with
//           a clz / ctz.  Writes g^2, or -1 where the column has no wall.
// Pass 2: a workgroup owns one row and stages g^2 in LDS in chunks of SG_EDT_CHUNK columns.  A thread owns one pixel of a tile of
// 256 and scans outward from its own x, r = 0, 1, 2, ...; it stops as soon as r^2 >= its best so far, which is exact because every
// later candidate is at least r^2.  A row longer than a chunk is walked in chunks, the tile's own first and then its neighbours
// nearest first; a chunk that no thread of the workgroup can still improve from (distance to the chunk squared >= best) is neither
// staged nor scanned.  Consecutive lanes read consecutive dwords of LDS, so the reads are conflict-free.
// The plane without a wall pixel: the counter is 0, the column launch returns at once and the row launch writes -1.
// Workspace: [counter: 16 bytes][masks: ceil(H / 32) W uint32, rounded up to 16 bytes][g^2: H W int32].
#include "sgan_common.h"
#include "sgan_reduce.h"

#define SG_EDT_SEG 32            // rows per segment: one mask word
#define SG_EDT_THREADS 256
#define SG_EDT_CHUNK 2048        // columns of g^2 staged at once (8 KB of LDS)
#define SG_EDT_MAX_DIM 32768
#define SG_EDT_INF 0x7fffffff    // above every distance: (H - 1)^2 + (W - 1)^2 <= 2 * 32767^2 < 2^31 - 1
static_assert(SG_EDT_CHUNK % SG_EDT_THREADS == 0, "a tile of 256 pixels lies in one chunk");

// a refused call: the reason goes to sgan_last_error, the entry returns 1 and has launched nothing
#define SG_REFUSE(cond, ...)                            \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

__global__ void sg_edt_zero_kernel(unsigned* counter) {
    if (blockIdx.x == 0 && threadIdx.x < 4) counter[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(SG_EDT_THREADS) void sg_edt_mask_kernel(const float* __restrict__ plane, int64_t pix_stride, int H, int W,
                                                                     unsigned* __restrict__ masks, unsigned* counter) {
    const int x = blockIdx.x * SG_EDT_THREADS + threadIdx.x, seg = blockIdx.y;
    unsigned m = 0u;
    if (x < W) {
        const int y0 = seg * SG_EDT_SEG, rows = H - y0 < SG_EDT_SEG ? H - y0 : SG_EDT_SEG;
        for (int r = 0; r < rows; ++r)
            if (plane[((int64_t)(y0 + r) * W + x) * pix_stride] > 0.5f) m |= 1u << r;      // a NaN and an exact 0.5 are not wall
        masks[(int64_t)seg * W + x] = m;
    }
    int n = __builtin_popcount(m);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (unsigned)n);
}

__global__ __launch_bounds__(SG_EDT_THREADS) void sg_edt_column_kernel(const unsigned* __restrict__ masks, const unsigned* __restrict__ counter,
                                                                       int H, int W, int nseg, int32_t* __restrict__ gsq) {
    if (counter[0] == 0u) return;      // no wall anywhere (uniform over the grid): the row launch writes -1 without reading g^2
    const int x = blockIdx.x * SG_EDT_THREADS + threadIdx.x, seg = blockIdx.y;
    if (x >= W) return;
    const unsigned m = masks[(int64_t)seg * W + x];
    int up = -1, down = -1;      // the nearest wall row above / below the segment, -1 = none
    for (int s = seg - 1; s >= 0; --s) {
        const unsigned mm = masks[(int64_t)s * W + x];
        if (mm) {
            up = s * SG_EDT_SEG + 31 - __builtin_clz(mm);
            break;
        }
    }
    for (int s = seg + 1; s < nseg; ++s) {
        const unsigned mm = masks[(int64_t)s * W + x];
        if (mm) {
            down = s * SG_EDT_SEG + __builtin_ctz(mm);
            break;
        }
    }
    const int y0 = seg * SG_EDT_SEG, rows = H - y0 < SG_EDT_SEG ? H - y0 : SG_EDT_SEG;
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const unsigned lo = m & (0xffffffffu >> (31 - r)), hi = m >> r;      // the segment's wall rows <= r, and >= r shifted down by r
        const int yu = lo ? y0 + 31 - __builtin_clz(lo) : up;
        const int yd = hi ? y + __builtin_ctz(hi) : down;
        int g = -1;
        if (yu >= 0) g = y - yu;
        if (yd >= 0 && (g < 0 || yd - y < g)) g = yd - y;
        gsq[(int64_t)y * W + x] = g < 0 ? -1 : g * g;      // g <= 32767
    }
}

__global__ __launch_bounds__(SG_EDT_THREADS) void sg_edt_row_kernel(const int32_t* __restrict__ gsq, const unsigned* __restrict__ counter, int W,
                                                                    int32_t* __restrict__ dsq) {
    __shared__ int32_t G[SG_EDT_CHUNK];
    __shared__ int any[3];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * W;
    if (counter[0] == 0u) {      // uniform over the grid
        for (int x = tid; x < W; x += SG_EDT_THREADS) dsq[row + x] = -1;
        return;
    }
    if (tid < 3) any[tid] = 0;
    SG_SYNC();      // any[] zero
    const int nchunks = (W + SG_EDT_CHUNK - 1) / SG_EDT_CHUNK, ntiles = (W + SG_EDT_THREADS - 1) / SG_EDT_THREADS;
    int staged = -1, it = 0;      // the chunk in G; the visits so far: both the same in every thread
    for (int t = 0; t < ntiles; ++t) {
        const int x = t * SG_EDT_THREADS + tid;
        const bool valid = x < W;
        const int home = t * SG_EDT_THREADS / SG_EDT_CHUNK;
        int best = SG_EDT_INF;
        for (int k = 0; k < 2 * nchunks - 1; ++k) {      // home, home - 1, home + 1, home - 2, ...
            const int c = home + ((k & 1) ? -((k + 1) >> 1) : (k >> 1));
            if (c < 0 || c >= nchunks) continue;
            const int lo = c * SG_EDT_CHUNK, hi = lo + SG_EDT_CHUNK < W ? lo + SG_EDT_CHUNK : W;
            const int dmin = x < lo ? lo - x : (x >= hi ? x - (hi - 1) : 0);      // <= 32767 wherever valid
            const bool need = valid && dmin * dmin < best;
            // One barrier decides for the workgroup whether anybody still needs this chunk.  Visit `it` uses any[it % 3]; thread 0
            // clears the next visit's slot, which was last read two visits ago, behind the barrier of the visit before this one.
            if (tid == 0) any[(it + 1) % 3] = 0;
            if (need) any[it % 3] = 1;
            SG_SYNC();      // any[it % 3] complete; every thread has left the scan of the chunk that is in G
            const bool go = any[it % 3] != 0;
            ++it;
            if (!go) continue;
            if (staged != c) {
                for (int i = tid; i < hi - lo; i += SG_EDT_THREADS) G[i] = gsq[row + lo + i];
                SG_SYNC();      // the chunk is in G
                staged = c;
            }
            if (!need) continue;
            const int rmax = (x - lo > hi - 1 - x) ? x - lo : hi - 1 - x;
            for (int r = dmin; r <= rmax; ++r) {
                const int rr = r * r;
                if (rr >= best) break;      // every later candidate is at least r^2
                const int xl = x - r, xr = x + r;
                if (xl >= lo && xl < hi) {
                    const int v = G[xl - lo];
                    if (v >= 0 && rr + v < best) best = rr + v;
                }
                if (r > 0 && xr >= lo && xr < hi) {
                    const int v = G[xr - lo];
                    if (v >= 0 && rr + v < best) best = rr + v;
                }
            }
        }
        if (valid) dsq[row + x] = best;      // the plane has a wall pixel, so its column gave every row a candidate
    }
}

struct SgEdtLayout {
    int nseg;
    int64_t mask_bytes, bytes;
};

static bool sg_edt_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= SG_EDT_MAX_DIM && W <= SG_EDT_MAX_DIM && (int64_t)H * W < (1ll << 30);
}

static SgEdtLayout sg_edt_layout(int32_t H, int32_t W) {
    SgEdtLayout l;
    l.nseg = (H + SG_EDT_SEG - 1) / SG_EDT_SEG;
    l.mask_bytes = (4ll * l.nseg * W + 15) & ~15ll;
    l.bytes = 16 + l.mask_bytes + 4ll * H * W;
    return l;
}

extern "C" int64_t sgan_edt_workspace(int32_t H, int32_t W) {
    if (!sg_edt_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_edt_layout(H, W).bytes;
}

extern "C" int sgan_edt_sq(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* dsq, void* workspace, int64_t workspace_bytes,
                           int32_t* dev_err, void* stream) {
    SG_REFUSE(plane && dsq && workspace && dev_err, "null pointer");
    SG_REFUSE(sg_edt_shape_ok(H, W) && pix_stride >= 1, "bad shape %d x %d (H, W <= %d, H W < 2^30), pixel stride %lld", H, W, SG_EDT_MAX_DIM,
               (long long)pix_stride);
    const SgEdtLayout l = sg_edt_layout(H, W);
    SG_REFUSE(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_edt_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)l.bytes, H, W);
    SG_REFUSE(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    unsigned* counter = (unsigned*)workspace;
    unsigned* masks = (unsigned*)((char*)workspace + 16);
    int32_t* gsq = (int32_t*)((char*)workspace + 16 + l.mask_bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 cols((W + SG_EDT_THREADS - 1) / SG_EDT_THREADS, l.nseg);      // <= 128 x 1024
    hipLaunchKernelGGL(sg_edt_zero_kernel, dim3(1), dim3(64), 0, st, counter);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_edt_mask_kernel, cols, dim3(SG_EDT_THREADS), 0, st, plane, pix_stride, H, W, masks, counter);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_edt_column_kernel, cols, dim3(SG_EDT_THREADS), 0, st, (const unsigned*)masks, (const unsigned*)counter, H, W, l.nseg, gsq);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_edt_row_kernel, dim3(H), dim3(SG_EDT_THREADS), 0, st, (const int32_t*)gsq, (const unsigned*)counter, W, dsq);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_edt_row_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The counts behind BoundF, HausD and ASSD from two distance transforms.  Two launches whose grids depend on (H, W) only.
//   count: a grid-stride pass; a workgroup gathers its histograms and counters in LDS, its two fp64 sums with sg_block_sum, and
//          stores them in a slot of its own in the workspace -- no atomics in global memory and nothing to zero.
//   final: one workgroup adds entry k of the slots in a fixed order (a max for the two maxima), so the fp64 sums repeat to the bit
//          too; it then decides "Hausdorff defined", adds to the accumulators and writes the optional outputs.
// Workspace: SG_BND_BLOCKS slots of SG_BND_SLOT 8-byte entries: [0 .. 71] int64 as acc_i[0 .. 71], [72], [73] double as acc_f[0], [1].
// ------------------------------------------------------------------------------------------------------------------------------
#define SG_BND_BLOCKS 512
#define SG_BND_INTS 72
#define SG_BND_SLOT 74
#define SG_BND_FAR 900      // 30^2: above it, bin 31

// ceil(sqrt(d)) for 0 <= d <= 900 in integers, 31 for d > 900 and for d < 0 (the other map has no wall)
__device__ __forceinline__ int sg_bnd_bin(int d) {
    if (d < 0 || d > SG_BND_FAR) return SGAN_BND_BINS - 1;
    int k = (int)sqrtf((float)d);
    while (k * k < d) ++k;
    while (k > 0 && (k - 1) * (k - 1) >= d) --k;
    return k;
}

__global__ __launch_bounds__(256) void sg_bnd_count_kernel(const int32_t* __restrict__ t_dsq, const int32_t* __restrict__ s_dsq, int64_t n,
                                                           int64_t* __restrict__ slots) {
    __shared__ int part[SG_BND_INTS];
    __shared__ double red[2][4];
    for (int k = threadIdx.x; k < SG_BND_INTS; k += 256) part[k] = 0;
    SG_SYNC();      // part[] zero
    int cnt[2] = {0, 0}, def[2] = {0, 0}, far[2] = {0, 0};      // side 0: the prediction's wall pixels, side 1: the truth's
    double sum[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int t = t_dsq[i], s = s_dsq[i];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            if ((side ? t : s) != 0) continue;      // not a wall pixel of this side's map
            const int d = side ? s : t;             // its distance^2 to the other map
            ++cnt[side];
            atomicAdd(&part[side * SGAN_BND_BINS + sg_bnd_bin(d)], 1);
            if (d >= 0) {
                ++def[side];
                sum[side] += sqrt((double)d);
                far[side] = d > far[side] ? d : far[side];
            }
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        if (cnt[side]) atomicAdd(&part[64 + side], cnt[side]);
        if (def[side]) atomicAdd(&part[68 + side], def[side]);
        if (far[side]) atomicMax(&part[70 + side], far[side]);
    }
    const double s0 = sg_block_sum<4>(sum[0], red[0]);      // its barrier covers part[] as well
    const double s1 = sg_block_sum<4>(sum[1], red[1]);
    int64_t* slot = slots + (int64_t)blockIdx.x * SG_BND_SLOT;
    if (threadIdx.x < SG_BND_INTS) slot[threadIdx.x] = part[threadIdx.x];
    if (threadIdx.x == 0) {
        ((double*)slot)[72] = s0;
        ((double*)slot)[73] = s1;
    }
}

// One workgroup of SG_BND_GROUPS x 128 threads.  Thread (group g, entry k) combines entry k of the g-th run of consecutive slots,
// eight loads in flight at a time (one after the other, 512 dependent round trips to memory took 190 us); the groups' partial
// results meet in LDS in group order.  Every count is >= 0, so 0 stands for a slot past the end in the sums and the maxima alike.
#define SG_BND_GROUPS 8
__global__ __launch_bounds__(SG_BND_GROUPS * 128) void sg_bnd_final_kernel(const int64_t* __restrict__ slots, int nslots, int64_t* acc_i,
                                                                           double* acc_f, int64_t* counts_out, double* sums_out) {
    __shared__ int64_t ipart[SG_BND_GROUPS][SG_BND_INTS];
    __shared__ double fpart[SG_BND_GROUPS][2];
    __shared__ int64_t tot[SGAN_BND_COUNTS];
    __shared__ double ftot[2];
    const int k = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int per = (nslots + SG_BND_GROUPS - 1) / SG_BND_GROUPS, b0 = g * per, b1 = b0 + per < nslots ? b0 + per : nslots;
    if (k < SG_BND_INTS) {
        int64_t v = 0;
        for (int b = b0; b < b1; b += 8) {
            int64_t e[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) e[u] = b + u < b1 ? slots[(int64_t)(b + u) * SG_BND_SLOT + k] : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) v = k >= 70 ? (e[u] > v ? e[u] : v) : v + e[u];
        }
        ipart[g][k] = v;
    } else if (k < SG_BND_SLOT) {
        double v = 0.0;
        for (int b = b0; b < b1; b += 8) {
            double e[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) e[u] = b + u < b1 ? ((const double*)slots)[(int64_t)(b + u) * SG_BND_SLOT + k] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) v += e[u];      // slot order: the sum repeats to the bit
        }
        fpart[g][k - SG_BND_INTS] = v;
    }
    SG_SYNC();      // ipart[] and fpart[] complete
    if (g == 0 && k < SGAN_BND_COUNTS) {
        int64_t v = 0;
        if (k < SG_BND_INTS)
            for (int q = 0; q < SG_BND_GROUPS; ++q) v = k >= 70 ? (ipart[q][k] > v ? ipart[q][k] : v) : v + ipart[q][k];
        tot[k] = v;
    }
    if (g == 1 && k < 2) {
        double v = 0.0;
        for (int q = 0; q < SG_BND_GROUPS; ++q) v += fpart[q][k];
        ftot[k] = v;
    }
    SG_SYNC();      // tot[] and ftot[] complete
    if (g != 0) return;
    const bool both = tot[64] > 0 && tot[65] > 0;      // then every wall pixel has a defined distance
    if (k < SGAN_BND_COUNTS) {
        const int64_t v = k == 66 ? 1 : (k == 67 ? (both ? 1 : 0) : tot[k]);
        if (k == 70 || k == 71) acc_i[k] = acc_i[k] > v ? acc_i[k] : v;
        else if (k < SG_BND_INTS) acc_i[k] += v;
        else acc_i[k] = 0;
        if (counts_out) counts_out[k] = v;
    }
    if (k == 0) {
        const int64_t far = tot[70] > tot[71] ? tot[70] : tot[71];
        const double haus = both ? sqrt((double)far) : 0.0;
        acc_f[0] += ftot[0];
        acc_f[1] += ftot[1];
        acc_f[2] += haus;
        acc_f[3] = 0.0;
        if (sums_out) {
            sums_out[0] = ftot[0];
            sums_out[1] = ftot[1];
            sums_out[2] = haus;
            sums_out[3] = 0.0;
        }
    }
}

static int sg_bnd_grid(int64_t n) {
    const int64_t want = (n + 255) / 256;
    return (int)(want < SG_BND_BLOCKS ? want : SG_BND_BLOCKS);
}

extern "C" int64_t sgan_boundary_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return 8ll * SG_BND_SLOT * sg_bnd_grid((int64_t)H * W);
}

extern "C" int sgan_boundary_accumulate(const int32_t* t_dsq, const int32_t* s_dsq, int32_t H, int32_t W, void* workspace,
                                        int64_t workspace_bytes, int64_t* acc_i, double* acc_f, int64_t* counts_out, double* sums_out,
                                        int32_t* dev_err, void* stream) {
    SG_REFUSE(t_dsq && s_dsq && workspace && acc_i && acc_f && dev_err, "null pointer");
    SG_REFUSE(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "bad shape %d x %d", H, W);
    const int64_t n = (int64_t)H * W;
    const int grid = sg_bnd_grid(n);
    const int64_t need = 8ll * SG_BND_SLOT * grid;
    SG_REFUSE(workspace_bytes >= need, "workspace of %lld bytes, %lld needed for %d x %d (sgan_boundary_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)need, H, W);
    SG_REFUSE(((uintptr_t)workspace & 7) == 0, "workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_bnd_count_kernel, dim3(grid), dim3(256), 0, st, t_dsq, s_dsq, n, (int64_t*)workspace);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_bnd_final_kernel, dim3(1), dim3(SG_BND_GROUPS * 128), 0, st, (const int64_t*)workspace, grid, acc_i, acc_f, counts_out, sums_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_bnd_count_kernel";
    return SGAN_OK;
}
