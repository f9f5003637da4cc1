// Splitting merged cells at wall gaps (include/sgan_hip.h, "splitting merged cells"): one marker per core of the
// free space (the pixels whose exact distance to the wall is at least a radius), the markers grown back through the free pixels in
// synchronous rounds, a wall pixel set wherever two different markers meet.  The distance transform and the labelling of the cores
// are the library's own exact kernels, called through their public entries (sgan_edt_sq, sgan_ccl_label); this file holds the
// threshold pass between them, the flood and the cut.  Everything after the transform is integers, and every pixel's label is a
// function of the input alone (DESIGN.md §R25 has the induction), so nothing depends on the order workgroups or atomics arrive in.
//
//   thresh: the int32 dsq plane to the plane sgan_ccl_label reads: 0.0 on a core pixel (d >= split_rsq), 1.0 elsewhere, so that
//           the "free" components it labels are the cores; zeroes the round counters.
//   flood:  labels are int32: -1 wall (and everything outside the image), 0 a free pixel not reached yet, else the core label
//           (1 + the core component's smallest raster index).  One round: a pixel that is 0 takes the smallest positive label among
//           its eight neighbours of the round before.  A label at round r depends on the pixels at most r away, so a workgroup holds
//           a 48 x 32 core with an 8-pixel halo (a 64 x 48 region, one wave per region row) in LDS and runs up to 8 rounds there:
//           after round s the outermost s rings of the region may be wrong, the rest is exact, and the core is written back
//           (sgan_thin's pattern).  Two label planes are ping-ponged between launches, because a tile's halo is its neighbours' state
//           BEFORE the launch.  The first launch reads the labelling and takes the wall from dsq == 0.  A tile in which a round
//           labelled nothing anywhere in the region stops its rounds there: no later round can label anything either.
//           cnt[r] = core pixels labelled in round r, over all tiles: the image's count, since the cores tile the image.  A launch
//           whose predecessor's last round labelled nothing returns at once and leaves its destination untouched.
//   cut:    derives from cnt how many flood launches ran, which names the live label plane; a free labelled pixel whose E, SW, S or
//           SE neighbour carries another nonzero label becomes wall (every 8-adjacent pair is seen from exactly one of its members);
//           writes out = wall | cut and finishes the counters.
// Workspace: [sgan_edt_sq's workspace][dsq: H W int32][core: H W float][labels 0: H W int32][labels 1: H W int32]
// [cnt: SG_SPLIT_MAX_ROUNDS int32], each rounded up to 16 bytes.
#include "sgan_common.h"

#define SG_SPLIT_K 8                                      // halo = rounds per launch
#define SG_SPLIT_TH 32                                    // core rows of a tile
#define SG_SPLIT_RW 64                                    // region width: one wave holds one row of the region, one LDS bank per lane
#define SG_SPLIT_TW (SG_SPLIT_RW - 2 * SG_SPLIT_K)        // core columns of a tile
#define SG_SPLIT_RH (SG_SPLIT_TH + 2 * SG_SPLIT_K)
#define SG_SPLIT_THREADS 256
#define SG_SPLIT_PER 4                                    // pixels per thread of the streaming passes, 256 apart
#define SG_SPLIT_BLOCK (SG_SPLIT_THREADS * SG_SPLIT_PER)
#define SG_SPLIT_MAX_RSQ 4096
#define SG_SPLIT_MAX_ROUNDS 4096
#define SG_SPLIT_MAX_DIM 32768                            // sgan_edt_sq's limit
#define SG_SPLIT_ERR_BUDGET 64                            // round max_rounds still labelled something

#define SG_SPLIT_REFUSE(cond, ...)                      \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

// acc[k] += the sum of v over the wave; every lane of the wave calls it
__device__ __forceinline__ void sg_split_add(int64_t* acc, int k, int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)&acc[k], (unsigned long long)v);
}

__global__ __launch_bounds__(SG_SPLIT_THREADS) void sg_split_thresh_kernel(const int32_t* __restrict__ dsq, int n, int rsq, float* __restrict__ core,
                                                                           int32_t* __restrict__ cnt, int rounds) {
    const int base = blockIdx.x * SG_SPLIT_BLOCK + threadIdx.x;      // n < 2^30: no overflow
    for (int j = blockIdx.x * SG_SPLIT_THREADS + threadIdx.x; j < rounds; j += gridDim.x * SG_SPLIT_THREADS) cnt[j] = 0;
#pragma unroll
    for (int k = 0; k < SG_SPLIT_PER; ++k) {
        const int i = base + k * SG_SPLIT_THREADS;
        if (i < n) core[i] = dsq[i] >= rsq ? 0.f : 1.f;      // -1 (no wall at all) is below every radius: no core, nothing to split
    }
}

// Rounds r0 .. r0 + nr - 1 (nr <= SG_SPLIT_K) of the tile at (blockIdx.x, blockIdx.y): src -> dst.  dsq: given to the first launch
// only, whose src is the labelling of the cores (0 on the wall); every later src carries the wall as -1.
__global__ __launch_bounds__(SG_SPLIT_THREADS) void sg_split_flood_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dsq,
                                                                          int32_t* __restrict__ dst, int H, int W, int32_t* cnt, int r0, int nr) {
    if (r0 > 0 && cnt[r0 - 1] == 0) return;      // converged before this launch (uniform over the grid): dst stays as it is
    __shared__ int32_t M[2][SG_SPLIT_RH * SG_SPLIT_RW];
    __shared__ int labelled[SG_SPLIT_K], touched[SG_SPLIT_K];
    const int tid = threadIdx.x;
    const int cx0 = blockIdx.x * SG_SPLIT_TW, cy0 = blockIdx.y * SG_SPLIT_TH;
    for (int p = tid; p < SG_SPLIT_RH * SG_SPLIT_RW; p += SG_SPLIT_THREADS) {
        const int y = cy0 - SG_SPLIT_K + p / SG_SPLIT_RW, x = cx0 - SG_SPLIT_K + p % SG_SPLIT_RW;
        int32_t v = -1;      // outside the image: wall
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int i = y * W + x;
            v = (dsq && dsq[i] == 0) ? -1 : src[i];
        }
        M[0][p] = v;
    }
    if (tid < SG_SPLIT_K) labelled[tid] = touched[tid] = 0;
    SG_SYNC();      // the region and the two counter rows are in place
    const int rx = tid % SG_SPLIT_RW;
    int s = 0;
    while (s < nr) {
        const int32_t* a = M[s & 1];
        int32_t* b = M[(s & 1) ^ 1];
        const int lo = s + 1;      // rings 0 .. s are not needed any more
        int got = 0, got_core = 0;
        if (rx >= lo && rx < SG_SPLIT_RW - lo) {
            for (int ry = lo + tid / SG_SPLIT_RW; ry < SG_SPLIT_RH - lo; ry += SG_SPLIT_THREADS / SG_SPLIT_RW) {      // uniform over a wave
                const int p = ry * SG_SPLIT_RW + rx;
                int32_t v = a[p];
                if (v == 0) {
                    // label - 1 as unsigned: a positive label stays small, 0 and -1 become the two largest values
                    unsigned m = (unsigned)a[p - SG_SPLIT_RW - 1] - 1u;
                    m = min(m, (unsigned)a[p - SG_SPLIT_RW] - 1u);
                    m = min(m, (unsigned)a[p - SG_SPLIT_RW + 1] - 1u);
                    m = min(m, (unsigned)a[p - 1] - 1u);
                    m = min(m, (unsigned)a[p + 1] - 1u);
                    m = min(m, (unsigned)a[p + SG_SPLIT_RW - 1] - 1u);
                    m = min(m, (unsigned)a[p + SG_SPLIT_RW] - 1u);
                    m = min(m, (unsigned)a[p + SG_SPLIT_RW + 1] - 1u);
                    if (m < 0x7fffffffu) {
                        v = (int32_t)(m + 1u);
                        ++got;
                        if (rx >= SG_SPLIT_K && rx < SG_SPLIT_RW - SG_SPLIT_K && ry >= SG_SPLIT_K && ry < SG_SPLIT_RH - SG_SPLIT_K) ++got_core;
                    }
                }
                b[p] = v;
            }
        }
        if (got_core) atomicAdd(&labelled[s], got_core);
        if (got) atomicOr(&touched[s], 1);
        SG_SYNC();      // round s is complete in b, and nobody reads a any more: the next one overwrites it
        ++s;
        if (touched[s - 1] == 0) break;      // uniform: nothing left to label in this region, now or in any later round
    }
    const int32_t* f = M[s & 1];
    for (int p = tid; p < SG_SPLIT_TH * SG_SPLIT_TW; p += SG_SPLIT_THREADS) {
        const int cy = p / SG_SPLIT_TW, cx = p % SG_SPLIT_TW, y = cy0 + cy, x = cx0 + cx;
        if (y < H && x < W) dst[y * W + x] = f[(cy + SG_SPLIT_K) * SG_SPLIT_RW + cx + SG_SPLIT_K];
    }
    if (tid < nr && labelled[tid]) atomicAdd(&cnt[r0 + tid], labelled[tid]);
}

// Flood launch j >= 1 ran iff cnt[j * SG_SPLIT_K - 1] > 0, and the launches that ran are the first ones; launch j writes plane
// (j + 1) & 1, so with `ran` launches run in all the live plane is number ran & 1.
__global__ __launch_bounds__(SG_SPLIT_THREADS) void sg_split_cut_kernel(const int32_t* __restrict__ l0, const int32_t* __restrict__ l1,
                                                                        const int32_t* __restrict__ cnt, int rounds, int H, int W,
                                                                        float* __restrict__ out, int64_t* acc, int32_t* dev_err) {
    __shared__ int ran, active;
    if (threadIdx.x == 0) {
        ran = 1;
        active = 0;
    }
    SG_SYNC();      // the two counts initialised
    for (int r = threadIdx.x; r < rounds; r += SG_SPLIT_THREADS) {
        if (cnt[r] > 0) {
            atomicAdd(&active, 1);
            if ((r + 1) % SG_SPLIT_K == 0 && r + 1 < rounds) atomicAdd(&ran, 1);
        }
    }
    SG_SYNC();      // the two counts complete
    const int32_t* __restrict__ L = (ran & 1) ? l1 : l0;
    const int n = H * W;
    const int base = blockIdx.x * SG_SPLIT_BLOCK + threadIdx.x;
    int cores = 0, cuts = 0, reached = 0;
#pragma unroll
    for (int k = 0; k < SG_SPLIT_PER; ++k) {
        const int i = base + k * SG_SPLIT_THREADS;
        if (i >= n) continue;
        const int y = i / W, x = i - y * W;
        const int32_t v = L[i];
        bool cut = false;
        if (v > 0) {
            const bool e = x + 1 < W, w = x > 0, s = y + 1 < H;
            int32_t q;
            if (e && (q = L[i + 1]) > 0 && q != v) cut = true;
            if (s && w && (q = L[i + W - 1]) > 0 && q != v) cut = true;
            if (s && (q = L[i + W]) > 0 && q != v) cut = true;
            if (s && e && (q = L[i + W + 1]) > 0 && q != v) cut = true;
            ++reached;
            cores += v == i + 1 ? 1 : 0;      // a core component is counted at its root: label - 1 == raster index
        }
        out[i] = (v < 0 || cut) ? 1.f : 0.f;
        cuts += cut ? 1 : 0;
    }
    const bool short_of = cnt[rounds - 1] > 0;      // the budget's last round still labelled something
    if (blockIdx.x == 0 && threadIdx.x == 0 && short_of)
        __hip_atomic_fetch_or(dev_err, SG_SPLIT_ERR_BUDGET, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!acc) return;      // uniform
    sg_split_add(acc, 0, cores);
    sg_split_add(acc, 1, cuts);
    sg_split_add(acc, 2, reached);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (active) atomicAdd((unsigned long long*)&acc[3], (unsigned long long)active);
        if (short_of) atomicAdd((unsigned long long*)&acc[4], 1ull);
        atomicAdd((unsigned long long*)&acc[5], 1ull);
    }
}

struct SgSplitLayout {
    int64_t off_dsq, off_core, off_lab0, off_lab1, off_cnt, bytes;
};

static bool sg_split_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= SG_SPLIT_MAX_DIM && W <= SG_SPLIT_MAX_DIM && (int64_t)H * W < (1ll << 30);
}

static SgSplitLayout sg_split_layout(int32_t H, int32_t W) {
    const int64_t plane = (4ll * H * W + 15) & ~15ll;
    SgSplitLayout l;
    l.off_dsq = (sgan_edt_workspace(H, W) + 15) & ~15ll;
    l.off_core = l.off_dsq + plane;
    l.off_lab0 = l.off_core + plane;
    l.off_lab1 = l.off_lab0 + plane;
    l.off_cnt = l.off_lab1 + plane;
    l.bytes = l.off_cnt + 4ll * SG_SPLIT_MAX_ROUNDS;
    return l;
}

extern "C" int64_t sgan_split_workspace(int32_t H, int32_t W) {
    if (!sg_split_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_split_layout(H, W).bytes;
}

extern "C" int sgan_split_cells(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t split_rsq, int32_t max_rounds, float* out,
                                int64_t* acc, void* workspace, int64_t workspace_bytes, int32_t* dev_err, void* stream) {
    SG_SPLIT_REFUSE(plane && out && workspace && dev_err, "null pointer");
    SG_SPLIT_REFUSE(sg_split_shape_ok(H, W) && pix_stride >= 1, "bad shape %d x %d (H, W <= %d, H W < 2^30), pixel stride %lld", H, W,
                    SG_SPLIT_MAX_DIM, (long long)pix_stride);
    SG_SPLIT_REFUSE(split_rsq >= 1 && split_rsq <= SG_SPLIT_MAX_RSQ && max_rounds >= 1 && max_rounds <= SG_SPLIT_MAX_ROUNDS,
                    "bad parameter: split_rsq %d (1 .. %d), max_rounds %d (1 .. %d)", split_rsq, SG_SPLIT_MAX_RSQ, max_rounds,
                    SG_SPLIT_MAX_ROUNDS);
    SG_SPLIT_REFUSE((const float*)out != plane, "out aliases the plane");
    const SgSplitLayout l = sg_split_layout(H, W);
    SG_SPLIT_REFUSE(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_split_workspace); nothing was launched",
                    (long long)workspace_bytes, (long long)l.bytes, H, W);
    SG_SPLIT_REFUSE(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    int32_t* dsq = (int32_t*)((char*)workspace + l.off_dsq);
    float* core = (float*)((char*)workspace + l.off_core);
    int32_t* lab[2] = {(int32_t*)((char*)workspace + l.off_lab0), (int32_t*)((char*)workspace + l.off_lab1)};
    int32_t* cnt = (int32_t*)((char*)workspace + l.off_cnt);
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W;
    const dim3 grid((n + SG_SPLIT_BLOCK - 1) / SG_SPLIT_BLOCK), block(SG_SPLIT_THREADS);
    const dim3 tiles((W + SG_SPLIT_TW - 1) / SG_SPLIT_TW, (H + SG_SPLIT_TH - 1) / SG_SPLIT_TH);      // at most 683 x 1024
    int rc;

    if ((rc = sgan_edt_sq(plane, pix_stride, H, W, dsq, workspace, l.off_dsq, dev_err, stream)) != SGAN_OK) return rc;
    hipLaunchKernelGGL(sg_split_thresh_kernel, grid, block, 0, st, (const int32_t*)dsq, n, split_rsq, core, cnt, max_rounds);
    SGAN_LAUNCH_CHECK();
    if ((rc = sgan_ccl_label(core, 1, H, W, lab[0], dev_err, stream)) != SGAN_OK) return rc;
    int j = 0;
    for (int r0 = 0; r0 < max_rounds; r0 += SG_SPLIT_K, ++j) {
        const int nr = max_rounds - r0 < SG_SPLIT_K ? max_rounds - r0 : SG_SPLIT_K;
        hipLaunchKernelGGL(sg_split_flood_kernel, tiles, block, 0, st, (const int32_t*)lab[j & 1], j == 0 ? (const int32_t*)dsq : (const int32_t*)nullptr,
                           lab[(j + 1) & 1], H, W, cnt, r0, nr);
        SGAN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sg_split_cut_kernel, grid, block, 0, st, (const int32_t*)lab[0], (const int32_t*)lab[1], (const int32_t*)cnt, max_rounds, H, W,
                       out, acc, dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_split_flood_kernel";
    return SGAN_OK;
}
