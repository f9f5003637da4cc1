// Topology scores of a wall map against the truth (include/sgan_hip.h, "topology scores"): the Betti numbers of
// every window of both maps, and the four skeleton counts of clDice.  Integers only; every number is exact and repeats to the bit.
//
// Betti numbers of a window (wh x ww <= 64 x 64 pixels, cut out of the map: everything outside it is free):
//   b0 = the 8-connected components of the wall pixels,  b1 = the 4-connected components of the free pixels that own no pixel of
//   the window's edge.  One workgroup of 256 threads per (window, map); no workgroup waits for another.
//   LDS: rows[64]    one uint64 of wall bits per row of the window (bit x = pixel x), built with a ballot per row;
//        parent[4096] the union-find forest over pixel y * 64 + x.  Wall and free pixels are disjoint sets of nodes, so ONE forest holds
//                    both labellings: a wall pixel is only ever united with wall pixels, a free one with free ones;
//        edge[128]   one bit per node: "this free root owns an edge pixel".
//   Union: a link always goes from the larger index to the smaller (atomicMin on the larger root's slot), so parent[i] <= i at every
//   moment, whatever the interleaving.  A find from i therefore ends in at most i < 4096 steps, and every retry of a unite starts
//   from a strictly smaller larger-root than the one before, so it ends in at most 4096 rounds.  Both loops are written with that
//   bound; one that runs out sets SGAN_TOPO_ERR_BIT of dev_err and the window writes (-1, -1), which the summing launch skips.
//   A serpentine (one component, ~N^2 / 2 pixels long) is N^2 / 2 unites and the finds compress the paths as they walk them; a
//   checkerboard (N^2 / 2 free components) is N^2 roots counted.  Neither changes the bound.
//   Which neighbours a pixel unites with: a wall pixel with N when N is wall (N then already ties W, NW and NE to it through their
//   own links), else with W, or with NW when W is not wall, and with NE; a free pixel with W and with N.
//   Roots are counted with a ballot and a popcount per wave, the four waves' counts meet in LDS.
// Summing: a grid-stride launch over the windows adds windows, |b0(S) - b0(T)|, |b1(S) - b1(T)| and the four plain sums, reduced per
//   wave and per workgroup, with one 64-bit atomic add per workgroup and counter.  Skeleton: a grid-stride launch over the pixels
//   counts the thinned pixels of each map and those of them that are wall in the other map, reduced the same way.
// Workspace: int32 [windows][2 maps: 0 = prediction, 1 = truth][b0, b1].
#include "sgan_common.h"
#include "sgan_reduce.h"

#define SG_TOPO_THREADS 256
#define SG_TOPO_PITCH 64             // nodes per row of the forest: the largest window
#define SG_TOPO_NODES (SG_TOPO_PITCH * SG_TOPO_PITCH)
#define SG_TOPO_SUM_BLOCKS 64        // workgroups of the summing launch, at most
#define SG_TOPO_SKEL_BLOCKS 256      // ... of the skeleton launch
#define SG_TOPO_MAX_DIM 32768

// a refused call: the reason goes to sgan_last_error, the entry returns 1 and has launched nothing
#define SG_REFUSE(cond, ...)                            \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

// the forest is read and written by every thread of the workgroup between two barriers: relaxed atomics at workgroup scope, so that
// no value is kept in a register across a link another thread makes
__device__ __forceinline__ int sg_topo_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The root of i, the paths halved on the way (parent[i] = min(parent[i], grandparent): a slot only ever decreases).  At most
// SG_TOPO_NODES steps, since every step goes to a smaller index; *bad is set if that bound is ever not enough.
__device__ __forceinline__ int sg_topo_find(int* parent, int i, int* bad) {
    for (int k = 0; k < SG_TOPO_NODES; ++k) {
        const int p = sg_topo_ld(&parent[i]);
        if (p == i) return i;
        const int g = sg_topo_ld(&parent[p]);
        if (g != p) atomicMin(&parent[i], g);
        i = p;
    }
    *bad = 1;
    return i;
}

// Unites the sets of a and b.  A round links the larger root under the smaller with an atomicMin; when another thread got to that
// slot first (it held `old` < a, no root any more) the round goes on with (old, b), both below the a it started with.
__device__ __forceinline__ void sg_topo_unite(int* parent, int a, int b, int* bad) {
    for (int k = 0; k < SG_TOPO_NODES; ++k) {
        a = sg_topo_find(parent, a, bad);
        b = sg_topo_find(parent, b, bad);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
    *bad = 1;
}

__global__ __launch_bounds__(SG_TOPO_THREADS) void sg_topo_betti_kernel(const float* __restrict__ s, int64_t s_ld, const float* __restrict__ t,
                                                                        int64_t t_ld, int W, int wh, int ww, int nx, int stride,
                                                                        int32_t* __restrict__ betti, int64_t* counts_out, int32_t* dev_err) {
    __shared__ unsigned long long rows[SG_TOPO_PITCH];
    __shared__ int parent[SG_TOPO_NODES];
    __shared__ unsigned edge[SG_TOPO_NODES / 32];
    __shared__ int cnt[SG_TOPO_THREADS / 64][2];
    __shared__ int bad;
    const int tid = threadIdx.x, x = tid & 63, wave = tid >> 6;
    const int win = blockIdx.x, map = blockIdx.y;
    if (counts_out && win == 0 && map == 0 && tid < SGAN_TOPO_COUNTS) counts_out[tid] = 0;      // the later launches add to it
    const float* plane = map ? t : s;
    const int64_t ld = map ? t_ld : s_ld;
    const int oy = (win / nx) * stride, ox = (win % nx) * stride;      // oy + wh <= H and ox + ww <= W by the host's window count
    if (tid < SG_TOPO_NODES / 32) edge[tid] = 0u;
    if (tid == 0) bad = 0;
    for (int y = wave; y < wh; y += SG_TOPO_THREADS / 64) {      // a wave owns a row: lane x is pixel x
        const bool in = x < ww;
        const bool wall = in && plane[((int64_t)(oy + y) * W + ox + x) * ld] > 0.5f;      // a NaN and an exact 0.5 are not wall
        const unsigned long long m = __ballot(wall);
        if (x == 0) rows[y] = m;
        if (in) parent[y * SG_TOPO_PITCH + x] = y * SG_TOPO_PITCH + x;
    }
    SG_SYNC();      // rows[], parent[], edge[] and bad are set
    int mybad = 0;
    for (int y = wave; y < wh; y += SG_TOPO_THREADS / 64) {
        if (x >= ww) continue;
        const int i = y * SG_TOPO_PITCH + x;
        const unsigned long long here = rows[y], up = y ? rows[y - 1] : 0ull;
        const bool has_w = x > 0, has_n = y > 0;
        if ((here >> x) & 1ull) {      // wall, 8-connected
            const bool n = (up >> x) & 1ull;
            const bool w = has_w && ((here >> (x - 1)) & 1ull), nw = has_w && ((up >> (x - 1)) & 1ull);
            const bool ne = x + 1 < ww && ((up >> (x + 1)) & 1ull);
            if (n) {
                sg_topo_unite(parent, i, i - SG_TOPO_PITCH, &mybad);
            } else {
                if (w) sg_topo_unite(parent, i, i - 1, &mybad);
                else if (nw) sg_topo_unite(parent, i, i - SG_TOPO_PITCH - 1, &mybad);
                if (ne) sg_topo_unite(parent, i, i - SG_TOPO_PITCH + 1, &mybad);
            }
        } else {                       // free, 4-connected
            if (has_w && !((here >> (x - 1)) & 1ull)) sg_topo_unite(parent, i, i - 1, &mybad);
            if (has_n && !((up >> x) & 1ull)) sg_topo_unite(parent, i, i - SG_TOPO_PITCH, &mybad);
        }
    }
    SG_SYNC();      // the forest is complete: from here on it is only read
    int n0 = 0;
    for (int y = wave; y < wh; y += SG_TOPO_THREADS / 64) {
        const bool in = x < ww;
        const int i = y * SG_TOPO_PITCH + x;
        const bool wall = in && ((rows[y] >> x) & 1ull);
        const bool root = in && parent[i] == i;
        n0 += __builtin_popcountll(__ballot(wall && root));
        if (in && !wall && (y == 0 || y == wh - 1 || x == 0 || x == ww - 1)) {
            const int r = sg_topo_find(parent, i, &mybad);
            atomicOr(&edge[r >> 5], 1u << (r & 31));
        }
    }
    if (mybad) bad = 1;
    SG_SYNC();      // edge[] complete
    int n1 = 0;
    for (int y = wave; y < wh; y += SG_TOPO_THREADS / 64) {
        const bool in = x < ww;
        const int i = y * SG_TOPO_PITCH + x;
        const bool hole = in && !((rows[y] >> x) & 1ull) && parent[i] == i && !((edge[i >> 5] >> (i & 31)) & 1u);
        n1 += __builtin_popcountll(__ballot(hole));
    }
    if (x == 0) {
        cnt[wave][0] = n0;
        cnt[wave][1] = n1;
    }
    SG_SYNC();      // cnt[] and bad complete
    if (tid == 0) {
        int b0 = 0, b1 = 0;
        for (int w = 0; w < SG_TOPO_THREADS / 64; ++w) {
            b0 += cnt[w][0];
            b1 += cnt[w][1];
        }
        if (bad) {
            atomicOr(dev_err, SGAN_TOPO_ERR_BIT);
            b0 = b1 = -1;
        }
        int32_t* out = betti + ((int64_t)win * 2 + map) * 2;
        out[0] = b0;
        out[1] = b1;
    }
}

// the sum of v over the workgroup's 256 threads in thread 0 (and every first lane of wave 0); `red`: 4 entries of LDS, free for
// reuse behind the barrier this ends with
__device__ __forceinline__ long long sg_topo_block_sum(long long v, long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    SG_SYNC();
    const long long tot = red[0] + red[1] + red[2] + red[3];
    SG_SYNC();
    return tot;
}

__device__ __forceinline__ void sg_topo_add(int64_t* acc_i, int64_t* counts_out, int k, long long v) {
    if (!v) return;
    atomicAdd((unsigned long long*)&acc_i[k], (unsigned long long)v);
    if (counts_out) atomicAdd((unsigned long long*)&counts_out[k], (unsigned long long)v);
}

__global__ __launch_bounds__(SG_TOPO_THREADS) void sg_topo_sum_kernel(const int32_t* __restrict__ betti, int64_t nwin, int64_t* acc_i,
                                                                      int64_t* counts_out) {
    __shared__ long long red[4];
    long long v[7] = {0, 0, 0, 0, 0, 0, 0};      // windows, abs_d0, abs_d1, b0_s, b0_t, b1_s, b1_t
    for (int64_t w = (int64_t)blockIdx.x * SG_TOPO_THREADS + threadIdx.x; w < nwin; w += (int64_t)gridDim.x * SG_TOPO_THREADS) {
        const int4 b = *(const int4*)(betti + w * 4);      // (b0_s, b1_s, b0_t, b1_t); the workspace is 16-byte aligned
        if (b.x < 0 || b.z < 0) continue;                  // a window that did not converge contributes nothing
        v[0] += 1;
        v[1] += b.x > b.z ? b.x - b.z : b.z - b.x;
        v[2] += b.y > b.w ? b.y - b.w : b.w - b.y;
        v[3] += b.x;
        v[4] += b.z;
        v[5] += b.y;
        v[6] += b.w;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const long long tot = sg_topo_block_sum(v[k], red);
        if (threadIdx.x == 0) sg_topo_add(acc_i, counts_out, k, tot);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sg_topo_add(acc_i, counts_out, SGAN_TOPO_IMAGES, 1);
}

__global__ __launch_bounds__(SG_TOPO_THREADS) void sg_topo_skel_kernel(const float* __restrict__ s, int64_t s_ld, const float* __restrict__ t,
                                                                       int64_t t_ld, const float* __restrict__ s_thin,
                                                                       const float* __restrict__ t_thin, int64_t n, int64_t* acc_i,
                                                                       int64_t* counts_out) {
    __shared__ long long red[4];
    long long v[4] = {0, 0, 0, 0};      // skel_s, skel_s_in_t, skel_t, skel_t_in_s
    for (int64_t i = (int64_t)blockIdx.x * SG_TOPO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_TOPO_THREADS) {
        if (s_thin && s_thin[i] > 0.5f) {
            v[0] += 1;
            v[1] += t[i * t_ld] > 0.5f ? 1 : 0;
        }
        if (t_thin && t_thin[i] > 0.5f) {
            v[2] += 1;
            v[3] += s[i * s_ld] > 0.5f ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long tot = sg_topo_block_sum(v[k], red);
        if (threadIdx.x == 0) sg_topo_add(acc_i, counts_out, SGAN_TOPO_SKEL_S + k, tot);
    }
}

struct SgTopoLayout {
    int wh, ww, ny, nx;
    int64_t nwin, bytes;
};

static bool sg_topo_covered(int32_t window, int32_t stride) { return window >= 8 && window <= SG_TOPO_PITCH && stride >= 1 && stride <= window; }

static bool sg_topo_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= SG_TOPO_MAX_DIM && W <= SG_TOPO_MAX_DIM && (int64_t)H * W < (1ll << 30);
}

static SgTopoLayout sg_topo_layout(int32_t H, int32_t W, int32_t window, int32_t stride) {
    SgTopoLayout l;
    l.wh = window < H ? window : H;
    l.ww = window < W ? window : W;
    l.ny = (H - l.wh) / stride + 1;
    l.nx = (W - l.ww) / stride + 1;
    l.nwin = (int64_t)l.ny * l.nx;      // < 2^30
    l.bytes = 16 * l.nwin;
    return l;
}

extern "C" int64_t sgan_topo_workspace_bytes(int32_t H, int32_t W, int32_t window, int32_t stride) {
    if (!sg_topo_covered(window, stride)) return sgan_fail(SGAN_ERR_INVALID, "not covered: window %d (8..64), stride %d (1..window)", window, stride);
    if (!sg_topo_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_topo_layout(H, W, window, stride).bytes;
}

extern "C" int sgan_topo_accumulate(const float* t, int64_t t_ld, const float* s, int64_t s_ld, const float* t_thin, const float* s_thin,
                                    int32_t H, int32_t W, int32_t window, int32_t stride, void* workspace, int64_t workspace_bytes,
                                    int64_t* acc_i, int64_t* counts_out, int32_t* dev_err, void* stream) {
    SG_REFUSE(sg_topo_covered(window, stride), "not covered: window %d (8..64), stride %d (1..window)", window, stride);
    SG_REFUSE(t && s && workspace && acc_i && dev_err, "null pointer");
    SG_REFUSE(sg_topo_shape_ok(H, W) && t_ld >= 1 && s_ld >= 1, "bad shape %d x %d (H, W <= %d, H W < 2^30), pixel strides %lld, %lld", H, W,
               SG_TOPO_MAX_DIM, (long long)t_ld, (long long)s_ld);
    const SgTopoLayout l = sg_topo_layout(H, W, window, stride);
    SG_REFUSE(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d, window %d, stride %d (sgan_topo_workspace_bytes); "
               "nothing was launched", (long long)workspace_bytes, (long long)l.bytes, H, W, window, stride);
    SG_REFUSE(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* betti = (int32_t*)workspace;
    hipLaunchKernelGGL(sg_topo_betti_kernel, dim3((unsigned)l.nwin, 2), dim3(SG_TOPO_THREADS), 0, st, s, s_ld, t, t_ld, W, l.wh, l.ww, l.nx, stride,
                       betti, counts_out, dev_err);
    SGAN_LAUNCH_CHECK();
    const int64_t sum_want = (l.nwin + SG_TOPO_THREADS - 1) / SG_TOPO_THREADS;
    hipLaunchKernelGGL(sg_topo_sum_kernel, dim3((unsigned)(sum_want < SG_TOPO_SUM_BLOCKS ? sum_want : SG_TOPO_SUM_BLOCKS)), dim3(SG_TOPO_THREADS), 0,
                       st, (const int32_t*)betti, l.nwin, acc_i, counts_out);
    SGAN_LAUNCH_CHECK();
    if (t_thin || s_thin) {
        const int64_t n = (int64_t)H * W, want = (n + SG_TOPO_THREADS - 1) / SG_TOPO_THREADS;
        hipLaunchKernelGGL(sg_topo_skel_kernel, dim3((unsigned)(want < SG_TOPO_SKEL_BLOCKS ? want : SG_TOPO_SKEL_BLOCKS)), dim3(SG_TOPO_THREADS), 0,
                           st, s, s_ld, t, t_ld, s_thin, t_thin, n, acc_i, counts_out);
        SGAN_LAUNCH_CHECK();
    }
    g_sgan_last_kernel = "sg_topo_betti_kernel";
    return SGAN_OK;
}
