// Lovasz-softmax loss term (include/sgan_hip.h, "Lovasz-softmax"): the Lovasz extension of the Jaccard loss of up to
// 8 class planes, and its subgradient with respect to the prediction.
//
// The sort is a bitonic network on unique 64-bit keys, one key per pixel and listed class:
//   key = ((0xFFFFFFFF - bits(e)) << 32) | (i << 1) | fg        e = |fg - p| in fp32, i = y W + x, fg = (label == class)
// Ascending keys are e descending, ties by pixel index ascending; fg is a function of i and rides in bit 0, so the sorted key hands
// out pi(k), e and fg at once and no gather along pi is needed.  The network has P = max(4096, 2^ceil(log2 N)) inputs per class; the
// P - N pads are the all-ones key, which is above every pixel's key (a pixel's low word is below 2^21) and so ends behind them.
// Launches, the class being grid dimension y of each:
//   1      sg_lov_sort_chunk_kernel     builds the keys of a chunk of 4096 in LDS and runs the stages k = 2 .. 4096 there
//   then for every stage k = 8192 .. P:
//   log2(k) - 12   sg_lov_merge_global_kernel   one compare-exchange step of stride j >= 4096 in global memory
//   1      sg_lov_merge_chunk_kernel    the steps j = 2048 .. 1 of the stage in LDS
//   1      sg_lov_count_kernel          foreground count of every block of 1024 sorted keys
//   1      sg_lov_offsets_kernel        exclusive scan of the block counts (one workgroup per class) and G, the class's foreground
//   1      sg_lov_weights_kernel        the block's scan, c_k, g_k, pi(k), and the block's fp64 sum of e g into its slot
//   1      sg_lov_finish_kernel         one workgroup: L_c from the slots in a fixed order, the present count m, L, the scales 1 / m
// and for the backward
//   1      sg_lov_bwd_kernel            grid y = channel: a listed channel scatters gamma s g_k scale through pi (a bijection: every
//                                       pixel of the plane is written once, with +0 where the scale is 0), an unlisted one is zeroed.
// A phase depends on another only across a launch boundary; no workgroup waits on another, no floating-point atomic anywhere; the
// integer atomics are LDS counters.  Grids and launch count depend on (H, W, n) alone.
#include "sgan_common.h"
#include "sgan_reduce.h"

#define SG_LOV_CHUNK 4096            // keys of one LDS sort (32 KiB)
#define SG_LOV_CHUNK_LOG 12
#define SG_LOV_SORT_THREADS 512
#define SG_LOV_THREADS 256
#define SG_LOV_PER 4                 // sorted keys per thread of the scan launches
#define SG_LOV_BLOCK (SG_LOV_THREADS * SG_LOV_PER)
#define SG_LOV_PAD 0xFFFFFFFFFFFFFFFFull

#define SG_REFUSE(cond, ...)                            \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

struct SgLovClasses {
    int32_t cls[SGAN_LOVASZ_MAX_CLASSES];      // the listed classes
};

struct SgLovChannels {
    int32_t slot[64];      // per channel of the prediction: its place in the list, or -1
};

// the workspace, see the header
struct SgLovWs {
    double* state;
    double* g;
    unsigned long long* keys;
    double* slots;
    int32_t* perm;
    int32_t* bsum;
    int64_t N, P, nb, bytes;
};

static int64_t sg_lov_pow2(int64_t N) {
    int64_t P = SG_LOV_CHUNK;
    while (P < N) P <<= 1;
    return P;
}

static SgLovWs sg_lov_layout(void* base, int32_t H, int32_t W, int32_t n) {
    SgLovWs w;
    w.N = (int64_t)H * W;
    w.P = sg_lov_pow2(w.N);
    w.nb = (w.N + SG_LOV_BLOCK - 1) / SG_LOV_BLOCK;
    char* b = (char*)base;
    int64_t off = 0;
    w.state = (double*)(b + off);
    off += SGAN_LOVASZ_STATE_BYTES;
    w.g = (double*)(b + off);
    off += 8 * n * w.N;
    w.keys = (unsigned long long*)(b + off);
    off += 8 * n * w.P;
    w.slots = (double*)(b + off);
    off += 8 * n * w.nb;
    w.perm = (int32_t*)(b + off);
    off += 4 * n * w.N;
    w.bsum = (int32_t*)(b + off);
    off += 4 * n * w.nb;
    w.bytes = (off + 7) & ~7ll;
    return w;
}

// one compare-exchange of the bitonic network on LDS keys: pair t of stride j, ascending where the global index has bit k clear
__device__ __forceinline__ void sg_lov_cmpx(unsigned long long* s, unsigned t, unsigned j, bool up) {
    const unsigned i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i + j;
    const unsigned long long a = s[i], b = s[l];
    if ((a > b) == up) {
        s[i] = b;
        s[l] = a;
    }
}

__global__ __launch_bounds__(SG_LOV_SORT_THREADS) void sg_lov_sort_chunk_kernel(const float* __restrict__ p, int64_t cs, int64_t rs, int64_t ps,
                                                                                const int64_t* __restrict__ label, SgLovClasses cl, int W,
                                                                                int64_t N, int64_t P, unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long s[SG_LOV_CHUNK];
    const int c = blockIdx.y, cls = cl.cls[c];
    const int64_t base = (int64_t)blockIdx.x * SG_LOV_CHUNK;
    for (unsigned q = threadIdx.x; q < SG_LOV_CHUNK; q += SG_LOV_SORT_THREADS) {
        const int64_t i = base + q;
        unsigned long long key = SG_LOV_PAD;
        if (i < N) {
            const int y = (int)(i / W), x = (int)(i % W);
            const float pv = p[cls * cs + y * rs + x * ps];
            const bool fg = label[i] == (int64_t)cls;
            const float e = fabsf((fg ? 1.f : 0.f) - pv);
            key = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(e)) << 32) | (unsigned long long)(((unsigned)i << 1) | (fg ? 1u : 0u));
        }
        s[q] = key;
    }
    SG_SYNC();
    for (unsigned k = 2; k <= SG_LOV_CHUNK; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = threadIdx.x; t < SG_LOV_CHUNK / 2; t += SG_LOV_SORT_THREADS) {
                const unsigned i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
                sg_lov_cmpx(s, t, j, (((uint64_t)base + i) & k) == 0);
            }
            SG_SYNC();
        }
    }
    unsigned long long* out = keys + (int64_t)c * P + base;
    for (unsigned q = threadIdx.x; q < SG_LOV_CHUNK; q += SG_LOV_SORT_THREADS) out[q] = s[q];
}

// stage k, stride j >= SG_LOV_CHUNK: pair t of the P / 2
__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_merge_global_kernel(unsigned long long* __restrict__ keys, int64_t P, uint64_t k, uint64_t j) {
    const uint64_t t = (uint64_t)blockIdx.x * SG_LOV_THREADS + threadIdx.x;
    if (t >= (uint64_t)P / 2) return;
    unsigned long long* s = keys + (int64_t)blockIdx.y * P;
    const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
    const unsigned long long a = s[i], b = s[l];
    if ((a > b) == ((i & k) == 0)) {
        s[i] = b;
        s[l] = a;
    }
}

// stage k > SG_LOV_CHUNK, the strides below SG_LOV_CHUNK: one direction per chunk
__global__ __launch_bounds__(SG_LOV_SORT_THREADS) void sg_lov_merge_chunk_kernel(unsigned long long* __restrict__ keys, int64_t P, uint64_t k) {
    __shared__ unsigned long long s[SG_LOV_CHUNK];
    const int64_t base = (int64_t)blockIdx.x * SG_LOV_CHUNK;
    unsigned long long* io = keys + (int64_t)blockIdx.y * P + base;
    for (unsigned q = threadIdx.x; q < SG_LOV_CHUNK; q += SG_LOV_SORT_THREADS) s[q] = io[q];
    SG_SYNC();
    const bool up = ((uint64_t)base & k) == 0;
    for (unsigned j = SG_LOV_CHUNK / 2; j > 0; j >>= 1) {
        for (unsigned t = threadIdx.x; t < SG_LOV_CHUNK / 2; t += SG_LOV_SORT_THREADS) sg_lov_cmpx(s, t, j, up);
        SG_SYNC();
    }
    for (unsigned q = threadIdx.x; q < SG_LOV_CHUNK; q += SG_LOV_SORT_THREADS) io[q] = s[q];
}

// exclusive prefix of v over the workgroup's 256 threads in thread order; *total = the workgroup's sum.  `ws`: 4 ints of LDS, free
// again behind a barrier of the caller's.
__device__ __forceinline__ int sg_lov_block_scan(int v, int* ws, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    SG_SYNC();
    int before = 0, all = 0;
    for (int w = 0; w < SG_LOV_THREADS / 64; ++w) {
        const int x = ws[w];
        if (w < wave) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

// the four sorted keys of thread t of block b, as foreground flags (0 behind the N-th)
__device__ __forceinline__ void sg_lov_load4(const unsigned long long* __restrict__ s, int64_t k0, int64_t N, unsigned long long key[SG_LOV_PER],
                                             int f[SG_LOV_PER]) {
#pragma unroll
    for (int q = 0; q < SG_LOV_PER; ++q) {
        key[q] = k0 + q < N ? s[k0 + q] : SG_LOV_PAD;
        f[q] = k0 + q < N ? (int)(key[q] & 1ull) : 0;
    }
}

__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_count_kernel(const unsigned long long* __restrict__ keys, int64_t P, int64_t N, int nb,
                                                                      int32_t* __restrict__ bsum) {
    __shared__ int ws[SG_LOV_THREADS / 64];
    unsigned long long key[SG_LOV_PER];
    int f[SG_LOV_PER], total;
    sg_lov_load4(keys + (int64_t)blockIdx.y * P, (int64_t)blockIdx.x * SG_LOV_BLOCK + threadIdx.x * SG_LOV_PER, N, key, f);
    sg_lov_block_scan(f[0] + f[1] + f[2] + f[3], ws, &total);
    if (threadIdx.x == 0) bsum[(int64_t)blockIdx.y * nb + blockIdx.x] = total;
}

// block counts -> exclusive offsets, in place; G[c] = the class's foreground.  One workgroup per class, nb <= 1024 = 4 per thread.
__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_offsets_kernel(int32_t* __restrict__ bsum, int nb, int32_t* __restrict__ G) {
    __shared__ int ws[SG_LOV_THREADS / 64];
    int32_t* b = bsum + (int64_t)blockIdx.x * nb;
    const int b0 = threadIdx.x * SG_LOV_PER;
    int v[SG_LOV_PER], total;
#pragma unroll
    for (int q = 0; q < SG_LOV_PER; ++q) v[q] = b0 + q < nb ? b[b0 + q] : 0;
    int run = sg_lov_block_scan(v[0] + v[1] + v[2] + v[3], ws, &total);
#pragma unroll
    for (int q = 0; q < SG_LOV_PER; ++q) {
        if (b0 + q < nb) b[b0 + q] = run;
        run += v[q];
    }
    if (threadIdx.x == 0) G[blockIdx.x] = total;
}

__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_weights_kernel(const unsigned long long* __restrict__ keys, int64_t P, int64_t N, int nb,
                                                                        const int32_t* __restrict__ boff, const int32_t* __restrict__ G,
                                                                        int32_t* __restrict__ perm, double* __restrict__ gw,
                                                                        double* __restrict__ slots) {
    __shared__ int ws[SG_LOV_THREADS / 64];
    __shared__ double red[SG_LOV_THREADS / 64];
    const int c = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * SG_LOV_BLOCK + threadIdx.x * SG_LOV_PER;
    unsigned long long key[SG_LOV_PER];
    int f[SG_LOV_PER], total;
    sg_lov_load4(keys + (int64_t)c * P, k0, N, key, f);
    int64_t ck = sg_lov_block_scan(f[0] + f[1] + f[2] + f[3], ws, &total) + boff[(int64_t)c * nb + blockIdx.x];
    const int64_t Gc = G[c];
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < SG_LOV_PER; ++q) {
        const int64_t k = k0 + q;
        if (k >= N) break;
        ck += f[q];
        const int64_t I = Gc - ck, U = Gc + (k + 1 - ck);
        double g = 0.0;      // an absent class: I = 0 throughout, every weight is 0
        if (f[q])
            g = 1.0 / (double)U;
        else if (I > 0)
            g = (double)I / (double)(U * (U - 1));
        const float e = __uint_as_float(0xFFFFFFFFu - (unsigned)(key[q] >> 32));
        acc += (double)e * g;
        perm[(int64_t)c * N + k] = (int32_t)((unsigned)key[q] >> 1);
        gw[(int64_t)c * N + k] = g;
    }
    acc = sg_block_sum<SG_LOV_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) slots[(int64_t)c * nb + blockIdx.x] = acc;
}

// state (doubles): [0] L  [1] m  [2 + j] L_c of listed class j (0 if absent)  [10 + j] its scale 1 / m (0 if absent);
// the int32 G[8] stand at double 24
__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_finish_kernel(const double* __restrict__ slots, int nb, int n, double* __restrict__ state,
                                                                       float* __restrict__ loss_out) {
    __shared__ double red[SG_LOV_THREADS / 64];
    const int32_t* G = (const int32_t*)(state + 24);
    double Lc[SGAN_LOVASZ_MAX_CLASSES];
    for (int c = 0; c < n; ++c) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < nb; b += SG_LOV_THREADS) acc += slots[(int64_t)c * nb + b];
        Lc[c] = sg_block_sum<SG_LOV_THREADS / 64>(acc, red);
        SG_SYNC();
    }
    if (threadIdx.x != 0) return;
    int m = 0;
    double tot = 0.0;
    for (int c = 0; c < n; ++c) {
        if (G[c] > 0) {
            ++m;
            tot += Lc[c];
        }
    }
    const double L = m ? tot / (double)m : 0.0;
    state[0] = L;
    state[1] = (double)m;
    for (int c = 0; c < SGAN_LOVASZ_MAX_CLASSES; ++c) {
        const bool present = c < n && G[c] > 0;
        state[2 + c] = present ? Lc[c] : 0.0;
        state[10 + c] = present ? 1.0 / (double)m : 0.0;
    }
    loss_out[0] = (float)L;
}

__global__ __launch_bounds__(SG_LOV_THREADS) void sg_lov_bwd_kernel(const float* __restrict__ p, int64_t cs, int64_t rs, int64_t ps, SgLovChannels ch,
                                                                    int W, int64_t N, int64_t P, const unsigned long long* __restrict__ keys,
                                                                    const double* __restrict__ gw, const double* __restrict__ state,
                                                                    const float* __restrict__ gout, float* __restrict__ dp) {
    const int64_t k = (int64_t)blockIdx.x * SG_LOV_THREADS + threadIdx.x;
    if (k >= N) return;
    const int channel = blockIdx.y, c = ch.slot[channel];
    float* out = dp + (int64_t)channel * N;
    if (c < 0) {
        out[k] = 0.f;
        return;
    }
    const unsigned long long key = keys[(int64_t)c * P + k];
    const int64_t i = (int64_t)((unsigned)key >> 1);
    if (i >= N) return;      // never with a sorted workspace: the first N keys are the pixels'
    const double scale = state[10 + c];
    float v = 0.f;
    if (scale != 0.0) {
        const int y = (int)(i / W), x = (int)(i % W);
        const float pv = p[channel * cs + y * rs + x * ps], fg = (key & 1ull) ? 1.f : 0.f;
        const double s = (double)((pv > fg) - (pv < fg));
        v = (float)((gout ? (double)gout[0] : 1.0) * s * gw[(int64_t)c * N + k] * scale);
    }
    out[i] = v;
}

static bool sg_lov_covered(int32_t H, int32_t W, int32_t n) {
    return H >= 1 && W >= 1 && (int64_t)H * W <= SGAN_LOVASZ_MAX_PIXELS && n >= 1 && n <= SGAN_LOVASZ_MAX_CLASSES;
}

#define SG_LOV_COVERED(H, W, n)                                                                                                          \
    SG_REFUSE(sg_lov_covered(H, W, n), "not covered: %d x %d pixels, %d classes (H, W >= 1, H W <= 2^20, 1 .. %d classes)", H, W, n, \
              SGAN_LOVASZ_MAX_CLASSES)

static bool sg_lov_classes_ok(const int32_t* classes, int32_t n, int32_t C) {
    for (int a = 0; a < n; ++a) {
        if (classes[a] < 0 || classes[a] >= C) return false;
        for (int b = 0; b < a; ++b)
            if (classes[a] == classes[b]) return false;
    }
    return true;
}

static bool sg_lov_strides_ok(int32_t H, int32_t W, int64_t cs, int64_t rs, int64_t ps) {
    return cs >= 1 && ps >= 1 && (H == 1 || rs >= (int64_t)(W - 1) * ps + 1);
}

extern "C" int64_t sgan_lovasz_workspace_bytes(int32_t H, int32_t W, int32_t n) {
    if (!sg_lov_covered(H, W, n))
        return sgan_fail(SGAN_ERR_INVALID, "not covered: %d x %d pixels, %d classes (H, W >= 1, H W <= 2^20, 1 .. %d classes)", H, W, n,
                         SGAN_LOVASZ_MAX_CLASSES);
    return sg_lov_layout(nullptr, H, W, n).bytes;
}

extern "C" int sgan_lovasz_forward(const float* p, int64_t p_cs, int64_t p_rs, int64_t p_ps, const int64_t* label, const int32_t* classes,
                                   int32_t n, int32_t C, int32_t H, int32_t W, float* loss_out, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
    SG_LOV_COVERED(H, W, n);
    SG_REFUSE(p && label && classes && loss_out && workspace, "null pointer");
    SG_REFUSE(C >= 1 && C <= 64 && sg_lov_classes_ok(classes, n, C), "bad classes: %d distinct indices below C = %d (C <= 64) are needed", n, C);
    SG_REFUSE(sg_lov_strides_ok(H, W, p_cs, p_rs, p_ps), "bad strides %lld, %lld, %lld", (long long)p_cs, (long long)p_rs, (long long)p_ps);
    const SgLovWs w = sg_lov_layout(workspace, H, W, n);
    SG_REFUSE(workspace_bytes >= w.bytes, "workspace too small: %lld bytes, %lld needed (sgan_lovasz_workspace_bytes); nothing was launched",
              (long long)workspace_bytes, (long long)w.bytes);
    SG_REFUSE(((uintptr_t)workspace & 7) == 0, "workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    SgLovClasses cl;
    for (int a = 0; a < SGAN_LOVASZ_MAX_CLASSES; ++a) cl.cls[a] = a < n ? classes[a] : 0;
    const unsigned chunks = (unsigned)(w.P / SG_LOV_CHUNK), pairs = (unsigned)sg_cdiv(w.P / 2, SG_LOV_THREADS);
    hipLaunchKernelGGL(sg_lov_sort_chunk_kernel, dim3(chunks, n), dim3(SG_LOV_SORT_THREADS), 0, st, p, p_cs, p_rs, p_ps, label, cl, W, w.N, w.P,
                       w.keys);
    SGAN_LAUNCH_CHECK();
    for (uint64_t k = 2ull * SG_LOV_CHUNK; k <= (uint64_t)w.P; k <<= 1) {
        for (uint64_t j = k >> 1; j >= SG_LOV_CHUNK; j >>= 1) {
            hipLaunchKernelGGL(sg_lov_merge_global_kernel, dim3(pairs, n), dim3(SG_LOV_THREADS), 0, st, w.keys, w.P, k, j);
            SGAN_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sg_lov_merge_chunk_kernel, dim3(chunks, n), dim3(SG_LOV_SORT_THREADS), 0, st, w.keys, w.P, k);
        SGAN_LAUNCH_CHECK();
    }
    int32_t* G = (int32_t*)(w.state + 24);
    hipLaunchKernelGGL(sg_lov_count_kernel, dim3((unsigned)w.nb, n), dim3(SG_LOV_THREADS), 0, st, (const unsigned long long*)w.keys, w.P, w.N,
                       (int)w.nb, w.bsum);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_lov_offsets_kernel, dim3(n), dim3(SG_LOV_THREADS), 0, st, w.bsum, (int)w.nb, G);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_lov_weights_kernel, dim3((unsigned)w.nb, n), dim3(SG_LOV_THREADS), 0, st, (const unsigned long long*)w.keys, w.P, w.N,
                       (int)w.nb, (const int32_t*)w.bsum, (const int32_t*)G, w.perm, w.g, w.slots);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_lov_finish_kernel, dim3(1), dim3(SG_LOV_THREADS), 0, st, (const double*)w.slots, (int)w.nb, n, w.state, loss_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_lov_finish_kernel";
    return SGAN_OK;
}

extern "C" int sgan_lovasz_backward(const float* p, int64_t p_cs, int64_t p_rs, int64_t p_ps, const int32_t* classes, int32_t n, int32_t C,
                                    int32_t H, int32_t W, const float* gout, float* dp, const void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    SG_LOV_COVERED(H, W, n);
    SG_REFUSE(p && classes && dp && workspace, "null pointer");
    SG_REFUSE(C >= 1 && C <= 64 && sg_lov_classes_ok(classes, n, C), "bad classes: %d distinct indices below C = %d (C <= 64) are needed", n, C);
    SG_REFUSE(sg_lov_strides_ok(H, W, p_cs, p_rs, p_ps), "bad strides %lld, %lld, %lld", (long long)p_cs, (long long)p_rs, (long long)p_ps);
    const SgLovWs w = sg_lov_layout((void*)workspace, H, W, n);
    SG_REFUSE(workspace_bytes >= w.bytes, "workspace too small: %lld bytes, %lld needed (sgan_lovasz_workspace_bytes); nothing was launched",
              (long long)workspace_bytes, (long long)w.bytes);
    SG_REFUSE(((uintptr_t)workspace & 7) == 0, "workspace not 8-byte aligned");
    SgLovChannels ch;
    for (int a = 0; a < 64; ++a) ch.slot[a] = -1;
    for (int a = 0; a < n; ++a) ch.slot[classes[a]] = a;
    hipLaunchKernelGGL(sg_lov_bwd_kernel, dim3((unsigned)sg_cdiv(w.N, SG_LOV_THREADS), C), dim3(SG_LOV_THREADS), 0, (hipStream_t)stream, p, p_cs,
                       p_rs, p_ps, ch, W, w.N, w.P, (const unsigned long long*)w.keys, (const double*)w.g, (const double*)w.state, gout, dp);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_lov_bwd_kernel";
    return SGAN_OK;
}
