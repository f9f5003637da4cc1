// Soft-clDice loss term (include/sgan_hip.h, "soft-clDice"): the soft skeleton of a plane by iterated min / max
// selections, the four sums and the loss, and the gradient of the loss with respect to the probability plane.
//
// Planes of the workspace, dense [H * W] floats each, n = H W:
//   I_0 .. I_{K+1}   the input and its K + 1 erosions                       (forward; read again by the backward)
//   E_0 .. E_K       d L / d delta_j behind the relu's mask                 (backward)
//   G_a, G_b         d L / d I_j of the level in work and of the one before (backward, ping-pong)
// Forward: K + 1 launches erode (the first also copies the strided input to I_0), one launch walks the K + 1 levels per pixel
//   and writes S_K.  Nothing is rounded before delta: every I_j holds bits of the input.
// Finish: one launch of <= 64 workgroups sums A, B, C, D in fp64 (sg_block_sum, one slot per workgroup and sum, sg_publish_last);
//   the last workgroup adds the slots in order and writes the sums, L and the three scalar derivatives.
// Backward: one launch writes the E planes, then one launch per level j = K + 1 .. 0 GATHERS
//   G_j(x) = E_j(x) - sum over the <= 9 dilate windows y that select x in I_j of E_{j-1}(y)
//                   + sum over the <= 5 erode windows y that select x in I_j of G_{j+1}(y)
//   with every window's selection recomputed from I_j in the stated order (first pixel that attains the extreme wins).  The sum
//   runs in the order of the tables below; no atomics, no saved indices: the same bits on every run.  The level-0 launch writes
//   dp = gout (G_0 + gC S(T)).
// Every launch's grid depends on (H, W) alone and their number on K alone; scalars stay on the device.
#include "sgan_common.h"
#include "sgan_reduce.h"

#define SG_CLD_THREADS 256
#define SG_CLD_BLOCKS 64             // workgroups of the finish launch, at most: the slots of the state
#define SG_CLD_MAX_DIM 32768
#define SG_CLD_LEVELS (SGAN_CLDICE_MAX_ITERS + 1)

#define SG_REFUSE(cond, ...)                            \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

// the plus neighbourhood in the order centre, up, left, right, down; the 3 x 3 box centre first, then row-major
__device__ static const signed char SG_CLD_EDY[5] = {0, -1, 0, 0, 1};
__device__ static const signed char SG_CLD_EDX[5] = {0, 0, -1, 1, 0};
__device__ static const signed char SG_CLD_DDY[9] = {0, -1, -1, -1, 0, 0, 1, 1, 1};
__device__ static const signed char SG_CLD_DDX[9] = {0, -1, 0, 1, -1, 1, -1, 0, 1};

// min over the in-image plus neighbourhood of (y, x) in the dense plane I; *sel = the position in the order that attains it first
__device__ __forceinline__ float sg_cld_erode_at(const float* __restrict__ I, int y, int x, int H, int W, int* sel) {
    float m = I[(int64_t)y * W + x];
    int s = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const int yy = y + SG_CLD_EDY[k], xx = x + SG_CLD_EDX[k];
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const float v = I[(int64_t)yy * W + xx];
        if (v < m) {
            m = v;
            s = k;
        }
    }
    *sel = s;
    return m;
}

// max over the in-image 3 x 3 box
__device__ __forceinline__ float sg_cld_dilate_at(const float* __restrict__ I, int y, int x, int H, int W, int* sel) {
    float m = I[(int64_t)y * W + x];
    int s = 0;
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const int yy = y + SG_CLD_DDY[k], xx = x + SG_CLD_DDX[k];
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const float v = I[(int64_t)yy * W + xx];
        if (v > m) {
            m = v;
            s = k;
        }
    }
    *sel = s;
    return m;
}

// dst = erode(src); with copy != null the strided src is also copied there (I_0), and the erosion reads the strided plane
__global__ __launch_bounds__(SG_CLD_THREADS) void sg_cld_erode_kernel(const float* __restrict__ src, int64_t rs, int64_t ps, int H, int W,
                                                                      float* __restrict__ copy, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * SG_CLD_THREADS + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    float m = src[y * rs + x * ps];
    if (copy) copy[i] = m;
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const int yy = y + SG_CLD_EDY[k], xx = x + SG_CLD_EDX[k];
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        m = fminf(m, src[yy * rs + xx * ps]);
    }
    dst[i] = m;
}

// delta_j = max(I_j - dilate(I_{j+1}), 0) of pixel (y, x)
__device__ __forceinline__ float sg_cld_delta(const float* __restrict__ planes, int64_t n, int j, int64_t i, int y, int x, int H, int W) {
    int sel;
    const float d = sg_cld_dilate_at(planes + (int64_t)(j + 1) * n, y, x, H, W, &sel);
    return fmaxf(planes[(int64_t)j * n + i] - d, 0.f);
}

__global__ __launch_bounds__(SG_CLD_THREADS) void sg_cld_skel_kernel(const float* __restrict__ planes, int H, int W, int K, float* __restrict__ skel) {
    const int64_t n = (int64_t)H * W, i = (int64_t)blockIdx.x * SG_CLD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i % W);
    float S = sg_cld_delta(planes, n, 0, i, y, x, H, W);
    for (int j = 1; j <= K; ++j) {
        const float d = sg_cld_delta(planes, n, j, i, y, x, H, W);
        S = S + d * (1.f - S);
    }
    skel[i] = S;
}

// state (doubles): [0..3] A, B, C, D  [4] L  [5] gA  [6] gB  [7] gC  [8 + k * SG_CLD_BLOCKS + b] the slot of sum k, workgroup b;
// the ticket is the unsigned at double 8 + 4 * SG_CLD_BLOCKS
__global__ __launch_bounds__(SG_CLD_THREADS) void sg_cld_finish_kernel(const float* __restrict__ sp, const float* __restrict__ t, int64_t t_rs,
                                                                       int64_t t_ps, const float* __restrict__ st, const float* __restrict__ p,
                                                                       int64_t p_rs, int64_t p_ps, int H, int W, double* state, float* loss_out) {
    __shared__ double red[4][SG_CLD_THREADS / 64];
    __shared__ int last_lds;
    const int64_t n = (int64_t)H * W;
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SG_CLD_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_CLD_THREADS) {
        const int y = (int)(i / W), x = (int)(i % W);
        const double s = (double)sp[i], u = (double)st[i];
        a += s * (double)t[y * t_rs + x * t_ps];
        b += s;
        c += u * (double)p[y * p_rs + x * p_ps];
        d += u;
    }
    a = sg_block_sum<4>(a, red[0]);
    b = sg_block_sum<4>(b, red[1]);
    c = sg_block_sum<4>(c, red[2]);
    d = sg_block_sum<4>(d, red[3]);
    double* slots = state + 8;
    unsigned* ticket = (unsigned*)(state + 8 + 4 * SG_CLD_BLOCKS);
    if (threadIdx.x == 0) {
        slots[0 * SG_CLD_BLOCKS + blockIdx.x] = a;
        slots[1 * SG_CLD_BLOCKS + blockIdx.x] = b;
        slots[2 * SG_CLD_BLOCKS + blockIdx.x] = c;
    }
    if (!sg_publish_last(d, &slots[3 * SG_CLD_BLOCKS + blockIdx.x], ticket, gridDim.x - 1, &last_lds)) return;
    if (threadIdx.x != 0) return;
    __threadfence();
    double v[4];
    for (int k = 0; k < 4; ++k) {
        double sum = 0.0;
        for (unsigned g = 0; g < gridDim.x; ++g) sum += sg_slot_load(&slots[k * SG_CLD_BLOCKS + g]);
        v[k] = sum;
    }
    const double A = v[0], B = v[1], C = v[2], D = v[3];
    const double tp = (A + 1.0) / (B + 1.0), ts = (C + 1.0) / (D + 1.0);
    const double L = 1.0 - 2.0 * tp * ts / (tp + ts);
    const double dLdp = -2.0 * ts * ts / ((tp + ts) * (tp + ts)), dLds = -2.0 * tp * tp / ((tp + ts) * (tp + ts));
    state[0] = A;
    state[1] = B;
    state[2] = C;
    state[3] = D;
    state[4] = L;
    state[5] = dLdp / (B + 1.0);                                // d L / d S(P)(x) = gA T(x) + gB
    state[6] = -dLdp * (A + 1.0) / ((B + 1.0) * (B + 1.0));
    state[7] = dLds / (D + 1.0);                                // the direct term: d L / d P(x) += gC S(T)(x)
    loss_out[0] = (float)L;
    ticket[0] = 0u;
}

// E_j = d L / d delta_j where delta_j > 0, else 0, for every level, from d L / d S_K = gA T + gB
__global__ __launch_bounds__(SG_CLD_THREADS) void sg_cld_bwd_delta_kernel(const float* __restrict__ planes, const float* __restrict__ t, int64_t t_rs,
                                                                          int64_t t_ps, const double* __restrict__ state, int H, int W, int K,
                                                                          float* __restrict__ E) {
    const int64_t n = (int64_t)H * W, i = (int64_t)blockIdx.x * SG_CLD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / W), x = (int)(i % W);
    float dl[SG_CLD_LEVELS], sb[SG_CLD_LEVELS];      // delta_j and S_{j-1}; every index below is static
    float S = 0.f;
#pragma unroll
    for (int j = 0; j < SG_CLD_LEVELS; ++j) {
        if (j <= K) {
            dl[j] = sg_cld_delta(planes, n, j, i, y, x, H, W);
            sb[j] = S;
            S = j ? S + dl[j] * (1.f - S) : dl[0];
        }
    }
    float g = (float)state[5] * t[y * t_rs + x * t_ps] + (float)state[6];
#pragma unroll
    for (int j = SG_CLD_LEVELS - 1; j >= 1; --j) {
        if (j <= K) {
            E[(int64_t)j * n + i] = dl[j] > 0.f ? g * (1.f - sb[j]) : 0.f;
            g = g * (1.f - dl[j]);
        }
    }
    E[i] = dl[0] > 0.f ? g : 0.f;
}

// one level of the backward, see the head of the file.  Ej, Eprev, Gnext may each be null (the levels K + 1 and 0 lack one);
// st != null marks level 0: out = gout (G_0 + gC st), gout null = 1
__global__ __launch_bounds__(SG_CLD_THREADS) void sg_cld_bwd_gather_kernel(const float* __restrict__ I, const float* __restrict__ Ej,
                                                                           const float* __restrict__ Eprev, const float* __restrict__ Gnext, int H,
                                                                           int W, const float* __restrict__ st, const double* __restrict__ state,
                                                                           const float* __restrict__ gout, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SG_CLD_THREADS + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    float g = Ej ? Ej[i] : 0.f;
    if (Eprev) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {      // the window centred at (y, x) - offset k holds (y, x) at position k
            const int yy = y - SG_CLD_DDY[k], xx = x - SG_CLD_DDX[k];
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float e = Eprev[(int64_t)yy * W + xx];
            if (e == 0.f) continue;      // nothing to hand on: the selection need not be known
            int sel;
            sg_cld_dilate_at(I, yy, xx, H, W, &sel);
            if (sel == k) g -= e;
        }
    }
    if (Gnext) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int yy = y - SG_CLD_EDY[k], xx = x - SG_CLD_EDX[k];
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float e = Gnext[(int64_t)yy * W + xx];
            if (e == 0.f) continue;
            int sel;
            sg_cld_erode_at(I, yy, xx, H, W, &sel);
            if (sel == k) g += e;
        }
    }
    if (st) {
        g = g + (float)state[7] * st[i];
        if (gout) g = g * gout[0];
    }
    out[i] = g;
}

static bool sg_cld_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= SG_CLD_MAX_DIM && W <= SG_CLD_MAX_DIM && (int64_t)H * W < (1ll << 30);
}

static bool sg_cld_iters_ok(int32_t iters) { return iters >= 1 && iters <= SGAN_CLDICE_MAX_ITERS; }

static bool sg_cld_strides_ok(int32_t H, int32_t W, int64_t rs, int64_t ps) { return ps >= 1 && (H == 1 || rs >= (int64_t)(W - 1) * ps + 1); }

static int64_t sg_cld_bytes(int32_t H, int32_t W, int32_t iters, bool bwd) {
    return 4ll * H * W * ((iters + 2) + (bwd ? iters + 3 : 0));
}

static unsigned sg_cld_grid(int32_t H, int32_t W) { return (unsigned)sg_cdiv((int64_t)H * W, SG_CLD_THREADS); }

extern "C" int64_t sgan_cldice_workspace_bytes(int32_t H, int32_t W, int32_t iters, int32_t with_backward) {
    if (!sg_cld_iters_ok(iters)) return sgan_fail(SGAN_ERR_INVALID, "not covered: %d iterations (1..%d)", iters, SGAN_CLDICE_MAX_ITERS);
    if (!sg_cld_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_cld_bytes(H, W, iters, with_backward != 0);
}

extern "C" int sgan_soft_skeleton(const float* x, int64_t x_rs, int64_t x_ps, int32_t H, int32_t W, int32_t iters, float* skel,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    SG_REFUSE(sg_cld_iters_ok(iters), "not covered: %d iterations (1..%d)", iters, SGAN_CLDICE_MAX_ITERS);
    SG_REFUSE(x && skel && workspace, "null pointer");
    SG_REFUSE(sg_cld_shape_ok(H, W) && sg_cld_strides_ok(H, W, x_rs, x_ps), "bad shape %d x %d (H, W <= %d, H W < 2^30), strides %lld, %lld", H, W,
              SG_CLD_MAX_DIM, (long long)x_rs, (long long)x_ps);
    SG_REFUSE(workspace_bytes >= sg_cld_bytes(H, W, iters, false), "workspace of %lld bytes, %lld needed (sgan_cldice_workspace_bytes); nothing was "
              "launched", (long long)workspace_bytes, (long long)sg_cld_bytes(H, W, iters, false));
    SG_REFUSE(((uintptr_t)workspace & 3) == 0, "workspace not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    float* planes = (float*)workspace;
    const dim3 grid(sg_cld_grid(H, W)), block(SG_CLD_THREADS);
    hipLaunchKernelGGL(sg_cld_erode_kernel, grid, block, 0, st, x, x_rs, x_ps, H, W, planes, planes + n);
    SGAN_LAUNCH_CHECK();
    for (int j = 1; j <= iters; ++j) {
        hipLaunchKernelGGL(sg_cld_erode_kernel, grid, block, 0, st, (const float*)(planes + j * n), (int64_t)W, (int64_t)1, H, W, (float*)nullptr,
                           planes + (j + 1) * n);
        SGAN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sg_cld_skel_kernel, grid, block, 0, st, (const float*)planes, H, W, iters, skel);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_cld_skel_kernel";
    return SGAN_OK;
}

extern "C" int sgan_cldice_finish(const float* sp, const float* t, int64_t t_rs, int64_t t_ps, const float* st, const float* p, int64_t p_rs,
                                  int64_t p_ps, int32_t H, int32_t W, double* state, float* loss_out, void* stream) {
    SG_REFUSE(sp && t && st && p && state && loss_out, "null pointer");
    SG_REFUSE(sg_cld_shape_ok(H, W) && sg_cld_strides_ok(H, W, t_rs, t_ps) && sg_cld_strides_ok(H, W, p_rs, p_ps),
              "bad shape %d x %d (H, W <= %d, H W < 2^30) or strides", H, W, SG_CLD_MAX_DIM);
    SG_REFUSE(((uintptr_t)state & 7) == 0, "state not 8-byte aligned");
    const unsigned want = sg_cld_grid(H, W);
    hipLaunchKernelGGL(sg_cld_finish_kernel, dim3(want < SG_CLD_BLOCKS ? want : SG_CLD_BLOCKS), dim3(SG_CLD_THREADS), 0, (hipStream_t)stream, sp, t,
                       t_rs, t_ps, st, p, p_rs, p_ps, H, W, state, loss_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_cld_finish_kernel";
    return SGAN_OK;
}

extern "C" int sgan_cldice_backward(const float* t, int64_t t_rs, int64_t t_ps, const float* st, const double* state, const float* gout, int32_t H,
                                    int32_t W, int32_t iters, float* dp, void* workspace, int64_t workspace_bytes, void* stream) {
    SG_REFUSE(sg_cld_iters_ok(iters), "not covered: %d iterations (1..%d)", iters, SGAN_CLDICE_MAX_ITERS);
    SG_REFUSE(t && st && state && dp && workspace, "null pointer");
    SG_REFUSE(sg_cld_shape_ok(H, W) && sg_cld_strides_ok(H, W, t_rs, t_ps), "bad shape %d x %d (H, W <= %d, H W < 2^30), strides %lld, %lld", H, W,
              SG_CLD_MAX_DIM, (long long)t_rs, (long long)t_ps);
    SG_REFUSE(workspace_bytes >= sg_cld_bytes(H, W, iters, true), "workspace of %lld bytes, %lld needed (sgan_cldice_workspace_bytes with the "
              "backward); nothing was launched", (long long)workspace_bytes, (long long)sg_cld_bytes(H, W, iters, true));
    SG_REFUSE(((uintptr_t)workspace & 3) == 0, "workspace not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const int K = iters;
    const float* planes = (const float*)workspace;
    float* E = (float*)workspace + (int64_t)(K + 2) * n;
    float* G[2] = {E + (int64_t)(K + 1) * n, E + (int64_t)(K + 2) * n};
    const dim3 grid(sg_cld_grid(H, W)), block(SG_CLD_THREADS);
    hipLaunchKernelGGL(sg_cld_bwd_delta_kernel, grid, block, 0, s, planes, t, t_rs, t_ps, state, H, W, K, E);
    SGAN_LAUNCH_CHECK();
    for (int j = K + 1; j >= 0; --j) {      // G_j into G[j & 1], reading G_{j+1} from the other one
        const float* Ej = j <= K ? E + (int64_t)j * n : nullptr;
        const float* Eprev = j >= 1 ? E + (int64_t)(j - 1) * n : nullptr;
        const float* Gnext = j <= K ? G[(j + 1) & 1] : nullptr;
        hipLaunchKernelGGL(sg_cld_bwd_gather_kernel, grid, block, 0, s, planes + (int64_t)j * n, Ej, Eprev, Gnext, H, W, j == 0 ? st : nullptr, state,
                           gout, j == 0 ? dp : G[j & 1]);
        SGAN_LAUNCH_CHECK();
    }
    g_sgan_last_kernel = "sg_cld_bwd_gather_kernel";
    return SGAN_OK;
}
