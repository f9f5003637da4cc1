// Sliced Wasserstein distance between two image sets over Laplacian-pyramid patches (swd.py; include/sgan_hip.h, "sliced Wasserstein
// distance"): the mirror-border pyramid step, the patch gather with its fp64 statistics, and the distances -- project, sort, compare.
// No kernel of this file uses an atomic: every sum is taken in an order the launch shape fixes, so every result has the same bits on
// every run.  DESIGN.md §R26.
#include "sgan_reduce.h"
#include "sgan_swd.h"

#define SG_SWD_MAX_J 4096
#define SG_SWD_CHUNK_J 512      // directions whose projections the workspace holds at a time
#define SG_SWD_ERR_POS 128      // dev_err: a patch position outside the level

// ---- pyramid step ---------------------------------------------------------------------------------------------------------------------
// scipy's mode='mirror' on [0, n): d c b | a b c d | c b a.  |i| overshoots by at most 2 and n >= 4, so one reflection is enough.
__device__ __forceinline__ int sg_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// b = [1 4 6 4 1] / 16; the products b[i] b[j] and 4 b[i] b[j] are exact in fp32
__device__ __forceinline__ float sg_b5(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

// out[c][y][x] = sum_{dy,dx} g[dy][dx] in[c][mirror(2y + dy - 2)][mirror(2x + dx - 2)]: 25 terms, rows first
__global__ __launch_bounds__(256) void sg_lap_down_kernel(const float* __restrict__ in, int64_t in_ld, int64_t in_plane, int H, int W,
                                                          float* __restrict__ out, int64_t out_ld, int64_t out_plane) {
    const int Ho = H >> 1, Wo = W >> 1;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= Ho * Wo) return;
    const int y = o / Wo, x = o - y * Wo;
    const float* p = in + (int64_t)blockIdx.y * in_plane;
    int xs[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) xs[d] = sg_mirror(2 * x + d - 2, W);
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float* row = p + (int64_t)sg_mirror(2 * y + dy - 2, H) * in_ld;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) acc = fmaf(sg_b5(dy) * sg_b5(dx), row[xs[dx]], acc);
    }
    out[(int64_t)blockIdx.y * out_plane + (int64_t)y * out_ld + x] = acc;
}

// out[c][Y][X] = fine[c][Y][X] - sum 4 g[dy][dx] z[mirror(Y + dy - 2)][mirror(X + dx - 2)], z the coarse plane on the even sites of a
// zero plane of the fine size.  The mirror keeps parity, so only the taps that land on even sites count: 4, 6 or 9 of them.
__global__ __launch_bounds__(256) void sg_lap_up_sub_kernel(const float* __restrict__ fine, int64_t fine_ld, int64_t fine_plane,
                                                            const float* __restrict__ coarse, int64_t coarse_ld, int64_t coarse_plane, int H,
                                                            int W, float* __restrict__ out, int64_t out_ld, int64_t out_plane) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= H * W) return;
    const int Y = o / W, X = o - Y * W;
    const float* q = coarse + (int64_t)blockIdx.y * coarse_plane;
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const int yy = sg_mirror(Y + dy - 2, H);
        if (yy & 1) continue;
        const float* row = q + (int64_t)(yy >> 1) * coarse_ld;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            const int xx = sg_mirror(X + dx - 2, W);
            if (xx & 1) continue;
            acc = fmaf(4.f * (sg_b5(dy) * sg_b5(dx)), row[xx >> 1], acc);
        }
    }
    const float g = fine[(int64_t)blockIdx.y * fine_plane + (int64_t)Y * fine_ld + X];
    out[(int64_t)blockIdx.y * out_plane + (int64_t)Y * out_ld + X] = g - acc;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------
// Workgroup c copies channel c of the P patches and sums it.  One workgroup owns one channel's two accumulators, and the calls of a
// stream follow each other, so the accumulators grow in image order without a hand-off between workgroups.
__global__ __launch_bounds__(256) void sg_swd_gather_kernel(const float* __restrict__ img, int64_t ld, int64_t plane, int H, int W, int C,
                                                            const int32_t* __restrict__ pos, int P, float* __restrict__ desc, int row0,
                                                            double* __restrict__ acc, int32_t* __restrict__ dev_err) {
    __shared__ double red[4];
    __shared__ int any_bad;
    const int c = blockIdx.x, K = C * SG_SWD_TAPS;
    if (threadIdx.x == 0) any_bad = 0;
    SG_SYNC();
    const float* p = img + (int64_t)c * plane;
    double s = 0.0, q = 0.0;
    int bad = 0;
    for (int e = threadIdx.x; e < P * SG_SWD_TAPS; e += 256) {
        const int r = e / SG_SWD_TAPS, t = e - r * SG_SWD_TAPS;
        const int dy = t / SG_SWD_PATCH, dx = t - dy * SG_SWD_PATCH;
        const int y = pos[3 * r + 1], x = pos[3 * r + 2];
        float v = 0.f;
        if (y >= 0 && y <= H - SG_SWD_PATCH && x >= 0 && x <= W - SG_SWD_PATCH) v = p[(int64_t)(y + dy) * ld + (x + dx)];
        else bad = 1;
        desc[(int64_t)(row0 + r) * K + c * SG_SWD_TAPS + t] = v;
        s += (double)v;
        q += (double)v * (double)v;
    }
    if (bad) any_bad = 1;
    s = sg_block_sum<4>(s, red);
    SG_SYNC();
    q = sg_block_sum<4>(q, red);
    if (threadIdx.x == 0) {
        acc[c] += s;
        acc[C + c] += q;
        if (any_bad && c == 0) *dev_err |= SG_SWD_ERR_POS;      // every workgroup sees the same positions: one of them reports
    }
}

// ---- distances ------------------------------------------------------------------------------------------------------------------------
// the normalisation on load (sg_swd_norm, sg_swd_normalise) is sgan_swd.h's, shared with sgan_prd.hip
// Projection pass: proj[set][j - j0][i] = sum_k n_ik d_jk, k ascending, for a 64 x 64 tile of (rows, directions) per workgroup, one
// channel (49 values of k) staged at a time.  A thread owns rows ti + 16 a and directions 4 tj + b; the sum of one (row, direction)
// is the same chain of FMAs wherever the row stands, so equal rows give equal bits.
#define SG_SWD_PT 64
__global__ __launch_bounds__(256) void sg_swd_project_kernel(const float* __restrict__ descA, const float* __restrict__ descB,
                                                             const double* __restrict__ statsA, const double* __restrict__ statsB,
                                                             const float* __restrict__ dirs, int N, int C, int j0, int Jc,
                                                             float* __restrict__ proj) {
    __shared__ float As[SG_SWD_TAPS][SG_SWD_PT + 1];
    __shared__ float Ds[SG_SWD_TAPS][SG_SWD_PT + 1];
    const int K = C * SG_SWD_TAPS;
    const int set = blockIdx.z;
    const float* desc = set ? descB : descA;
    const double* stats = set ? statsB : statsA;
    const int i0 = blockIdx.x * SG_SWD_PT, jt = blockIdx.y * SG_SWD_PT;
    const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
    const double count = (double)N * (double)SG_SWD_TAPS;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int c = 0; c < C; ++c) {
        float m32, r32;
        sg_swd_norm(stats, C, c, count, m32, r32);
        SG_SYNC();
        for (int e = threadIdx.x; e < SG_SWD_PT * SG_SWD_TAPS; e += 256) {
            const int r = e / SG_SWD_TAPS, t = e - r * SG_SWD_TAPS;
            const int i = i0 + r, j = jt + r;
            As[t][r] = i < N ? sg_swd_normalise(desc[(int64_t)i * K + c * SG_SWD_TAPS + t], m32, r32) : 0.f;
            Ds[t][r] = j < Jc ? dirs[(int64_t)(j0 + j) * K + c * SG_SWD_TAPS + t] : 0.f;
        }
        SG_SYNC();
#pragma unroll 7
        for (int t = 0; t < SG_SWD_TAPS; ++t) {
            float av[4], dv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) av[a] = As[t][ti + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) dv[b] = Ds[t][4 * tj + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(av[a], dv[b], acc[a][b]);
        }
    }
    float* out = proj + (int64_t)set * Jc * N;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int j = jt + 4 * tj + b;
        if (j >= Jc) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + ti + 16 * a;
            if (i < N) out[(int64_t)j * N + i] = acc[a][b];
        }
    }
}

// Sort pass: one workgroup per direction.  Both projections sit in LDS, padded with +inf to NP = the power of two >= N (2 x 64 KiB at
// N = 16384, of the 160 KiB a workgroup may declare), and go through one bitonic network together: a stage has NP compare-exchanges,
// NP / 2 per array.  Then sum_i |sA_i - sB_i| over i < N in fp64: each thread its strided share, then the workgroup sum.
// FUSED: no projection pass; every thread projects its rows itself (the descriptor matrices are then read once per direction).
template <int NP>
struct SgSwdShape {
    static constexpr int T = NP / 2 < 64 ? 64 : (NP / 2 > 1024 ? 1024 : NP / 2);
};

template <int NP, bool FUSED>
__global__ __launch_bounds__(SgSwdShape<NP>::T) void sg_swd_sort_kernel(const float* __restrict__ proj, const float* __restrict__ descA,
                                                                         const float* __restrict__ descB, const double* __restrict__ statsA,
                                                                         const double* __restrict__ statsB, const float* __restrict__ dirs,
                                                                         int N, int C, int j0, int Jc, double* __restrict__ out) {
    constexpr int T = SgSwdShape<NP>::T;
    __shared__ float S[2 * NP];      // [0, NP): set A, [NP, 2 NP): set B
    __shared__ double red[T / 64];
    const int jj = blockIdx.x, tid = threadIdx.x;
    if constexpr (FUSED) {
        __shared__ float D[3 * SG_SWD_TAPS];
        __shared__ float MR[2][3][2];
        const int K = C * SG_SWD_TAPS;
        for (int k = tid; k < K; k += T) D[k] = dirs[(int64_t)(j0 + jj) * K + k];
        if (tid < 2 * C) {
            const int set = tid / C, c = tid - set * C;
            sg_swd_norm(set ? statsB : statsA, C, c, (double)N * (double)SG_SWD_TAPS, MR[set][c][0], MR[set][c][1]);
        }
        SG_SYNC();
        for (int e = tid; e < 2 * NP; e += T) {
            const int set = e / NP, i = e - set * NP;
            float v = __builtin_inff();
            if (i < N) {
                const float* row = (set ? descB : descA) + (int64_t)i * K;
                v = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float m32 = MR[set][c][0], r32 = MR[set][c][1];
                    for (int t = 0; t < SG_SWD_TAPS; ++t)
                        v = fmaf(sg_swd_normalise(row[c * SG_SWD_TAPS + t], m32, r32), D[c * SG_SWD_TAPS + t], v);
                }
            }
            S[e] = v;
        }
    } else {
        for (int e = tid; e < 2 * NP; e += T) {
            const int set = e / NP, i = e - set * NP;
            S[e] = i < N ? proj[((int64_t)set * Jc + jj) * N + i] : __builtin_inff();
        }
    }
    SG_SYNC();
    for (int k = 2; k <= NP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < NP; p += T) {
                const int set = p / (NP / 2), qq = p - set * (NP / 2);
                const int lo = ((qq & ~(j - 1)) << 1) | (qq & (j - 1));
                const int ia = set * NP + lo, ib = ia + j;
                const float a = S[ia], b = S[ib];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) {
                    S[ia] = b;
                    S[ib] = a;
                }
            }
            SG_SYNC();
        }
    }
    double acc = 0.0;
    for (int i = tid; i < N; i += T) acc += fabs((double)S[i] - (double)S[NP + i]);      // exact: the only roundings are the projections' and this sum's
    acc = sg_block_sum<T / 64>(acc, red);
    if (tid == 0) out[j0 + jj] = acc / (double)N;
}

static bool sg_swd_covered(int32_t N, int32_t K, int32_t J) {
    return N >= 1 && N <= SG_SWD_MAX_N && sg_swd_channels(K) && J >= 1 && J <= SG_SWD_MAX_J;
}

template <int NP>
static void sg_swd_sort_launch(bool fused, int Jc, hipStream_t st, const float* proj, const float* dA, const float* dB, const double* sA,
                               const double* sB, const float* dirs, int N, int C, int j0, double* out) {
    if (fused) hipLaunchKernelGGL((sg_swd_sort_kernel<NP, true>), dim3(Jc), dim3(SgSwdShape<NP>::T), 0, st, proj, dA, dB, sA, sB, dirs, N, C, j0, Jc, out);
    else hipLaunchKernelGGL((sg_swd_sort_kernel<NP, false>), dim3(Jc), dim3(SgSwdShape<NP>::T), 0, st, proj, dA, dB, sA, sB, dirs, N, C, j0, Jc, out);
}

extern "C" int sgan_lap_pyramid(int32_t mode, const float* fine, int64_t fine_ld, const float* coarse, int64_t coarse_ld, int32_t C,
                                int32_t H, int32_t W, float* out, int64_t out_ld, void* stream) {
    SGAN_CHECK(mode == SGAN_LAP_DOWN || mode == SGAN_LAP_UP_SUB, "mode %d (0 = down, 1 = up and subtract)", mode);
    SGAN_CHECK(fine && out && (mode == SGAN_LAP_DOWN || coarse), "null pointer");
    SGAN_CHECK(C >= 1 && C <= 65535 && H >= 4 && W >= 4 && !(H & 1) && !(W & 1) && (int64_t)H * W < (1ll << 30),
               "bad shape %d x %d x %d: both sides even and >= 4, H W < 2^30, at most 65535 planes", C, H, W);
    const int Ho = H / 2, Wo = W / 2;
    const int64_t out_w = mode == SGAN_LAP_DOWN ? Wo : W;
    SGAN_CHECK(fine_ld >= W && out_ld >= out_w && (mode == SGAN_LAP_DOWN || coarse_ld >= Wo), "a row pitch is shorter than its row");
    hipStream_t st = (hipStream_t)stream;
    if (mode == SGAN_LAP_DOWN) {
        hipLaunchKernelGGL(sg_lap_down_kernel, dim3((Ho * Wo + 255) / 256, C), dim3(256), 0, st, fine, fine_ld, fine_ld * H, H, W, out, out_ld,
                           out_ld * Ho);
        g_sgan_last_kernel = "sg_lap_down_kernel";
    } else {
        hipLaunchKernelGGL(sg_lap_up_sub_kernel, dim3((H * W + 255) / 256, C), dim3(256), 0, st, fine, fine_ld, fine_ld * H, coarse, coarse_ld,
                           coarse_ld * Ho, H, W, out, out_ld, out_ld * H);
        g_sgan_last_kernel = "sg_lap_up_sub_kernel";
    }
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_swd_gather(const float* img, int64_t ld, int32_t C, int32_t H, int32_t W, const int32_t* pos, int32_t P, float* desc,
                               int32_t row0, int32_t rows, double* acc, int32_t* dev_err, void* stream) {
    SGAN_CHECK(img && pos && desc && acc && dev_err, "null pointer");
    SGAN_CHECK(C >= 1 && C <= 3 && H >= SG_SWD_PATCH && W >= SG_SWD_PATCH && (int64_t)H * W < (1ll << 30) && ld >= W,
               "bad shape %d x %d x %d (1..3 planes, sides >= 7, H W < 2^30) or row pitch %lld", C, H, W, (long long)ld);
    SGAN_CHECK(P >= 1 && row0 >= 0 && rows <= SG_SWD_MAX_N && (int64_t)row0 + P <= rows,
               "rows [%d, %d + %d) do not lie in a descriptor matrix of %d rows (at most %d)", row0, row0, P, rows, SG_SWD_MAX_N);
    hipLaunchKernelGGL(sg_swd_gather_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, img, ld, ld * H, H, W, C, pos, P, desc, row0, acc,
                       dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_swd_gather_kernel";
    return SGAN_OK;
}

extern "C" int64_t sgan_swd_workspace(int32_t N, int32_t K, int32_t J) {
    if (!sg_swd_covered(N, K, J))
        return sgan_fail(SGAN_ERR_UNSUPPORTED, "swd distances cover 1 <= N <= %d, K in {49, 98, 147}, 1 <= J <= %d; got N %d, K %d, J %d",
                         SG_SWD_MAX_N, SG_SWD_MAX_J, N, K, J);
    const int64_t jc = J < SG_SWD_CHUNK_J ? J : SG_SWD_CHUNK_J;
    return ((2 * jc * (int64_t)N * 4 + 15) / 16) * 16;
}

extern "C" int sgan_swd_distances(const float* descA, const float* descB, const double* statsA, const double* statsB, const float* dirs,
                                  int32_t N, int32_t K, int32_t J, double* out, void* workspace, int64_t workspace_bytes, int32_t variant,
                                  void* stream) {
    SGAN_CHECK(descA && descB && statsA && statsB && dirs && out && workspace, "null pointer");
    const int64_t need = sgan_swd_workspace(N, K, J);
    if (need < 0) return SGAN_ERR_UNSUPPORTED;      // the message is set
    SGAN_CHECK(variant >= SGAN_SWD_AUTO && variant <= SGAN_SWD_FUSED, "variant %d (0 = auto, 1 = split, 2 = fused)", variant);
    SGAN_CHECK(workspace_bytes >= need, "workspace of %lld bytes, %lld needed for N %d, K %d, J %d (sgan_swd_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)need, N, K, J);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    const bool fused = variant == SGAN_SWD_FUSED;
    const int C = sg_swd_channels(K);
    float* proj = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    int NP = 64;
    while (NP < N) NP <<= 1;
    for (int j0 = 0; j0 < J; j0 += SG_SWD_CHUNK_J) {
        const int Jc = J - j0 < SG_SWD_CHUNK_J ? J - j0 : SG_SWD_CHUNK_J;
        if (!fused) {
            hipLaunchKernelGGL(sg_swd_project_kernel, dim3((N + SG_SWD_PT - 1) / SG_SWD_PT, (Jc + SG_SWD_PT - 1) / SG_SWD_PT, 2), dim3(256), 0, st,
                               descA, descB, statsA, statsB, dirs, N, C, j0, Jc, proj);
            SGAN_LAUNCH_CHECK();
        }
        switch (NP) {
            case 64: sg_swd_sort_launch<64>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 128: sg_swd_sort_launch<128>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 256: sg_swd_sort_launch<256>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 512: sg_swd_sort_launch<512>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 1024: sg_swd_sort_launch<1024>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 2048: sg_swd_sort_launch<2048>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 4096: sg_swd_sort_launch<4096>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            case 8192: sg_swd_sort_launch<8192>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
            default: sg_swd_sort_launch<16384>(fused, Jc, st, proj, descA, descB, statsA, statsB, dirs, N, C, j0, out); break;
        }
        SGAN_LAUNCH_CHECK();
    }
    g_sgan_last_kernel = "sg_swd_sort_kernel";
    return SGAN_OK;
}
