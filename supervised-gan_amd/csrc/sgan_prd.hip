// Precision / recall / density / coverage of two patch-descriptor sets by k-nearest-neighbour balls (swd.py --prd_k; include/sgan_hip.h,
// "precision, recall, density, coverage"): the all-pairs squared-distance pass with its two row-wise epilogues, the row norms of the Gram
// form, and the integer finish.  No kernel of this file uses an atomic and no result crosses workgroups: a workgroup owns 64 query rows,
// walks every reference column and finishes its rows itself, so every result has the same bits on every run.  DESIGN.md §R27.
#include "sgan_reduce.h"
#include "sgan_swd.h"

#define SG_PRD_T 64             // query rows of a workgroup, and reference columns of one step
#define SG_PRD_LD 65            // row pitch of the LDS images [k][row]: consecutive k land on consecutive banks
#define SG_PRD_KP 50            // k rows per channel: 49 and one zero row, so that the MFMA's pairs of k stay inside a channel
#define SG_PRD_MAX_K 8          // neighbours a row keeps

typedef float sg_f32x16 __attribute__((ext_vector_type(16)));

// v: the 8 smallest values seen so far, ascending (a multiset: equal values each count)
__device__ __forceinline__ void sg_prd_insert(float (&v)[SG_PRD_MAX_K], float d) {
    if (!(d < v[SG_PRD_MAX_K - 1])) return;
#pragma unroll
    for (int s = SG_PRD_MAX_K - 1; s > 0; --s) v[s] = d < v[s - 1] ? v[s - 1] : (d < v[s] ? d : v[s]);
    v[0] = d < v[0] ? d : v[0];
}

// Row norms of the Gram form: out[i] = sum_k n_ik^2, an FMA chain over k ascending on the normalised values.
__global__ __launch_bounds__(256) void sg_prd_norms_kernel(const float* __restrict__ desc, const double* __restrict__ stats, double count, int N,
                                                           int C, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* row = desc + (int64_t)i * C * SG_SWD_TAPS;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        float m32, r32;
        sg_swd_norm(stats, C, c, count, m32, r32);
        for (int t = 0; t < SG_SWD_TAPS; ++t) {
            const float n = sg_swd_normalise(row[c * SG_SWD_TAPS + t], m32, r32);
            acc = fmaf(n, n, acc);
        }
    }
    out[i] = acc;
}

// The pass.  Workgroup b owns query rows [64 b, 64 b + 64): their normalised values stay in LDS ([channel][k][row]); the reference
// columns pass through 64 at a time, one channel (49 k) staged per step.
//   DIRECT (GRAM = false): thread (ti, tj) holds the pairs (rows ti + 16 a, columns 4 tj + b), a, b < 4: d2 += (q - r)^2, k ascending.
//   GRAM: wave w holds the 32 x 32 quadrant (rows 32 (w & 1), columns 32 (w >> 1)) of q . r in one v_mfma_f32_32x32x2_f32 accumulator
//     with the REFERENCE columns as the MFMA's rows: lane l then holds ONE query row (l & 31) and 16 columns ((reg & 3) + 8 (reg >> 2) +
//     4 (l >> 5)), so its row-wise state is one row's; d2 = max(nq + nr - 2 q . r, 0).
//   KNN epilogue (self pass, descQ == descR): a row keeps the 8 smallest d2 over the admitted columns -- those outside its own group of
//     `group` consecutive rows; rad = the k-th, nn1 = the first.
//   ROWS epilogue: cnt = #{j : d2 <= radR[j]}, and the smallest d2 with the smallest j that attains it.
// A row's partial results (16 threads in DIRECT, 4 lanes in GRAM) meet in LDS at the end; thread r < 64 merges row r and writes it.
template <bool GRAM, bool KNN>
__global__ __launch_bounds__(256) void sg_prd_kernel(const float* __restrict__ descQ, const float* __restrict__ descR,
                                                     const double* __restrict__ stats, double count, const float* __restrict__ radR,
                                                     const float* __restrict__ normQ, const float* __restrict__ normR, int Nq, int Nr, int C,
                                                     int k, int group, float* __restrict__ out_f0, float* __restrict__ out_f1,
                                                     int32_t* __restrict__ out_cnt, int32_t* __restrict__ out_idx) {
    constexpr int NR = GRAM ? 1 : 4;                  // query rows a thread holds
    constexpr int NP = GRAM ? 4 : 16;                 // partial results per row
    __shared__ float Qs[3 * SG_PRD_KP * SG_PRD_LD];   // 39,000 B; the merge buffer at the end (at most 32 KiB)
    __shared__ float Rs[SG_PRD_KP * SG_PRD_LD];       // 13,000 B
    __shared__ float NrS[SG_PRD_T], RadS[SG_PRD_T];
    __shared__ float MR[3][2];
    const int K = C * SG_SWD_TAPS, tid = threadIdx.x;
    const int i0 = blockIdx.x * SG_PRD_T;
    const int ti = tid & 15, tj = tid >> 4;                                             // DIRECT
    const int lane = tid & 63, wv = tid >> 6, h = lane >> 5, c31 = lane & 31;           // GRAM
    const int ib = 32 * (wv & 1), jb = 32 * (wv >> 1);

    if (tid < C) sg_swd_norm(stats, C, tid, count, MR[tid][0], MR[tid][1]);
    for (int e = tid; e < SG_PRD_LD; e += 256) {      // the zero rows, written once
        Rs[SG_SWD_TAPS * SG_PRD_LD + e] = 0.f;
        for (int c = 0; c < C; ++c) Qs[(c * SG_PRD_KP + SG_SWD_TAPS) * SG_PRD_LD + e] = 0.f;
    }
    SG_SYNC();
    for (int e = tid; e < SG_PRD_T * K; e += 256) {
        const int r = e / K, kk = e - r * K, c = kk / SG_SWD_TAPS, t = kk - c * SG_SWD_TAPS;
        const int i = i0 + r;
        Qs[(c * SG_PRD_KP + t) * SG_PRD_LD + r] = i < Nq ? sg_swd_normalise(descQ[(int64_t)i * K + kk], MR[c][0], MR[c][1]) : 0.f;
    }

    // row-wise state
    int rowi[NR];
    float top[NR][SG_PRD_MAX_K];
    int lo[NR], hi[NR], cnt[NR], bidx[NR];
    float best[NR], nq[NR];
#pragma unroll
    for (int a = 0; a < NR; ++a) {
        const int i = i0 + (GRAM ? ib + c31 : ti + 16 * a);
        rowi[a] = i;
        lo[a] = (i / group) * group;
        const int64_t e = (int64_t)lo[a] + group;
        hi[a] = e < Nr ? (int)e : Nr;
        cnt[a] = 0;
        bidx[a] = 0x7fffffff;
        best[a] = __builtin_inff();
        nq[a] = (GRAM && i < Nq) ? normQ[i] : 0.f;
#pragma unroll
        for (int s = 0; s < SG_PRD_MAX_K; ++s) top[a][s] = __builtin_inff();
    }

    auto visit = [&](int a, int j, int jl, float d2) {
        if (j >= Nr) return;
        if constexpr (KNN) {
            if (j >= lo[a] && j < hi[a]) return;      // the row's own group: itself and the patches of its image
            sg_prd_insert(top[a], d2);
        } else {
            cnt[a] += d2 <= RadS[jl] ? 1 : 0;
            if (d2 < best[a] || (d2 == best[a] && j < bidx[a])) {
                best[a] = d2;
                bidx[a] = j;
            }
        }
    };

    for (int jt = 0; jt < Nr; jt += SG_PRD_T) {
        float acc[4][4];
        sg_f32x16 dot;
        if constexpr (GRAM) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dot[r] = 0.f;
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
        }
        for (int c = 0; c < C; ++c) {
            SG_SYNC();      // the readers of Rs (and, at c == 0, of NrS / RadS and the writers of Qs) are through
            const float m32 = MR[c][0], r32 = MR[c][1];
            for (int e = tid; e < SG_PRD_T * SG_SWD_TAPS; e += 256) {
                const int r = e / SG_SWD_TAPS, t = e - r * SG_SWD_TAPS;
                const int j = jt + r;
                Rs[t * SG_PRD_LD + r] = j < Nr ? sg_swd_normalise(descR[(int64_t)j * K + c * SG_SWD_TAPS + t], m32, r32) : 0.f;
            }
            if (c == 0 && tid < SG_PRD_T) {
                const int j = jt + tid;
                if constexpr (GRAM) NrS[tid] = j < Nr ? normR[j] : 0.f;
                if constexpr (!KNN) RadS[tid] = j < Nr ? radR[j] : 0.f;
            }
            SG_SYNC();
            const float* Qc = Qs + c * SG_PRD_KP * SG_PRD_LD;
            if constexpr (GRAM) {
#pragma unroll 5
                for (int s = 0; s < SG_PRD_KP / 2; ++s) {
                    const float rv = Rs[(2 * s + h) * SG_PRD_LD + jb + c31];
                    const float qv = Qc[(2 * s + h) * SG_PRD_LD + ib + c31];
                    dot = __builtin_amdgcn_mfma_f32_32x32x2f32(rv, qv, dot, 0, 0, 0);
                }
            } else {
#pragma unroll 7
                for (int t = 0; t < SG_SWD_TAPS; ++t) {
                    float qv[4], rv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) qv[a] = Qc[t * SG_PRD_LD + ti + 16 * a];
#pragma unroll
                    for (int b = 0; b < 4; ++b) rv[b] = Rs[t * SG_PRD_LD + 4 * tj + b];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float d = __fsub_rn(qv[a], rv[b]);
                            acc[a][b] = fmaf(d, d, acc[a][b]);
                        }
                }
            }
        }
        if constexpr (GRAM) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = jb + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float d2 = fmaxf(fmaf(-2.f, dot[r], __fadd_rn(nq[0], NrS[jl])), 0.f);
                visit(0, jt + jl, jl, d2);
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) visit(a, jt + 4 * tj + b, 4 * tj + b, acc[a][b]);
        }
    }

    // merge: partial p of row r
    SG_SYNC();
    float* Mf = Qs;
    int32_t* Mi = (int32_t*)Qs;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
        const int r = GRAM ? ib + c31 : ti + 16 * a;
        const int p = GRAM ? 2 * (wv >> 1) + h : tj;
        if constexpr (KNN) {
#pragma unroll
            for (int s = 0; s < SG_PRD_MAX_K; ++s) Mf[(r * NP + p) * SG_PRD_MAX_K + s] = top[a][s];
        } else {
            Mi[(r * NP + p) * 3 + 0] = cnt[a];
            Mf[(r * NP + p) * 3 + 1] = best[a];
            Mi[(r * NP + p) * 3 + 2] = bidx[a];
        }
    }
    SG_SYNC();
    if (tid >= SG_PRD_T || i0 + tid >= Nq) return;
    const int i = i0 + tid;
    if constexpr (KNN) {
        float v[SG_PRD_MAX_K];
#pragma unroll
        for (int s = 0; s < SG_PRD_MAX_K; ++s) v[s] = Mf[(tid * NP) * SG_PRD_MAX_K + s];
        for (int p = 1; p < NP; ++p)
            for (int s = 0; s < SG_PRD_MAX_K; ++s) sg_prd_insert(v, Mf[(tid * NP + p) * SG_PRD_MAX_K + s]);
        float kth = v[0];
#pragma unroll
        for (int s = 1; s < SG_PRD_MAX_K; ++s) kth = s == k - 1 ? v[s] : kth;
        out_f0[i] = kth;
        out_f1[i] = v[0];
    } else {
        int n = 0, bj = 0x7fffffff;
        float bd = __builtin_inff();
        for (int p = 0; p < NP; ++p) {
            n += Mi[(tid * NP + p) * 3 + 0];
            const float d = Mf[(tid * NP + p) * 3 + 1];
            const int j = Mi[(tid * NP + p) * 3 + 2];
            if (d < bd || (d == bd && j < bj)) {
                bd = d;
                bj = j;
            }
        }
        out_cnt[i] = n;
        out_f0[i] = bd;
        out_idx[i] = bj;
    }
}

// out4: #{cntB > 0}, #{cntA > 0}, sum cntB, #{nn_d2_A <= radA}.  One workgroup; integer sums, so the order does not show.
__global__ __launch_bounds__(256) void sg_prd_finish_kernel(const int32_t* __restrict__ cntB, const int32_t* __restrict__ cntA,
                                                            const float* __restrict__ nnA, const float* __restrict__ radA, int N,
                                                            int64_t* __restrict__ out4) {
    __shared__ long long red[4][256];
    long long s[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += 256) {
        s[0] += cntB[i] > 0;
        s[1] += cntA[i] > 0;
        s[2] += cntB[i];
        s[3] += nnA[i] <= radA[i];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = s[q];
    SG_SYNC();
    if (threadIdx.x < 4) {
        long long t = 0;
        for (int e = 0; e < 256; ++e) t += red[threadIdx.x][e];
        out4[threadIdx.x] = t;
    }
}

static bool sg_prd_rows_covered(int32_t N) { return N >= 1 && N <= SG_SWD_MAX_N; }

extern "C" int64_t sgan_prd_workspace(int32_t Nq, int32_t Nr, int32_t K) {
    if (!sg_prd_rows_covered(Nq) || !sg_prd_rows_covered(Nr) || !sg_swd_channels(K))
        return sgan_fail(SGAN_ERR_UNSUPPORTED, "the k-nearest-neighbour passes cover 1 <= N <= %d rows per set and K in {49, 98, 147}; got %d and %d rows, K %d",
                         SG_SWD_MAX_N, Nq, Nr, K);
    return (((int64_t)Nq + Nr) * 4 + 15) / 16 * 16;
}

// what the two passes check alike; < 0 with the message set, else the resolved variant
static int sg_prd_common(int32_t Nq, int32_t Nr, int32_t K, const void* ws, int64_t ws_bytes, int32_t variant) {
    const int64_t need = sgan_prd_workspace(Nq, Nr, K);
    if (need < 0) return SGAN_ERR_UNSUPPORTED;      // the message is set
    if (variant < SGAN_PRD_AUTO || variant > SGAN_PRD_GRAM) return sgan_fail(SGAN_ERR_INVALID, "variant %d (0 = auto, 1 = direct, 2 = gram)", variant);
    if (ws_bytes < need)
        return sgan_fail(SGAN_ERR_INVALID, "workspace of %lld bytes, %lld needed for %d and %d rows, K %d (sgan_prd_workspace); nothing was launched",
                         (long long)ws_bytes, (long long)need, Nq, Nr, K);
    if (((uintptr_t)ws & 15) != 0) return sgan_fail(SGAN_ERR_INVALID, "workspace not 16-byte aligned");
    return variant == SGAN_PRD_AUTO ? SGAN_PRD_GRAM : variant;      // the faster form at N = 16384, K = 147
}

extern "C" int sgan_knn_radii(const float* desc, const double* stats, int32_t N, int32_t K, int32_t k, int32_t group, float* rad, float* nn1,
                              void* ws, int64_t ws_bytes, int32_t variant, void* stream) {
    SGAN_CHECK(desc && stats && rad && nn1 && ws, "null pointer");
    const int v = sg_prd_common(N, N, K, ws, ws_bytes, variant);
    if (v < 0) return v;
    SGAN_CHECK(k >= 1 && k <= SG_PRD_MAX_K && group >= 1, "k %d (1..%d) or group %d (>= 1)", k, SG_PRD_MAX_K, group);
    SGAN_CHECK((int64_t)k <= (int64_t)N - group, "k %d > N - group = %d - %d: a row would have fewer than k admitted neighbours", k, N, group);
    const int C = sg_swd_channels(K);
    const double count = (double)N * (double)SG_SWD_TAPS;
    float* norms = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((N + SG_PRD_T - 1) / SG_PRD_T);
    if (v == SGAN_PRD_GRAM) {
        hipLaunchKernelGGL(sg_prd_norms_kernel, dim3((N + 255) / 256), dim3(256), 0, st, desc, stats, count, N, C, norms);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL((sg_prd_kernel<true, true>), grid, dim3(256), 0, st, desc, desc, stats, count, (const float*)nullptr, norms, norms, N, N,
                           C, k, group, rad, nn1, (int32_t*)nullptr, (int32_t*)nullptr);
    } else {
        hipLaunchKernelGGL((sg_prd_kernel<false, true>), grid, dim3(256), 0, st, desc, desc, stats, count, (const float*)nullptr,
                           (const float*)nullptr, (const float*)nullptr, N, N, C, k, group, rad, nn1, (int32_t*)nullptr, (int32_t*)nullptr);
    }
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_prd_kernel";
    return SGAN_OK;
}

extern "C" int sgan_prd_rows(const float* descQ, const float* descR, const double* stats, const float* radR, int32_t Nq, int32_t Nr, int32_t K,
                             int32_t* cnt, float* nn_d2, int32_t* nn_idx, void* ws, int64_t ws_bytes, int32_t variant, void* stream) {
    SGAN_CHECK(descQ && descR && stats && radR && cnt && nn_d2 && nn_idx && ws, "null pointer");
    const int v = sg_prd_common(Nq, Nr, K, ws, ws_bytes, variant);
    if (v < 0) return v;
    const int C = sg_swd_channels(K);
    const double count = (double)Nr * (double)SG_SWD_TAPS;
    float* normQ = (float*)ws;
    float* normR = normQ + Nq;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((Nq + SG_PRD_T - 1) / SG_PRD_T);
    if (v == SGAN_PRD_GRAM) {
        hipLaunchKernelGGL(sg_prd_norms_kernel, dim3((Nq + 255) / 256), dim3(256), 0, st, descQ, stats, count, Nq, C, normQ);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_prd_norms_kernel, dim3((Nr + 255) / 256), dim3(256), 0, st, descR, stats, count, Nr, C, normR);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL((sg_prd_kernel<true, false>), grid, dim3(256), 0, st, descQ, descR, stats, count, radR, normQ, normR, Nq, Nr, C, 0, 1,
                           nn_d2, (float*)nullptr, cnt, nn_idx);
    } else {
        hipLaunchKernelGGL((sg_prd_kernel<false, false>), grid, dim3(256), 0, st, descQ, descR, stats, count, radR, (const float*)nullptr,
                           (const float*)nullptr, Nq, Nr, C, 0, 1, nn_d2, (float*)nullptr, cnt, nn_idx);
    }
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_prd_kernel";
    return SGAN_OK;
}

extern "C" int sgan_prd_finish(const int32_t* cntB, const int32_t* cntA, const float* nn_d2_A, const float* radA, int32_t N, int64_t* out4,
                               void* stream) {
    SGAN_CHECK(cntB && cntA && nn_d2_A && radA && out4, "null pointer");
    SGAN_CHECK(sg_prd_rows_covered(N), "N %d: the finish covers 1 <= N <= %d", N, SG_SWD_MAX_N);
    hipLaunchKernelGGL(sg_prd_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cntB, cntA, nn_d2_A, radA, N, out4);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_prd_finish_kernel";
    return SGAN_OK;
}
