// Tversky (soft Dice, focal-Tversky) and focal loss terms of the segmentation trainers (include/sgan_hip.h, "Segmentation loss terms";
// DESIGN.md §R31): both read the LOGITS where the generator left them and return the gradient of the logits, so the term needs no
// softmax launch of its own and no way back through a prediction.
//
// Two streaming launches, one thread per pixel, 256-thread workgroups, grid-stride, the grid a function of npix alone:
//   sg_seg_terms_fwd_kernel   softmax / sigmoid of the pixel in registers; per listed channel the fp64 sums TP, FP, FN, and the focal
//                             numerator and norm: 3 n + 2 sums.  Every workgroup leaves its partials in slots of its own and draws a
//                             ticket (sgan_reduce.h); the last to arrive adds the slots in a fixed order, zeroes them, and thread 0
//                             writes the state (per class TP, FP, FN, D, TI, L_c, G(0), G(1); the focal sums; both losses) in fp64.
//   sg_seg_terms_bwd_kernel   the same p again, the per-class pair G(0), G(1) and the focal norm from the state, the two upstream
//                             gradients from device floats; writes dlogits = tversky part + focal part, padding channels zero.
// No floating-point atomics, no workgroup waits on another, nothing read back or allocated.  With 4-, 8-, 12- or 16-channel storage on
// every operand (16-byte aligned) a pixel is one to four 16-byte accesses per operand; any other layout takes the scalar form.
#include "sgan_reduce.h"

#define SG_ST_MAXC 16
#define SG_ST_BLOCKS 512
#define SG_ST_SUMS (3 * SGAN_SEGTERMS_MAX_CLASSES + 2)      // [3 j + 0 .. 2] TP, FP, FN of listed class j; [24] focal numerator, [25] norm
static_assert((SG_ST_SUMS * SG_ST_BLOCKS + 1) * sizeof(double) <= SGAN_SEGTERMS_WS_BYTES, "workspace size");
static_assert((8 * SGAN_SEGTERMS_MAX_CLASSES + 4) * sizeof(double) == SGAN_SEGTERMS_STATE_BYTES, "state size");

#define SG_ST_REFUSE(cond, ...)                         \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

struct StArgs {
    const float* z; int ld;
    int npix, C, mode;
    const int64_t* label;              // SGAN_SEGHEAD_SOFTMAX
    const float* t; int tld;           // SGAN_SEGHEAD_SIGMOID
    int n;                             // listed classes; 0: the Tversky term is off
    int32_t cls[SGAN_SEGTERMS_MAX_CLASSES];
    double alpha, beta, smooth, power;
    int focal;                         // 0: the focal term is off
    float gamma;
    const float* cw; int nw;
    double* state;
    // forward
    float* loss_t; float* loss_f;
    double* part; unsigned* ticket;
    // backward
    const float* gout_t; const float* gout_f;
    float* d; int dld;
};

// CS > 0: the row is CS floats at a 16-byte aligned address; CS == 0: `n` floats `ld` apart from their neighbours' rows, the rest zero
template <int CS>
__device__ __forceinline__ void st_load_row(const float* base, int64_t pix, int ld, int n, float (&v)[CS ? CS : SG_ST_MAXC]) {
    if constexpr (CS > 0) {
        const f32x4* src = reinterpret_cast<const f32x4*>(base + pix * CS);
#pragma unroll
        for (int q = 0; q < CS / 4; ++q) {
            const f32x4 x = src[q];
            v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < SG_ST_MAXC; ++c) v[c] = c < n ? base[pix * ld + c] : 0.f;
    }
}

// v[c >= C] is zero already: the padding channels are written as zeros
template <int CS>
__device__ __forceinline__ void st_store_row(float* base, int64_t pix, int ld, const float (&v)[CS ? CS : SG_ST_MAXC]) {
    if constexpr (CS > 0) {
        f32x4* dst = reinterpret_cast<f32x4*>(base + pix * CS);
#pragma unroll
        for (int q = 0; q < CS / 4; ++q) {
            f32x4 x;
            x[0] = v[4 * q]; x[1] = v[4 * q + 1]; x[2] = v[4 * q + 2]; x[3] = v[4 * q + 3];
            dst[q] = x;
        }
    } else {
#pragma unroll
        for (int c = 0; c < SG_ST_MAXC; ++c)
            if (c < ld) base[pix * ld + c] = v[c];
        for (int c = SG_ST_MAXC; c < ld; ++c) base[pix * ld + c] = 0.f;
    }
}

// softmax over the first C of N channels: p, and what the focal term reads: lp = z_y - logsumexp(z) and om = 1 - p_y taken as the sum
// of the other channels' exponentials over the whole sum (no cancellation near p_y = 1).  y < 0: lp and om are not meaningful.
template <int N>
__device__ __forceinline__ void st_softmax(const float (&z)[N], int C, int y, float (&p)[N], float& lp, float& om) {
    float m = -3.4e38f;
#pragma unroll
    for (int c = 0; c < N; ++c) m = c < C ? fmaxf(m, z[c]) : m;
    float sum = 0.f, others = 0.f, zy = 0.f;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        p[c] = c < C ? expf(z[c] - m) : 0.f;
        sum += p[c];
        others += c == y ? 0.f : p[c];
        zy = c == y ? z[c] : zy;
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < N; ++c) p[c] *= inv;
    lp = zy - (m + logf(sum));
    om = others * inv;
}

__device__ __forceinline__ float st_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// bit c is set where channel c is listed
__device__ __forceinline__ unsigned st_listed_mask(const StArgs& A) {
    unsigned mask = 0u;
    for (int j = 0; j < A.n; ++j) mask |= 1u << A.cls[j];
    return mask;
}

template <int CS>
__global__ __launch_bounds__(256) void sg_seg_terms_fwd_kernel(const StArgs A) {
    constexpr int N = CS ? CS : SG_ST_MAXC;
    __shared__ double red[4];
    __shared__ int last;
    const int C = A.C;
    const bool softmax = A.mode == SGAN_SEGHEAD_SOFTMAX;
    const unsigned mask = st_listed_mask(A);
    const bool focal = A.focal != 0;
    const float gamma = A.gamma;
    float cw[N];
    const int ncw = A.cw ? A.nw : 0;
#pragma unroll
    for (int c = 0; c < N; ++c) cw[c] = c < ncw ? A.cw[c] : 1.f;
    double tp[N], fp[N], fn[N], fnum = 0.0, fnorm = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) tp[c] = fp[c] = fn[c] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.npix; i += (int64_t)gridDim.x * 256) {
        float z[N], p[N];
        st_load_row<CS>(A.z, i, A.ld, C, z);
        if (softmax) {
            const int64_t yl = A.label[i];
            if (yl < 0 || yl >= C) continue;      // torch's ignore_index (-100) and anything out of range: no contribution to any sum
            const int y = (int)yl;
            float lp, om;
            st_softmax<N>(z, C, y, p, lp, om);
#pragma unroll
            for (int c = 0; c < N; ++c) {
                if (mask >> c & 1u) {
                    const double pd = (double)p[c];
                    if (c == y) { tp[c] += pd; fn[c] += 1.0 - pd; }
                    else fp[c] += pd;
                }
            }
            if (focal) {
                float w = 0.f;
#pragma unroll
                for (int c = 0; c < N; ++c) w = c == y ? cw[c] : w;
                fnum += (double)(w * (powf(om, gamma) * -lp));
                fnorm += (double)w;
            }
        } else {
            float t[N];
            st_load_row<CS>(A.t, i, A.tld, C, t);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < N; ++c) {
                if (c < C) {
                    const float pv = sg_sigmoid(z[c]), tv = t[c];
                    if (mask >> c & 1u) {
                        const double pd = (double)pv, td = (double)tv;
                        tp[c] += pd * td;
                        fp[c] += pd * (1.0 - td);
                        fn[c] += (1.0 - pd) * td;
                    }
                    if (focal) {
                        const float qv = sg_sigmoid(-z[c]);      // 1 - p without the cancellation
                        s += cw[c] * (tv * powf(qv, gamma) * st_softplus(-z[c]) + (1.f - tv) * powf(pv, gamma) * st_softplus(z[c]));
                    }
                }
            }
            fnum += (double)s;
        }
    }
    // the 3 n + 2 workgroup sums into this workgroup's slots, then the ticket
    const int n = A.n;
    double* part = A.part;
    double lastsum = 0.0;
#pragma unroll
    for (int k = 0; k < SG_ST_SUMS; ++k) {
        const bool active = k < 24 ? k / 3 < n : focal;
        if (!active) continue;      // uniform over the grid
        double v;
        if (k < 24) {
            const int ch = A.cls[k / 3];
            v = 0.0;
#pragma unroll
            for (int c = 0; c < N; ++c) v = c == ch ? (k % 3 == 0 ? tp[c] : k % 3 == 1 ? fp[c] : fn[c]) : v;
        } else {
            v = k == 24 ? fnum : fnorm;
        }
        lastsum = sg_block_sum<4>(v, red);
        SG_SYNC();      // frees `red` for the next sum
        if (threadIdx.x == 0) part[k * SG_ST_BLOCKS + blockIdx.x] = lastsum;
    }
    // thread 0 wrote every slot above; sg_publish_last stores the last active one once more, fences behind all of them and takes the ticket
    const int klast = focal ? SG_ST_SUMS - 1 : 3 * n - 1;
    if (!sg_publish_last(lastsum, &part[klast * SG_ST_BLOCKS + blockIdx.x], A.ticket, gridDim.x - 1, &last)) return;
    __threadfence();
    double S[SG_ST_SUMS];
#pragma unroll
    for (int k = 0; k < SG_ST_SUMS; ++k) {
        S[k] = 0.0;
        const bool active = k < 24 ? k / 3 < n : focal;
        if (!active) continue;
        double v = 0.0;
        for (unsigned b = threadIdx.x; b < gridDim.x; b += 256) {
            v += sg_slot_load(&part[k * SG_ST_BLOCKS + b]);
            part[k * SG_ST_BLOCKS + b] = 0.0;
        }
        S[k] = sg_block_sum<4>(v, red);
        SG_SYNC();
    }
    if (threadIdx.x != 0) return;
    double* st = A.state;
    double LT = 0.0;
#pragma unroll
    for (int j = 0; j < SGAN_SEGTERMS_MAX_CLASSES; ++j) {
        double TP = 0.0, FP = 0.0, FN = 0.0, D = 0.0, TI = 0.0, Lc = 0.0, G0 = 0.0, G1 = 0.0;
        if (j < n) {
            TP = S[3 * j]; FP = S[3 * j + 1]; FN = S[3 * j + 2];
            D = ((TP + A.alpha * FP) + A.beta * FN) + A.smooth;      // >= TP + smooth in this order of the roundings, so TI <= 1
            if (D > 0.0) {
                const double num = TP + A.smooth;
                TI = num / D;
                const double u = fmax(1.0 - TI, 0.0);
                if (u > 0.0) {
                    Lc = pow(u, A.power);
                    const double k = -(A.power / (double)n) * pow(u, A.power - 1.0);
                    G0 = k * (-(num * A.alpha) / (D * D));
                    G1 = k * (1.0 / D - (num * (1.0 - A.beta)) / (D * D));
                }
            }
            LT += Lc;
        }
        st[8 * j] = TP; st[8 * j + 1] = FP; st[8 * j + 2] = FN; st[8 * j + 3] = D;
        st[8 * j + 4] = TI; st[8 * j + 5] = Lc; st[8 * j + 6] = G0; st[8 * j + 7] = G1;
    }
    LT = n ? LT / (double)n : 0.0;
    double fnrm = 0.0, LF = 0.0;
    if (focal) {
        fnrm = softmax ? S[25] : (double)C * (double)A.npix;
        LF = fnrm > 0.0 ? S[24] / fnrm : 0.0;
    }
    st[64] = S[24]; st[65] = fnrm; st[66] = LT; st[67] = LF;
    A.loss_t[0] = (float)LT;
    A.loss_f[0] = (float)LF;
    A.ticket[0] = 0u;
}

template <int CS>
__global__ __launch_bounds__(256) void sg_seg_terms_bwd_kernel(const StArgs A) {
    constexpr int N = CS ? CS : SG_ST_MAXC;
    const int C = A.C;
    const bool softmax = A.mode == SGAN_SEGHEAD_SOFTMAX;
    const bool tversky = A.n > 0 && A.gout_t != nullptr;
    const bool focal = A.focal != 0 && A.gout_f != nullptr;
    const float gamma = A.gamma;
    // per channel the pair G(0), G(1) times the upstream gradient; zeros on an unlisted channel
    float g0[N], g1[N], cw[N];
#pragma unroll
    for (int c = 0; c < N; ++c) g0[c] = g1[c] = 0.f;
    if (tversky) {
        const double up = (double)A.gout_t[0];
        for (int j = 0; j < A.n; ++j) {
            const int ch = A.cls[j];
            const float a = (float)(up * A.state[8 * j + 6]), b = (float)(up * A.state[8 * j + 7]);
#pragma unroll
            for (int c = 0; c < N; ++c) {
                g0[c] = c == ch ? a : g0[c];
                g1[c] = c == ch ? b : g1[c];
            }
        }
    }
    const int ncw = A.cw ? A.nw : 0;
#pragma unroll
    for (int c = 0; c < N; ++c) cw[c] = c < ncw ? A.cw[c] : 1.f;
    float fscale = 0.f;      // upstream gradient over the norm
    if (focal) {
        const double nrm = A.state[65];
        fscale = nrm > 0.0 ? (float)((double)A.gout_f[0] / nrm) : 0.f;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.npix; i += (int64_t)gridDim.x * 256) {
        float z[N], p[N], d[N];
#pragma unroll
        for (int c = 0; c < N; ++c) d[c] = 0.f;
        bool ok = true;
        int y = -1;
        if (softmax) {
            const int64_t yl = A.label[i];
            ok = yl >= 0 && yl < C;
            y = ok ? (int)yl : -1;
        }
        if (ok && (tversky || focal)) {
            st_load_row<CS>(A.z, i, A.ld, C, z);
            if (softmax) {
                float lp, om;
                st_softmax<N>(z, C, y, p, lp, om);
                if (tversky) {
                    float s = 0.f, g[N];
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        g[c] = c == y ? g1[c] : g0[c];
                        s += p[c] * g[c];
                    }
#pragma unroll
                    for (int c = 0; c < N; ++c) d[c] = c < C ? p[c] * (g[c] - s) : 0.f;
                }
                if (focal) {
                    float w = 0.f, pt = 0.f;
#pragma unroll
                    for (int c = 0; c < N; ++c) { w = c == y ? cw[c] : w; pt = c == y ? p[c] : pt; }
                    float k = -powf(om, gamma);
                    if (gamma != 0.f && om != 0.f) k += gamma * pt * powf(om, gamma - 1.f) * lp;
                    const float ws = w * fscale * k;
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        const float f = c < C ? ws * ((c == y ? 1.f : 0.f) - p[c]) : 0.f;
                        d[c] += f;
                    }
                }
            } else {
                float t[N];
                st_load_row<CS>(A.t, i, A.tld, C, t);
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    if (c < C) {
                        const float pv = sg_sigmoid(z[c]), qv = sg_sigmoid(-z[c]), tv = t[c];
                        float dv = 0.f;
                        if (tversky) dv = pv * qv * (g0[c] + tv * (g1[c] - g0[c]));
                        if (focal) {
                            const float neg = tv * powf(qv, gamma) * (gamma * pv * st_softplus(-z[c]) + qv);
                            const float pos = (1.f - tv) * powf(pv, gamma) * (gamma * qv * st_softplus(z[c]) + pv);
                            const float f = cw[c] * fscale * (pos - neg);
                            dv += f;
                        }
                        d[c] = dv;
                    }
                }
            }
        }
        st_store_row<CS>(A.d, i, A.dld, d);
    }
}

static inline bool st_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool FWD>
static void st_launch(int cs, int blocks, hipStream_t st, const StArgs& A) {
    const dim3 g(blocks), b(256);
    if constexpr (FWD) {
        if (cs == 4) hipLaunchKernelGGL((sg_seg_terms_fwd_kernel<4>), g, b, 0, st, A);
        else if (cs == 8) hipLaunchKernelGGL((sg_seg_terms_fwd_kernel<8>), g, b, 0, st, A);
        else if (cs == 12) hipLaunchKernelGGL((sg_seg_terms_fwd_kernel<12>), g, b, 0, st, A);
        else if (cs == 16) hipLaunchKernelGGL((sg_seg_terms_fwd_kernel<16>), g, b, 0, st, A);
        else hipLaunchKernelGGL((sg_seg_terms_fwd_kernel<0>), g, b, 0, st, A);
    } else {
        if (cs == 4) hipLaunchKernelGGL((sg_seg_terms_bwd_kernel<4>), g, b, 0, st, A);
        else if (cs == 8) hipLaunchKernelGGL((sg_seg_terms_bwd_kernel<8>), g, b, 0, st, A);
        else if (cs == 12) hipLaunchKernelGGL((sg_seg_terms_bwd_kernel<12>), g, b, 0, st, A);
        else if (cs == 16) hipLaunchKernelGGL((sg_seg_terms_bwd_kernel<16>), g, b, 0, st, A);
        else hipLaunchKernelGGL((sg_seg_terms_bwd_kernel<0>), g, b, 0, st, A);
    }
}

// what both entries check and fill; 1 with the reason set: not covered, nothing to launch
static int st_common(StArgs& A, const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                     int32_t tld, const int32_t* classes, int32_t n, double alpha, double beta, double smooth, double power, int32_t focal,
                     double gamma, const float* class_w, int32_t nw, const double* state) {
    SG_ST_REFUSE(C >= 1 && C <= SG_ST_MAXC, "not covered: %d channels (1 .. %d)", C, SG_ST_MAXC);
    SG_ST_REFUSE(n >= 0 && n <= SGAN_SEGTERMS_MAX_CLASSES, "not covered: %d listed classes (0 .. %d)", n, SGAN_SEGTERMS_MAX_CLASSES);
    SG_ST_REFUSE(n > 0 || focal, "not covered: both terms are off (no listed class and no focal term)");
    SG_ST_REFUSE(logits && label_or_target && state && (n == 0 || classes), "null pointer");
    SG_ST_REFUSE(mode == SGAN_SEGHEAD_SOFTMAX || mode == SGAN_SEGHEAD_SIGMOID, "mode is SGAN_SEGHEAD_SOFTMAX or SGAN_SEGHEAD_SIGMOID");
    SG_ST_REFUSE(npix > 0 && ld >= C && (mode == SGAN_SEGHEAD_SOFTMAX || tld >= C), "bad argument: %d pixels, rows of %d and %d for %d channels", npix,
                 ld, tld, C);
    for (int a = 0; a < n; ++a) {
        SG_ST_REFUSE(classes[a] >= 0 && classes[a] < C, "listed class %d is not below C = %d", classes[a], C);
        for (int b = 0; b < a; ++b) SG_ST_REFUSE(classes[a] != classes[b], "listed class %d repeats", classes[a]);
    }
    if (n > 0)
        SG_ST_REFUSE(alpha >= 0.0 && beta >= 0.0 && alpha + beta > 0.0 && smooth >= 0.0 && power > 0.0 && power <= 4.0,
                     "Tversky parameters: alpha, beta >= 0 with alpha + beta > 0, smooth >= 0, 0 < power <= 4 (got %g, %g, %g, %g)", alpha, beta,
                     smooth, power);
    if (focal) {
        SG_ST_REFUSE(gamma >= 0.0 && gamma <= 8.0, "focal gamma in [0, 8] (got %g)", gamma);
        SG_ST_REFUSE(nw >= 0 && (!class_w || (mode == SGAN_SEGHEAD_SOFTMAX ? nw >= C : nw <= C)), "class weights: C of them (softmax), 0..C (sigmoid)");
    }
    SG_ST_REFUSE(((uintptr_t)state & 7) == 0, "state not 8-byte aligned");
    const bool softmax = mode == SGAN_SEGHEAD_SOFTMAX;
    A.z = logits; A.ld = ld; A.npix = npix; A.C = C; A.mode = mode;
    A.label = softmax ? static_cast<const int64_t*>(label_or_target) : nullptr;
    A.t = softmax ? nullptr : static_cast<const float*>(label_or_target);
    A.tld = tld; A.n = n;
    for (int a = 0; a < SGAN_SEGTERMS_MAX_CLASSES; ++a) A.cls[a] = a < n ? classes[a] : 0;
    A.alpha = alpha; A.beta = beta; A.smooth = smooth; A.power = power;
    A.focal = focal ? 1 : 0; A.gamma = (float)gamma;
    A.cw = focal ? class_w : nullptr; A.nw = (focal && class_w) ? (nw < C ? nw : C) : 0;
    A.state = const_cast<double*>(state);
    A.loss_t = A.loss_f = nullptr; A.part = nullptr; A.ticket = nullptr;
    A.gout_t = A.gout_f = nullptr; A.d = nullptr; A.dld = 0;
    return SGAN_OK;
}

static int st_blocks(int32_t npix) {
    const int blocks = sg_cdiv(npix, 256);
    return blocks > SG_ST_BLOCKS ? SG_ST_BLOCKS : blocks;
}

extern "C" int sgan_seg_terms_forward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                                      int32_t tld, const int32_t* classes, int32_t n, double alpha, double beta, double smooth, double power,
                                      int32_t focal, double gamma, const float* class_w, int32_t nw, double* state, float* loss_tversky,
                                      float* loss_focal, void* workspace, void* stream) {
    StArgs A;
    if (int rc = st_common(A, logits, ld, npix, C, mode, label_or_target, tld, classes, n, alpha, beta, smooth, power, focal, gamma, class_w, nw,
                           state))
        return rc;
    SG_ST_REFUSE(loss_tversky && loss_focal && workspace, "null pointer");
    SG_ST_REFUSE(((uintptr_t)workspace & 7) == 0, "workspace of SGAN_SEGTERMS_WS_BYTES (8-byte aligned) required");
    A.loss_t = loss_tversky; A.loss_f = loss_focal;
    A.part = static_cast<double*>(workspace);
    A.ticket = reinterpret_cast<unsigned*>(A.part + SG_ST_SUMS * SG_ST_BLOCKS);
    const bool softmax = mode == SGAN_SEGHEAD_SOFTMAX;
    const bool vec = (ld == 4 || ld == 8 || ld == 12 || ld == 16) && (softmax || tld == ld) && st_al16(logits) && (softmax || st_al16(label_or_target));
    st_launch<true>(vec ? ld : 0, st_blocks(npix), (hipStream_t)stream, A);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_seg_terms_fwd_kernel";
    return SGAN_OK;
}

extern "C" int sgan_seg_terms_backward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                                       int32_t tld, const int32_t* classes, int32_t n, int32_t focal, double gamma, const float* class_w,
                                       int32_t nw, const double* state, const float* gout_tversky, const float* gout_focal, float* dlogits,
                                       int32_t dld, void* stream) {
    StArgs A;
    // the Tversky parameters live in the state's pairs: the backward reads none of them
    if (int rc = st_common(A, logits, ld, npix, C, mode, label_or_target, tld, classes, n, 0.5, 0.5, 1.0, 1.0, focal, gamma, class_w, nw, state))
        return rc;
    SG_ST_REFUSE(dlogits, "null pointer");
    SG_ST_REFUSE(dld >= C, "gradient rows of %d for %d channels", dld, C);
    A.gout_t = gout_tversky; A.gout_f = gout_focal; A.d = dlogits; A.dld = dld;
    const bool softmax = mode == SGAN_SEGHEAD_SOFTMAX;
    const bool vec = (ld == 4 || ld == 8 || ld == 12 || ld == 16) && dld == ld && (softmax || tld == ld) && st_al16(logits) && st_al16(dlogits) &&
                     (softmax || st_al16(label_or_target));
    st_launch<false>(vec ? ld : 0, st_blocks(npix), (hipStream_t)stream, A);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_seg_terms_bwd_kernel";
    return SGAN_OK;
}
