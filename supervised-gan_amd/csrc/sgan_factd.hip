// Losses of the two trainers that multiply or weight probability maps:
//   * the factored-discriminator GAN loss of `--model twostage_factd` (models/twostage_factD_model.py:256-296,352-383 with util.mul,
//     util/util.py:131-145): sigmoid, bilinear x2, reflection pad, product, BCE / MSE and every scalar around them, up to 8 terms in
//     one launch -- the counterpart of sg_gan_loss_multi_fwd_kernel (sgan_ew.hip) on products of two maps;
//   * the channel sigmoid and the weighted BCE of `--use_sigmoid_ss` (models/segm_model.py:155-160,216-236).
// LDS holds nothing but the per-wave partial sums of the block reductions.
#include "sgan_reduce.h"

// ------------------------------------------------------------------------------------------
// Factored GAN loss.  Term j:  a1 = sig1 ? sigmoid(l1) : l1   [h1, w1]        a2 = sig2 ? sigmoid(l2) : l2   [H2, W2]
//   u = up == 2 ? bilinear_x2(a1) : a1   [hu, wu]      (the taps of sg_bilinear_up2_fwd_kernel: align_corners = False)
//   q[y, x] = u[refl(y - pt), refl(x - pl)]            pl = floor(dW / 2), pr = dW - pl, pb = floor(dH / 2), pt = dH - pb
//   p = q * a2,  loss_j = mean crit(p, target_j),  total = sum_j weight_j loss_j
// The gradients are gathers: a pixel of l2 needs its own p; a pixel of l1 walks the <= 4 x 4 positions of u it feeds and, for
// each, the interior position of q plus the <= 2 mirrored ones per axis (every pad is smaller than the map, so a position is
// mirrored at most once per side).  No float atomics: the same inputs give the same bits.
// ------------------------------------------------------------------------------------------
struct SgFactd {
    const float* l1[8];
    const float* l2[8];
    float* dl1[8];
    float* dl2[8];
    int32_t ld1[8], ld2[8], dld1[8], dld2[8];
    int32_t h1[8], w1[8], H2[8], W2[8], up[8];
    float target[8], weight[8];
    int32_t n, mode;
};

struct FdTerm {      // one term's fields in registers
    const float* l1;
    const float* l2;
    int ld1, ld2, h1, w1, hu, wu, H2, W2, up, pt, pl;
    float tg;
    bool sig1, sig2, mse;
};

__device__ __forceinline__ FdTerm fd_term(const SgFactd& J, int j) {
    FdTerm T;
    T.l1 = J.l1[j]; T.l2 = J.l2[j]; T.ld1 = J.ld1[j]; T.ld2 = J.ld2[j];
    T.h1 = J.h1[j]; T.w1 = J.w1[j]; T.H2 = J.H2[j]; T.W2 = J.W2[j]; T.up = J.up[j];
    T.hu = T.h1 * T.up; T.wu = T.w1 * T.up;
    const int dH = T.H2 - T.hu, dW = T.W2 - T.wu;
    T.pt = dH - dH / 2;      // the top takes the remainder (util.py:140-144)
    T.pl = dW / 2;
    T.tg = J.target[j];
    T.sig1 = (J.mode & SGAN_FACTD_SIG1) != 0; T.sig2 = (J.mode & SGAN_FACTD_SIG2) != 0; T.mse = (J.mode & SGAN_FACTD_MSE) != 0;
    return T;
}

__device__ __forceinline__ float fd_a1(const FdTerm& T, int iy, int ix) {
    const float v = T.l1[((int64_t)iy * T.w1 + ix) * T.ld1];
    return T.sig1 ? sg_sigmoid(v) : v;
}

__device__ __forceinline__ float fd_a2(const FdTerm& T, int y, int x) {
    const float v = T.l2[((int64_t)y * T.W2 + x) * T.ld2];
    return T.sig2 ? sg_sigmoid(v) : v;
}

// u[uy, ux]: out[2i + a] = 0.75 in[i] + 0.25 in[clamp(i - 1 + 2a)], separable, in the order sg_bilinear_up2_fwd_kernel adds them
__device__ __forceinline__ float fd_u(const FdTerm& T, int uy, int ux) {
    if (T.up == 1) return fd_a1(T, uy, ux);
    const int iy = uy >> 1, ix = ux >> 1;
    const int ny = min(max(iy - 1 + 2 * (uy & 1), 0), T.h1 - 1), nx = min(max(ix - 1 + 2 * (ux & 1), 0), T.w1 - 1);
    const float a = fd_a1(T, iy, ix), b = fd_a1(T, iy, nx), d = fd_a1(T, ny, ix), f = fd_a1(T, ny, nx);
    return 0.75f * (0.75f * a + 0.25f * b) + 0.25f * (0.75f * d + 0.25f * f);
}

__device__ __forceinline__ int fd_reflect(int r, int n) { return r < 0 ? -r : (r >= n ? 2 * (n - 1) - r : r); }

__device__ __forceinline__ float fd_loss(const FdTerm& T, float p) {
    if (T.mse) return (p - T.tg) * (p - T.tg);
    return sg_bce_term(p, T.tg);
}

// d crit / d p times `go` (= upstream * weight / pixels), the expressions of sg_gan_loss_multi_fwd_kernel
__device__ __forceinline__ float fd_dcrit(const FdTerm& T, float p, float go) {
    if (T.mse) return 2.f * (p - T.tg) * go;
    return sg_bce_dterm(p, T.tg) * go;
}

// d total / d l2 of pixel (y, x), given q and a2 there
__device__ __forceinline__ float fd_grad_l2(const FdTerm& T, float q, float a2, float go) {
    const float g = fd_dcrit(T, q * a2, go) * q;
    return T.sig2 ? g * ((1.f - a2) * a2) : g;
}

// sum over the positions of q that show u[uy, ux] of d total / d q there
__device__ __forceinline__ float fd_gather_q(const FdTerm& T, int uy, int ux, float go) {
    const float uv = fd_u(T, uy, ux);
    // rows of q (relative to the interior's origin) that read row uy of u: itself, its mirror above, its mirror below
    int ry[3], rx[3], ny = 0, nx = 0;
    ry[ny++] = uy;
    if (uy >= 1 && uy <= T.pt) ry[ny++] = -uy;
    if (2 * (T.hu - 1) - uy >= T.hu && 2 * (T.hu - 1) - uy + T.pt < T.H2) ry[ny++] = 2 * (T.hu - 1) - uy;
    rx[nx++] = ux;
    if (ux >= 1 && ux <= T.pl) rx[nx++] = -ux;
    if (2 * (T.wu - 1) - ux >= T.wu && 2 * (T.wu - 1) - ux + T.pl < T.W2) rx[nx++] = 2 * (T.wu - 1) - ux;
    float s = 0.f;
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b) {
            const float a2 = fd_a2(T, ry[a] + T.pt, rx[b] + T.pl);
            s += fd_dcrit(T, uv * a2, go) * a2;
        }
    return s;
}

// d total / d l1 of pixel (iy, ix)
__device__ __forceinline__ float fd_grad_l1(const FdTerm& T, int iy, int ix, float go) {
    float s;
    if (T.up == 1) {
        s = fd_gather_q(T, iy, ix, go);
    } else {      // the adjoint of the x2 taps, as sg_bilinear_up2_bwd_kernel walks them
        s = 0.f;
        for (int a = 0; a < 4; ++a) {
            const int uy = min(max(2 * iy - 1 + a, 0), T.hu - 1);
            const float wy = (a == 0 || a == 3) ? 0.25f : 0.75f;
            float row = 0.f;
            for (int b = 0; b < 4; ++b) {
                const int ux = min(max(2 * ix - 1 + b, 0), T.wu - 1);
                const float wx = (b == 0 || b == 3) ? 0.25f : 0.75f;
                row += wx * fd_gather_q(T, uy, ux, go);
            }
            s += wy * row;
        }
    }
    if (T.sig1) {
        const float a1 = fd_a1(T, iy, ix);
        s *= (1.f - a1) * a1;
    }
    return s;
}

__device__ __forceinline__ void fd_store(float* base, int64_t i, int ld, float v) {
    float* o = base + i * ld;
    o[0] = v;
    for (int c = 1; c < ld; ++c) o[c] = 0.f;
}

// workgroup b of nb writes its slice of d total / d l1 of term j
__device__ __forceinline__ void fd_write_l1_grad(const SgFactd& J, const FdTerm& T, int j, int b, int nb, float go) {
    float* dl1 = J.dl1[j];
    if (!dl1) return;
    const int dld1 = J.dld1[j], n1 = T.h1 * T.w1;
    for (int i = b * 256 + threadIdx.x; i < n1; i += nb * 256) fd_store(dl1, i, dld1, fd_grad_l1(T, i / T.w1, i % T.w1, go));
}

// Grid (SG_FACTD_BLOCKS, n): workgroup (b, j) leaves the fp64 partial sum of its slice of term j in `part`, writes its slice of the
// gradients for an upstream gradient of 1 where the job carries buffers, and takes a ticket; the last one turns the partials into
// each[] and the weighted total and leaves the counter at zero (sg_gan_loss_multi_fwd_kernel's finish: no fill per call).
#define SG_FACTD_BLOCKS 16
__global__ __launch_bounds__(256) void sg_factd_loss_multi_fwd_kernel(SgFactd J, double* part, unsigned* counter, float* each, float* total) {
    __shared__ double wsum[4];
    __shared__ int last;
    const int j = blockIdx.y, b = blockIdx.x;
    const FdTerm T = fd_term(J, j);
    const int np = T.H2 * T.W2;
    const float go = J.weight[j] / (float)np;
    float* dl2 = J.dl2[j];
    const int dld2 = J.dld2[j];
    double acc = 0.0;
    for (int i = b * 256 + threadIdx.x; i < np; i += SG_FACTD_BLOCKS * 256) {
        const int y = i / T.W2, x = i % T.W2;
        const float q = fd_u(T, fd_reflect(y - T.pt, T.hu), fd_reflect(x - T.pl, T.wu));
        const float a2 = fd_a2(T, y, x);
        acc += (double)fd_loss(T, q * a2);
        if (dl2) fd_store(dl2, i, dld2, fd_grad_l2(T, q, a2, go));
    }
    fd_write_l1_grad(J, T, j, b, SG_FACTD_BLOCKS, go);
    const double sum = sg_block_sum<4>(acc, wsum);
    if (!sg_publish_last(sum, &part[j * SG_FACTD_BLOCKS + b], counter, (unsigned)(SG_FACTD_BLOCKS * J.n - 1), &last) || threadIdx.x >= 64) return;
    __threadfence();                                         // every other workgroup's partial is visible from here on
    const int t = threadIdx.x;
    const bool has = t < J.n;
    sg_finish_terms<SG_FACTD_BLOCKS>(part, has, has ? (double)(J.H2[t] * J.W2[t]) : 1.0, has ? J.weight[t] : 0.f, each, total, counter);
}

// the gradients again, for an upstream gradient other than 1
__global__ __launch_bounds__(256) void sg_factd_loss_multi_bwd_kernel(SgFactd J, const float* gout) {
    const int j = blockIdx.y, b = blockIdx.x;
    const FdTerm T = fd_term(J, j);
    const int np = T.H2 * T.W2;
    const float go = gout[0] * J.weight[j] / (float)np;
    float* dl2 = J.dl2[j];
    if (dl2) {
        const int dld2 = J.dld2[j];
        for (int i = b * 256 + threadIdx.x; i < np; i += SG_FACTD_BLOCKS * 256) {
            const int y = i / T.W2, x = i % T.W2;
            const float q = fd_u(T, fd_reflect(y - T.pt, T.hu), fd_reflect(x - T.pl, T.wu));
            fd_store(dl2, i, dld2, fd_grad_l2(T, q, fd_a2(T, y, x), go));
        }
    }
    fd_write_l1_grad(J, T, j, b, SG_FACTD_BLOCKS, go);
}

// 0: launch; 1: outside the envelope ("not covered": nothing is written); < 0: a malformed call
static int fd_fill(SgFactd& J, const sgan_factd_loss_job* jobs, int n, int mode) {
    if (!jobs || n < 1) return sgan_fail(SGAN_ERR_INVALID, "no factored-loss jobs");
    if (mode < 0 || mode > 7) return sgan_fail(SGAN_ERR_INVALID, "mode is a sum of SGAN_FACTD_SIG1 / _SIG2 / _MSE");
    if (n > 8) return 1;
    // BCE wants a product of two probabilities: a raw score times a probability can leave [0, 1]
    if (!(mode & SGAN_FACTD_MSE) && (mode & (SGAN_FACTD_SIG1 | SGAN_FACTD_SIG2)) != (SGAN_FACTD_SIG1 | SGAN_FACTD_SIG2)) return 1;
    memset(&J, 0, sizeof(J));
    J.n = n;
    J.mode = mode;
    for (int i = 0; i < n; ++i) {
        const sgan_factd_loss_job& s = jobs[i];
        if (!s.l1 || !s.l2 || s.h1 < 1 || s.w1 < 1 || s.H2 < 1 || s.W2 < 1 || s.ld1 < 1 || s.ld2 < 1 || (s.dl1 && s.dld1 < 1) ||
            (s.dl2 && s.dld2 < 1) || (int64_t)s.H2 * s.W2 > (1 << 24))      // pixel indices are ints
            return sgan_fail(SGAN_ERR_INVALID, "bad factored-loss job %d", i);
        if (s.up != 1 && s.up != 2) return 1;
        const int hu = s.h1 * s.up, wu = s.w1 * s.up;
        if (hu > s.H2 || wu > s.W2) return 1;                       // util.mul returns None here
        const int dH = s.H2 - hu, dW = s.W2 - wu;
        if (dH - dH / 2 >= hu || dW - dW / 2 >= wu) return 1;       // torch's reflect rule: every pad smaller than the dimension
        J.l1[i] = s.l1; J.l2[i] = s.l2; J.dl1[i] = s.dl1; J.dl2[i] = s.dl2;
        J.ld1[i] = s.ld1; J.ld2[i] = s.ld2; J.dld1[i] = s.dld1; J.dld2[i] = s.dld2;
        J.h1[i] = s.h1; J.w1[i] = s.w1; J.H2[i] = s.H2; J.W2[i] = s.W2; J.up[i] = s.up;
        J.target[i] = s.target; J.weight[i] = s.weight;
    }
    return SGAN_OK;
}

extern "C" int sgan_factd_loss_multi_fwd(const sgan_factd_loss_job* jobs, int32_t n, int32_t mode, float* each_out, float* total_out,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    SgFactd J;
    int rc = fd_fill(J, jobs, n, mode);
    if (rc) return rc;
    SGAN_CHECK(each_out && total_out, "null output");
    SGAN_CHECK(workspace && workspace_bytes >= SGAN_FACTD_LOSS_WS_BYTES && ((uintptr_t)workspace & 7) == 0,
               "workspace of SGAN_FACTD_LOSS_WS_BYTES (8-byte aligned) required");
    static_assert((8 * SG_FACTD_BLOCKS + 1) * sizeof(double) <= SGAN_FACTD_LOSS_WS_BYTES, "workspace size");
    double* part = static_cast<double*>(workspace);
    unsigned* counter = reinterpret_cast<unsigned*>(part + 8 * SG_FACTD_BLOCKS);
    hipLaunchKernelGGL(sg_factd_loss_multi_fwd_kernel, dim3(SG_FACTD_BLOCKS, n), dim3(256), 0, (hipStream_t)stream, J, part, counter,
                       each_out, total_out);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_factd_loss_multi_bwd(const sgan_factd_loss_job* jobs, int32_t n, int32_t mode, const float* gout, void* stream) {
    SgFactd J;
    int rc = fd_fill(J, jobs, n, mode);
    if (rc) return rc;
    SGAN_CHECK(gout, "null gout");
    hipLaunchKernelGGL(sg_factd_loss_multi_bwd_kernel, dim3(SG_FACTD_BLOCKS, n), dim3(256), 0, (hipStream_t)stream, J, gout);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------
// `--use_sigmoid_ss`: sigmoid over the C logical channels of an NHWC map (padding channels of the result: zeros), and
//   loss = mean_{c, pix} w(pix) * bce(p_c, t_c),   w = 1 + sum_{i < nw} t_i * (cw_i - 1)
// with the weight evaluated from the class-weight vector where it is used.
// ------------------------------------------------------------------------------------------
#define SG_BCEW_MAXC 16
__global__ __launch_bounds__(256) void sg_sigmoid_nhwc_fwd_kernel(const float* z, int ld, int npix, int C, float* p, int pld) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        for (int c = 0; c < pld; ++c) p[(int64_t)i * pld + c] = c < C ? sg_sigmoid(z[(int64_t)i * ld + c]) : 0.f;
}

__global__ __launch_bounds__(256) void sg_sigmoid_nhwc_bwd_kernel(const float* dp, int dpld, const float* p, int pld, int npix, int C,
                                                                  float* dz, int dzld) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        for (int c = 0; c < dzld; ++c) {
            const float pv = c < C ? p[(int64_t)i * pld + c] : 0.f;
            dz[(int64_t)i * dzld + c] = c < C ? dp[(int64_t)i * dpld + c] * pv * (1.f - pv) : 0.f;
        }
}

__device__ __forceinline__ float sg_bcew_weight(const float* t, const float* cw, int nw) {
    float w = 1.f;
    for (int i = 0; i < nw; ++i) w += t[i] * (cw[i] - 1.f);
    return w;
}

// workgroup b leaves its fp64 partial in part[b]; the last one (ticket) adds them in order and leaves the ticket at zero
__global__ __launch_bounds__(256) void sg_bce_weighted_fwd_kernel(const float* p, int pld, const float* t, int tld, int npix, int C,
                                                                  const float* cw, int nw, double* part, unsigned* ticket, float* loss_out) {
    __shared__ double wsum[4];
    __shared__ int last;
    double acc = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const float* tp = t + (int64_t)i * tld;
        const float w = sg_bcew_weight(tp, cw, nw);
        float s = 0.f;
        for (int c = 0; c < C; ++c) {
            const float pv = p[(int64_t)i * pld + c], tv = tp[c];
            s += sg_bce_term(pv, tv);
        }
        acc += (double)w * (double)s;
    }
    const double mine = sg_block_sum<4>(acc, wsum);
    if (!sg_publish_last(mine, &part[blockIdx.x], ticket, gridDim.x - 1, &last) || threadIdx.x != 0) return;
    __threadfence();
    double sum = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) sum += sg_slot_load(&part[b]);
    loss_out[0] = (float)(sum / ((double)C * (double)npix));
    ticket[0] = 0u;
}

__global__ __launch_bounds__(256) void sg_bce_weighted_bwd_kernel(const float* p, int pld, const float* t, int tld, int npix, int C,
                                                                  const float* cw, int nw, const float* gout, float* dp, int dpld) {
    const float go = gout[0] / ((float)C * (float)npix);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const float* tp = t + (int64_t)i * tld;
        const float w = sg_bcew_weight(tp, cw, nw) * go;
        for (int c = 0; c < dpld; ++c) {
            float d = 0.f;
            if (c < C) {
                const float pv = p[(int64_t)i * pld + c];
                d = w * (pv - tp[c]) / sg_bce_dden(pv);
            }
            dp[(int64_t)i * dpld + c] = d;
        }
    }
}

extern "C" int sgan_sigmoid_nhwc_fwd(const float* z, int32_t ld, int32_t npix, int32_t C, float* p, int32_t pld, void* stream) {
    SGAN_CHECK(z && p && npix > 0 && C >= 1 && C <= SG_BCEW_MAXC && ld >= C && pld >= C, "bad argument (1..%d channels)", SG_BCEW_MAXC);
    int blocks = sg_cdiv(npix, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sg_sigmoid_nhwc_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, z, ld, npix, C, p, pld);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_sigmoid_nhwc_bwd(const float* dp, int32_t dpld, const float* p, int32_t pld, int32_t npix, int32_t C, float* dz,
                                     int32_t dzld, void* stream) {
    SGAN_CHECK(dp && p && dz && npix > 0 && C >= 1 && C <= SG_BCEW_MAXC && dpld >= C && pld >= C && dzld >= C, "bad argument");
    int blocks = sg_cdiv(npix, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sg_sigmoid_nhwc_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dp, dpld, p, pld, npix, C, dz, dzld);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

#define SG_BCEW_BLOCKS 64
extern "C" int sgan_bce_weighted_fwd(const float* p, int32_t pld, const float* t, int32_t tld, int32_t npix, int32_t C,
                                     const float* class_w, int32_t nw, float* loss_out, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    SGAN_CHECK(p && t && loss_out && npix > 0 && C >= 1 && C <= SG_BCEW_MAXC && pld >= C && tld >= C, "bad argument (1..%d channels)",
               SG_BCEW_MAXC);
    SGAN_CHECK(nw >= 0 && nw <= C && (nw == 0 || class_w), "0..C class weights");
    SGAN_CHECK(workspace && workspace_bytes >= SGAN_BCE_WEIGHTED_WS_BYTES && ((uintptr_t)workspace & 7) == 0,
               "workspace of SGAN_BCE_WEIGHTED_WS_BYTES (8-byte aligned) required");
    static_assert((SG_BCEW_BLOCKS + 1) * sizeof(double) <= SGAN_BCE_WEIGHTED_WS_BYTES, "workspace size");
    double* part = static_cast<double*>(workspace);
    unsigned* ticket = reinterpret_cast<unsigned*>(part + SG_BCEW_BLOCKS);
    int blocks = sg_cdiv(npix, 256);
    if (blocks > SG_BCEW_BLOCKS) blocks = SG_BCEW_BLOCKS;
    hipLaunchKernelGGL(sg_bce_weighted_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, pld, t, tld, npix, C, class_w, nw,
                       part, ticket, loss_out);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_bce_weighted_bwd(const float* p, int32_t pld, const float* t, int32_t tld, int32_t npix, int32_t C,
                                     const float* class_w, int32_t nw, const float* gout, float* dp, int32_t dpld, void* stream) {
    SGAN_CHECK(p && t && gout && dp && npix > 0 && C >= 1 && C <= SG_BCEW_MAXC && pld >= C && tld >= C && dpld >= C, "bad argument");
    SGAN_CHECK(nw >= 0 && nw <= C && (nw == 0 || class_w), "0..C class weights");
    int blocks = sg_cdiv(npix, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(sg_bce_weighted_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, pld, t, tld, npix, C, class_w, nw,
                       gout, dp, dpld);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}
