// The loss section of a segmentation step that has no discriminator behind the prediction (`--which_model_netD None`,
// models/segm_model.py:203-228 with loss_G = loss_G_CE): the channel softmax (or sigmoid) that turns the U-Net's logits into the
// prediction, the class-weighted cross-entropy (or weighted BCE) against the label, and d loss / d logits, in ONE pass over the logits.
// The composition it replaces reads the logits three or four times (sgan_softmax_fwd, sgan_ce_fwd, sgan_ce_bwd; or sgan_sigmoid_nhwc_fwd,
// sgan_bce_weighted_fwd, sgan_bce_weighted_bwd, sgan_sigmoid_nhwc_bwd) and takes the exponentials up to three times.  Valid only while the
// loss is the one consumer of the prediction: a gradient arriving at p from elsewhere has no way into dlogits (losses.seg_head asserts it).
//
// One thread per pixel, 256-thread workgroups, grid-stride.  With 4-, 8-, 12- or 16-channel storage on every operand (and 16-byte aligned
// bases) a pixel is one to four 16-byte loads and as many stores per output; any other layout takes the scalar form of the same
// arithmetic.  Every workgroup leaves its fp64 partial in a slot of its own and draws a ticket (its one atomic); the last one sums the
// slots in a fixed order -- the same bits on every run --, writes the loss, and leaves the workspace zeroed for the next call.
#include "sgan_reduce.h"

#define SG_SH_MAXC 16
#define SG_SH_BLOCKS 512
static_assert((SG_SH_BLOCKS + 1) * sizeof(double) <= SGAN_SEGHEAD_WS_BYTES, "workspace size");

struct ShArgs {
    const float* z; int ld;
    int npix, C, mode;
    const int64_t* label;              // SGAN_SEGHEAD_SOFTMAX
    const float* t; int tld;           // SGAN_SEGHEAD_SIGMOID
    const float* cw; int nw;
    const float* padd;                 // PW kernels: added to the class weight of every pixel whose label is in range
    const float* norm;
    float* p; int pld;
    float* d; int dld;                 // d == nullptr: no gradient
    float* loss;
    double* part; unsigned* ticket;
};

// CS > 0: the row is CS floats at a 16-byte aligned address; CS == 0: `n` floats `ld` apart from their neighbours' rows, the rest zero
template <int CS>
__device__ __forceinline__ void sh_load_row(const float* base, int64_t pix, int ld, int n, float (&v)[CS ? CS : SG_SH_MAXC]) {
    if constexpr (CS > 0) {
        const f32x4* src = reinterpret_cast<const f32x4*>(base + pix * CS);
#pragma unroll
        for (int q = 0; q < CS / 4; ++q) {
            const f32x4 x = src[q];
            v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < SG_SH_MAXC; ++c) v[c] = c < n ? base[pix * ld + c] : 0.f;
    }
}

// v[c >= C] is zero already: the padding channels are written as zeros
template <int CS>
__device__ __forceinline__ void sh_store_row(float* base, int64_t pix, int ld, const float (&v)[CS ? CS : SG_SH_MAXC]) {
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
        for (int c = 0; c < SG_SH_MAXC; ++c)
            if (c < ld) base[pix * ld + c] = v[c];
        for (int c = SG_SH_MAXC; c < ld; ++c) base[pix * ld + c] = 0.f;
    }
}

// The workgroup's sum goes through the hand-off of sgan_reduce.h; false in every workgroup but the last to arrive.  There `total` is
// the sum of all slots in a fixed order (a strided sum per thread, then the workgroup sum) and the slots are zero again.
__device__ __forceinline__ bool sh_total(double acc, double* part, unsigned* ticket, double* red, int* last, double& total) {
    const double sum = sg_block_sum<4>(acc, red);
    if (!sg_publish_last(sum, &part[blockIdx.x], ticket, gridDim.x - 1, last)) return false;      // its barrier frees `red`
    __threadfence();
    double v = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += 256) {
        v += sg_slot_load(&part[b]);
        part[b] = 0.0;
    }
    total = sg_block_sum<4>(v, red);
    return true;
}

// PW (softmax mode only): the weight of pixel i is cw[y_i] + padd[i]
template <int CS, bool PW>
__global__ __launch_bounds__(256) void sg_seg_head_kernel(const ShArgs A) {
    constexpr int N = CS ? CS : SG_SH_MAXC;
    __shared__ double red[4];
    __shared__ int last;
    const int C = A.C;
    const bool softmax = A.mode == SGAN_SEGHEAD_SOFTMAX;
    float cw[N];
    const int ncw = A.cw ? (softmax ? C : A.nw) : 0;
#pragma unroll
    for (int c = 0; c < N; ++c) cw[c] = c < ncw ? A.cw[c] : 1.f;
    float scale;      // what every gradient element is multiplied with beside its pixel's weight
    if (softmax) {
        const float n = A.norm[0];
        scale = n > 0.f ? 1.f / n : 0.f;
    } else {
        scale = 1.f / ((float)C * (float)A.npix);
    }
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.npix; i += (int64_t)gridDim.x * 256) {
        float z[N], p[N], d[N];
        sh_load_row<CS>(A.z, i, A.ld, C, z);
        if (softmax) {
            const int64_t yl = A.label[i];
            const bool ok = yl >= 0 && yl < C;      // torch's ignore_index (-100) and anything out of range: no contribution
            const int y = ok ? (int)yl : -1;
            float m = -3.4e38f;
#pragma unroll
            for (int c = 0; c < N; ++c) m = c < C ? fmaxf(m, z[c]) : m;
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < N; ++c) { p[c] = c < C ? expf(z[c] - m) : 0.f; sum += p[c]; }
            const float inv = 1.f / sum, lse = m + logf(sum);
            float zy = 0.f, w = 0.f;
#pragma unroll
            for (int c = 0; c < N; ++c) { zy = c == y ? z[c] : zy; w = c == y ? cw[c] : w; }
            if constexpr (PW) w = ok ? w + A.padd[i] : 0.f;
            const float ws = w * scale;
#pragma unroll
            for (int c = 0; c < N; ++c) {
                p[c] *= inv;
                d[c] = c < C ? ws * (p[c] - (c == y ? 1.f : 0.f)) : 0.f;
            }
            if (ok) acc += (double)(w * (lse - zy));
        } else {
            float t[N];
            sh_load_row<CS>(A.t, i, A.tld, C, t);
            float w = 1.f;
#pragma unroll
            for (int c = 0; c < N; ++c) w += c < ncw ? t[c] * (cw[c] - 1.f) : 0.f;
            const float ws = w * scale;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < N; ++c) {
                float pv = 0.f, dv = 0.f;
                if (c < C) {
                    pv = sg_sigmoid(z[c]);
                    const float tv = t[c];
                    s += sg_bce_term(pv, tv);
                    dv = ws * (pv - tv) / sg_bce_dden(pv) * pv * (1.f - pv);      // sgan_bce_weighted_bwd, then sgan_sigmoid_nhwc_bwd
                }
                p[c] = pv;
                d[c] = dv;
            }
            acc += (double)w * (double)s;
        }
        sh_store_row<CS>(A.p, i, A.pld, p);
        if (A.d) sh_store_row<CS>(A.d, i, A.dld, d);
    }
    double total;
    if (!sh_total(acc, A.part, A.ticket, red, &last, total)) return;
    if (threadIdx.x == 0) {
        if (softmax) {
            const double n = (double)A.norm[0];
            A.loss[0] = n > 0.0 ? (float)(total / n) : 0.f;
        } else {
            A.loss[0] = (float)(total / ((double)C * (double)A.npix));
        }
        A.ticket[0] = 0u;
    }
}

template <bool PW>
__global__ __launch_bounds__(256) void sg_label_weight_sum_kernel(const int64_t* label, int npix, int C, const float* class_w,
                                                                  const float* pixel_add, float* out, double* part, unsigned* ticket) {
    __shared__ double red[4];
    __shared__ int last;
    float cw[SG_SH_MAXC];
#pragma unroll
    for (int c = 0; c < SG_SH_MAXC; ++c) cw[c] = (class_w && c < C) ? class_w[c] : 1.f;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const int64_t yl = label[i];
        const int y = (yl >= 0 && yl < C) ? (int)yl : -1;
        float w = 0.f;
#pragma unroll
        for (int c = 0; c < SG_SH_MAXC; ++c) w = c == y ? cw[c] : w;
        if constexpr (PW) w = y >= 0 ? w + pixel_add[i] : 0.f;      // the weight sg_seg_head_kernel<., true> gives the pixel
        acc += (double)w;
    }
    double total;
    if (!sh_total(acc, part, ticket, red, &last, total)) return;
    if (threadIdx.x == 0) {
        out[0] = (float)total;
        ticket[0] = 0u;
    }
}

static inline bool sh_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int sh_weight_sum(const int64_t* label, int32_t npix, int32_t C, const float* class_w, const float* pixel_add, float* out,
                         void* workspace, void* stream) {
    SGAN_CHECK(npix > 0 && C >= 1, "bad argument (1..%d classes)", SG_SH_MAXC);
    SGAN_CHECK(((uintptr_t)workspace & 7) == 0, "workspace of SGAN_SEGHEAD_WS_BYTES (8-byte aligned) required");
    double* part = static_cast<double*>(workspace);
    unsigned* ticket = reinterpret_cast<unsigned*>(part + SG_SH_BLOCKS);
    int blocks = sg_cdiv(npix, 256);
    if (blocks > SG_SH_BLOCKS) blocks = SG_SH_BLOCKS;
    if (pixel_add)
        hipLaunchKernelGGL(sg_label_weight_sum_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, label, npix, C, class_w, pixel_add,
                           out, part, ticket);
    else
        hipLaunchKernelGGL(sg_label_weight_sum_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, label, npix, C, class_w, pixel_add,
                           out, part, ticket);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_label_weight_sum(const int64_t* label, int32_t npix, int32_t C, const float* class_w, float* out, void* workspace,
                                     void* stream) {
    if (!label || !out || !workspace || C > SG_SH_MAXC) return 1;
    return sh_weight_sum(label, npix, C, class_w, nullptr, out, workspace, stream);
}

extern "C" int sgan_pixel_weight_sum(const int64_t* label, int32_t npix, int32_t C, const float* class_w, const float* pixel_add, float* out,
                                     void* workspace, void* stream) {
    if (!label || !pixel_add || !out || !workspace || C > SG_SH_MAXC) return 1;
    return sh_weight_sum(label, npix, C, class_w, pixel_add, out, workspace, stream);
}

// cs: the channels of a 16-byte row layout (4, 8, 12, 16), or 0 for the scalar form
template <bool PW>
static void sh_launch(int cs, int blocks, hipStream_t st, const ShArgs& A) {
    const dim3 g(blocks), b(256);
    if (cs == 4) hipLaunchKernelGGL((sg_seg_head_kernel<4, PW>), g, b, 0, st, A);
    else if (cs == 8) hipLaunchKernelGGL((sg_seg_head_kernel<8, PW>), g, b, 0, st, A);
    else if (cs == 12) hipLaunchKernelGGL((sg_seg_head_kernel<12, PW>), g, b, 0, st, A);
    else if (cs == 16) hipLaunchKernelGGL((sg_seg_head_kernel<16, PW>), g, b, 0, st, A);
    else hipLaunchKernelGGL((sg_seg_head_kernel<0, PW>), g, b, 0, st, A);
}

// what sgan_seg_head and sgan_seg_head_pw share: the argument checks and the launch; pixel_add != NULL selects the PW kernels
static int sh_head(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                   const float* class_w, int32_t nw, const float* pixel_add, const float* norm, float* p_out, int32_t pld, float* dlogits,
                   int32_t dld, float* loss_out, void* workspace, void* stream) {
    const bool softmax = mode == SGAN_SEGHEAD_SOFTMAX;
    SGAN_CHECK(npix > 0 && C >= 1 && ld >= C && pld >= C && (!dlogits || dld >= C), "bad argument (1..%d channels)", SG_SH_MAXC);
    SGAN_CHECK(softmax || tld >= C, "target rows shorter than C");
    SGAN_CHECK(nw >= 0 && (!class_w || (softmax ? nw >= C : nw <= C)) && (class_w || softmax || nw == 0),
               "class weights: C of them (softmax), 0..C (sigmoid)");
    SGAN_CHECK(((uintptr_t)workspace & 7) == 0, "workspace of SGAN_SEGHEAD_WS_BYTES (8-byte aligned) required");
    ShArgs A;
    A.z = logits; A.ld = ld; A.npix = npix; A.C = C; A.mode = mode;
    A.label = softmax ? static_cast<const int64_t*>(label_or_target) : nullptr;
    A.t = softmax ? nullptr : static_cast<const float*>(label_or_target);
    A.tld = tld; A.cw = class_w; A.nw = class_w ? nw : 0; A.padd = pixel_add; A.norm = norm;
    A.p = p_out; A.pld = pld; A.d = dlogits; A.dld = dld; A.loss = loss_out;
    A.part = static_cast<double*>(workspace);
    A.ticket = reinterpret_cast<unsigned*>(A.part + SG_SH_BLOCKS);
    int blocks = sg_cdiv(npix, 256);
    if (blocks > SG_SH_BLOCKS) blocks = SG_SH_BLOCKS;
    // 16-byte rows: every operand stored with the same 4, 8, 12 or 16 channels, on aligned bases
    const bool vec = (ld == 4 || ld == 8 || ld == 12 || ld == 16) && pld == ld && (!dlogits || dld == ld) && (softmax || tld == ld) && sh_al16(logits) &&
                     sh_al16(p_out) && sh_al16(dlogits) && (softmax || sh_al16(label_or_target));
    if (pixel_add) sh_launch<true>(vec ? ld : 0, blocks, (hipStream_t)stream, A);
    else sh_launch<false>(vec ? ld : 0, blocks, (hipStream_t)stream, A);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_seg_head(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                             int32_t tld, const float* class_w, int32_t nw, const float* norm, float* p_out, int32_t pld, float* dlogits,
                             int32_t dld, float* loss_out, void* workspace, void* stream) {
    if (!logits || !label_or_target || !p_out || !loss_out || !workspace || C > SG_SH_MAXC) return 1;
    SGAN_CHECK(mode == SGAN_SEGHEAD_SOFTMAX || mode == SGAN_SEGHEAD_SIGMOID, "mode is SGAN_SEGHEAD_SOFTMAX or SGAN_SEGHEAD_SIGMOID");
    if (mode == SGAN_SEGHEAD_SOFTMAX && !norm) return 1;
    return sh_head(logits, ld, npix, C, mode, label_or_target, tld, class_w, nw, nullptr, norm, p_out, pld, dlogits, dld, loss_out, workspace,
                   stream);
}

extern "C" int sgan_seg_head_pw(const float* logits, int32_t ld, int32_t npix, int32_t C, const int64_t* label, const float* class_w,
                                int32_t nw, const float* pixel_add, const float* norm, float* p_out, int32_t pld, float* dlogits,
                                int32_t dld, float* loss_out, void* workspace, void* stream) {
    if (!logits || !label || !pixel_add || !norm || !p_out || !loss_out || !workspace || C > SG_SH_MAXC) return 1;
    return sh_head(logits, ld, npix, C, SGAN_SEGHEAD_SOFTMAX, label, 0, class_w, nw, pixel_add, norm, p_out, pld, dlogits, dld, loss_out,
                   workspace, stream);
}
