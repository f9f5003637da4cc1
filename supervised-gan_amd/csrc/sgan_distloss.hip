// Distance-map loss terms of the segmentation trainers (include/sgan_hip.h, "Distance-map loss terms"): the signed
// squared distance map of a plane, and the boundary loss (Kervadec et al., MIDL 2019) and the distance-transform Hausdorff loss
// (Karimi & Salcudean, TMI 2019, HD_DT) of one class, read from the LOGITS where the generator left them.
//
// The signed map is two calls of the library's exact transform through its public entry (sgan_edt_sq) and two streaming passes of
// this file between and behind them:
//   complement: comp = 1 where the plane is not > 0.5 (a NaN and an exact 0.5 are outside), else 0; the second transform reads it.
//   combine:    the first transform left d_out (distance^2 to the nearest inside pixel) in the caller's plane, the second d_in
//               (to the nearest outside pixel) in the workspace: sdsq = d_out where d_out > 0, -d_in on an inside pixel, and 0 where
//               either reads -1 (sgan_edt_sq's "the plane has no such pixel", the same everywhere): decided per pixel, on the device.
// Every value is an integer, so nothing depends on an order.  Workspace: [sgan_edt_sq's workspace][comp: H W float][d_in: H W int32],
// each rounded up to 16 bytes.
//
// The loss node is two streaming launches, one thread per pixel, 256-thread workgroups, grid-stride, the grid a function of npix alone:
//   sg_dist_loss_fwd_kernel   p of the class in registers (fp32), then in fp64 phi p and (p - g)^2 F; the two workgroup sums go to
//                             slots of the workgroup's own and a ticket is drawn (sgan_reduce.h); the last to arrive adds the slots in
//                             a fixed order, zeroes them, and thread 0 writes the state and both losses.
//   sg_dist_loss_bwd_kernel   the same p again, G = gout_B phi / N + gout_H 2 (p - g) F / N in fp64, rounded once; dz in fp32.
// No floating-point atomics, no workgroup waits on another, nothing read back or allocated.
#include "sgan_reduce.h"

#define SG_DL_MAXC 16
#define SG_DL_BLOCKS 512
#define SG_DL_THREADS 256
static_assert((2 * SG_DL_BLOCKS + 1) * sizeof(double) <= SGAN_DISTLOSS_WS_BYTES, "workspace size");
static_assert(5 * sizeof(double) <= SGAN_DISTLOSS_STATE_BYTES, "state size");

#define SG_DL_REFUSE(cond, ...)                         \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

// ---- the signed squared distance map --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_DL_THREADS) void sg_sedt_complement_kernel(const float* __restrict__ plane, int64_t pix_stride, int64_t n,
                                                                           float* __restrict__ comp) {
    for (int64_t i = (int64_t)blockIdx.x * SG_DL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_DL_THREADS)
        comp[i] = plane[i * pix_stride] > 0.5f ? 0.f : 1.f;      // a NaN and an exact 0.5 are outside
}

__global__ __launch_bounds__(SG_DL_THREADS) void sg_sedt_combine_kernel(const int32_t* __restrict__ d_in, int64_t n, int32_t* sdsq) {
    for (int64_t i = (int64_t)blockIdx.x * SG_DL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SG_DL_THREADS) {
        const int32_t a = sdsq[i], b = d_in[i];      // a == 0: an inside pixel; b == 0: an outside pixel; -1: no such pixel anywhere
        sdsq[i] = (a < 0 || b < 0) ? 0 : (a > 0 ? a : -b);
    }
}

struct SgSedtLayout {
    int64_t off_comp, off_din, bytes;
};

static bool sg_sedt_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (int64_t)H * W < (1ll << 30);      // sgan_edt_sq's
}

static SgSedtLayout sg_sedt_layout(int32_t H, int32_t W) {
    const int64_t plane = (4ll * H * W + 15) & ~15ll;
    SgSedtLayout l;
    l.off_comp = (sgan_edt_workspace(H, W) + 15) & ~15ll;
    l.off_din = l.off_comp + plane;
    l.bytes = l.off_din + plane;
    return l;
}

static int sg_sedt_grid(int64_t n) {
    const int64_t want = (n + SG_DL_THREADS - 1) / SG_DL_THREADS;
    return (int)(want < 2048 ? want : 2048);
}

extern "C" int64_t sgan_signed_edt_workspace(int32_t H, int32_t W) {
    if (!sg_sedt_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_sedt_layout(H, W).bytes;
}

extern "C" int sgan_signed_edt_sq(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* sdsq, void* workspace,
                                  int64_t workspace_bytes, int32_t* dev_err, void* stream) {
    SG_DL_REFUSE(plane && sdsq && workspace && dev_err, "null pointer");
    SG_DL_REFUSE(sg_sedt_shape_ok(H, W) && pix_stride >= 1, "bad shape %d x %d (H, W <= 32768, H W < 2^30), pixel stride %lld", H, W,
                 (long long)pix_stride);
    const SgSedtLayout l = sg_sedt_layout(H, W);
    SG_DL_REFUSE(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_signed_edt_workspace); nothing was launched",
                 (long long)workspace_bytes, (long long)l.bytes, H, W);
    SG_DL_REFUSE(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    float* comp = (float*)((char*)workspace + l.off_comp);
    int32_t* d_in = (int32_t*)((char*)workspace + l.off_din);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    const dim3 grid(sg_sedt_grid(n)), block(SG_DL_THREADS);
    int rc;
    // every argument of the two transforms was checked above: neither can refuse behind a launch
    if ((rc = sgan_edt_sq(plane, pix_stride, H, W, sdsq, workspace, l.off_comp, dev_err, stream)) != SGAN_OK) return rc;
    hipLaunchKernelGGL(sg_sedt_complement_kernel, grid, block, 0, st, plane, pix_stride, n, comp);
    SGAN_LAUNCH_CHECK();
    if ((rc = sgan_edt_sq(comp, 1, H, W, d_in, workspace, l.off_comp, dev_err, stream)) != SGAN_OK) return rc;
    hipLaunchKernelGGL(sg_sedt_combine_kernel, grid, block, 0, st, (const int32_t*)d_in, n, sdsq);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_sedt_combine_kernel";
    return SGAN_OK;
}

// ---- the loss node ---------------------------------------------------------------------------------------------------------------
struct DlArgs {
    const float* z; int ld;
    int npix, C, mode, cls;
    const int64_t* label;              // SGAN_SEGHEAD_SOFTMAX
    const float* t; int tld;           // SGAN_SEGHEAD_SIGMOID
    const int32_t* tmap; const int32_t* pmap;
    int boundary, hausdorff;
    double alpha;
    // forward
    double* state; float* loss_b; float* loss_h;
    double* part; unsigned* ticket;
    // backward
    const float* gout_b; const float* gout_h;
    float* d; int dld;
};

// CS > 0: the row is CS floats at a 16-byte aligned address; CS == 0: `n` floats `ld` apart from their neighbours' rows, the rest zero
template <int CS>
__device__ __forceinline__ void dl_load_row(const float* base, int64_t pix, int ld, int n, float (&v)[CS ? CS : SG_DL_MAXC]) {
    if constexpr (CS > 0) {
        const f32x4* src = reinterpret_cast<const f32x4*>(base + pix * CS);
#pragma unroll
        for (int q = 0; q < CS / 4; ++q) {
            const f32x4 x = src[q];
            v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < SG_DL_MAXC; ++c) v[c] = c < n ? base[pix * ld + c] : 0.f;
    }
}

// v[c >= C] is zero already: the padding channels are written as zeros
template <int CS>
__device__ __forceinline__ void dl_store_row(float* base, int64_t pix, int ld, const float (&v)[CS ? CS : SG_DL_MAXC]) {
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
        for (int c = 0; c < SG_DL_MAXC; ++c)
            if (c < ld) base[pix * ld + c] = v[c];
        for (int c = SG_DL_MAXC; c < ld; ++c) base[pix * ld + c] = 0.f;
    }
}

// softmax over the first C of N channels; returns p of channel `cls`, and in `om` 1 - p taken as the sum of the other channels'
// exponentials over the whole sum (no cancellation near p = 1)
template <int N>
__device__ __forceinline__ float dl_softmax(const float (&z)[N], int C, int cls, float (&p)[N], float& om) {
    float m = -3.4e38f;
#pragma unroll
    for (int c = 0; c < N; ++c) m = c < C ? fmaxf(m, z[c]) : m;
    float sum = 0.f, others = 0.f;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        p[c] = c < C ? expf(z[c] - m) : 0.f;
        sum += p[c];
        others += c == cls ? 0.f : p[c];
    }
    const float inv = 1.f / sum;
    om = others * inv;
    float pc = 0.f;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        p[c] *= inv;
        pc = c == cls ? p[c] : pc;
    }
    return pc;
}

// Kervadec's level set from the signed squared map: the distance outside, -(distance - 1) inside, 0 where the map is 0
__device__ __forceinline__ double dl_phi(int s) {
    return s > 0 ? sqrt((double)s) : (s < 0 ? 1.0 - sqrt(-(double)s) : 0.0);
}

// F = |t|^(alpha / 2) + |p|^(alpha / 2); at alpha == 2 the exact integer |t| + |p| < 2^32
__device__ __forceinline__ double dl_field(int t, int p, double alpha) {
    const double a = fabs((double)t), b = fabs((double)p);
    if (alpha == 2.0) return a + b;
    const double h = 0.5 * alpha;
    return (a > 0.0 ? pow(a, h) : 0.0) + (b > 0.0 ? pow(b, h) : 0.0);
}

template <int CS>
__global__ __launch_bounds__(SG_DL_THREADS) void sg_dist_loss_fwd_kernel(const DlArgs A) {
    constexpr int N = CS ? CS : SG_DL_MAXC;
    __shared__ double red[4];
    __shared__ int last;
    const int C = A.C, cls = A.cls;
    const bool softmax = A.mode == SGAN_SEGHEAD_SOFTMAX;
    const bool boundary = A.boundary != 0, hausdorff = A.hausdorff != 0;
    double sb = 0.0, sh = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SG_DL_THREADS + threadIdx.x; i < A.npix; i += (int64_t)gridDim.x * SG_DL_THREADS) {
        float pc, g;
        if (softmax) {
            const int64_t yl = A.label[i];
            if (yl < 0 || yl >= C) continue;      // torch's ignore_index (-100) and anything out of range: no contribution to any sum
            float z[N], p[N], om;
            dl_load_row<CS>(A.z, i, A.ld, C, z);
            pc = dl_softmax<N>(z, C, cls, p, om);
            g = yl == cls ? 1.f : 0.f;
        } else {
            pc = sg_sigmoid(A.z[i * A.ld + cls]);
            g = A.t[i * A.tld + cls];
        }
        const int s = A.tmap[i];
        if (boundary) sb += dl_phi(s) * (double)pc;
        if (hausdorff) {
            const double e = (double)pc - (double)g;
            sh += e * e * dl_field(s, A.pmap[i], A.alpha);
        }
    }
    double* part = A.part;
    const double tb = sg_block_sum<4>(sb, red);
    SG_SYNC();      // frees `red` for the second sum
    if (threadIdx.x == 0) part[blockIdx.x] = tb;
    const double th = sg_block_sum<4>(sh, red);
    // thread 0 wrote the first slot above; sg_publish_last stores the second, fences behind both and takes the ticket
    if (!sg_publish_last(th, &part[SG_DL_BLOCKS + blockIdx.x], A.ticket, gridDim.x - 1, &last)) return;
    __threadfence();
    double S[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double v = 0.0;
        for (unsigned b = threadIdx.x; b < gridDim.x; b += SG_DL_THREADS) {
            v += sg_slot_load(&part[k * SG_DL_BLOCKS + b]);
            part[k * SG_DL_BLOCKS + b] = 0.0;
        }
        SG_SYNC();      // every thread has read `red` of the sum before
        S[k] = sg_block_sum<4>(v, red);
    }
    if (threadIdx.x != 0) return;
    const double n = (double)A.npix;
    const double LB = boundary ? S[0] / n : 0.0, LH = hausdorff ? S[1] / n : 0.0;
    double* st = A.state;
    st[0] = S[0]; st[1] = S[1]; st[2] = n; st[3] = LB; st[4] = LH;
    A.loss_b[0] = (float)LB;
    A.loss_h[0] = (float)LH;
    A.ticket[0] = 0u;
}

template <int CS>
__global__ __launch_bounds__(SG_DL_THREADS) void sg_dist_loss_bwd_kernel(const DlArgs A) {
    constexpr int N = CS ? CS : SG_DL_MAXC;
    const int C = A.C, cls = A.cls;
    const bool softmax = A.mode == SGAN_SEGHEAD_SOFTMAX;
    const bool boundary = A.boundary != 0 && A.gout_b != nullptr, hausdorff = A.hausdorff != 0 && A.gout_h != nullptr;
    const double inv_n = 1.0 / (double)A.npix;
    const double ub = boundary ? (double)A.gout_b[0] * inv_n : 0.0;
    const double uh = hausdorff ? 2.0 * (double)A.gout_h[0] * inv_n : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SG_DL_THREADS + threadIdx.x; i < A.npix; i += (int64_t)gridDim.x * SG_DL_THREADS) {
        float d[N];
#pragma unroll
        for (int c = 0; c < N; ++c) d[c] = 0.f;
        bool ok = boundary || hausdorff;
        int64_t yl = 0;
        if (softmax) {
            yl = A.label[i];
            ok = ok && yl >= 0 && yl < C;
        }
        if (ok) {
            float z[N], p[N], pc, g, om = 0.f;
            if (softmax) {
                dl_load_row<CS>(A.z, i, A.ld, C, z);
                pc = dl_softmax<N>(z, C, cls, p, om);
                g = yl == cls ? 1.f : 0.f;
            } else {
                pc = sg_sigmoid(A.z[i * A.ld + cls]);
                g = A.t[i * A.tld + cls];
            }
            const int s = A.tmap[i];
            double G = 0.0;
            if (boundary) G = ub * dl_phi(s);
            if (hausdorff) G += uh * ((double)pc - (double)g) * dl_field(s, A.pmap[i], A.alpha);
            const float Gp = (float)G * pc;
            if (softmax) {
#pragma unroll
                for (int c = 0; c < N; ++c) d[c] = c < C ? (c == cls ? Gp * om : -(Gp * p[c])) : 0.f;
            } else {
                const float dv = Gp * sg_sigmoid(-A.z[i * A.ld + cls]);      // 1 - p without the cancellation
#pragma unroll
                for (int c = 0; c < N; ++c) d[c] = c == cls ? dv : 0.f;
            }
        }
        dl_store_row<CS>(A.d, i, A.dld, d);
    }
}

static inline bool dl_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool FWD>
static void dl_launch(int cs, int blocks, hipStream_t st, const DlArgs& A) {
    const dim3 g(blocks), b(SG_DL_THREADS);
    if constexpr (FWD) {
        if (cs == 4) hipLaunchKernelGGL((sg_dist_loss_fwd_kernel<4>), g, b, 0, st, A);
        else if (cs == 8) hipLaunchKernelGGL((sg_dist_loss_fwd_kernel<8>), g, b, 0, st, A);
        else if (cs == 12) hipLaunchKernelGGL((sg_dist_loss_fwd_kernel<12>), g, b, 0, st, A);
        else if (cs == 16) hipLaunchKernelGGL((sg_dist_loss_fwd_kernel<16>), g, b, 0, st, A);
        else hipLaunchKernelGGL((sg_dist_loss_fwd_kernel<0>), g, b, 0, st, A);
    } else {
        if (cs == 4) hipLaunchKernelGGL((sg_dist_loss_bwd_kernel<4>), g, b, 0, st, A);
        else if (cs == 8) hipLaunchKernelGGL((sg_dist_loss_bwd_kernel<8>), g, b, 0, st, A);
        else if (cs == 12) hipLaunchKernelGGL((sg_dist_loss_bwd_kernel<12>), g, b, 0, st, A);
        else if (cs == 16) hipLaunchKernelGGL((sg_dist_loss_bwd_kernel<16>), g, b, 0, st, A);
        else hipLaunchKernelGGL((sg_dist_loss_bwd_kernel<0>), g, b, 0, st, A);
    }
}

// what both entries check and fill; 1 with the reason set: not covered, nothing to launch
static int dl_common(DlArgs& A, const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                     int32_t tld, int32_t cls, const int32_t* t_sdsq, const int32_t* p_sdsq, int32_t boundary, int32_t hausdorff,
                     double alpha) {
    SG_DL_REFUSE(C >= 1 && C <= SG_DL_MAXC, "not covered: %d channels (1 .. %d)", C, SG_DL_MAXC);
    SG_DL_REFUSE(boundary || hausdorff, "not covered: both terms are off (boundary and hausdorff are 0)");
    SG_DL_REFUSE(logits && label_or_target && t_sdsq && (!hausdorff || p_sdsq), "null pointer");
    SG_DL_REFUSE(mode == SGAN_SEGHEAD_SOFTMAX || mode == SGAN_SEGHEAD_SIGMOID, "mode is SGAN_SEGHEAD_SOFTMAX or SGAN_SEGHEAD_SIGMOID");
    SG_DL_REFUSE(npix > 0 && ld >= C && (mode == SGAN_SEGHEAD_SOFTMAX || tld >= C), "bad argument: %d pixels, rows of %d and %d for %d channels", npix,
                 ld, tld, C);
    SG_DL_REFUSE(cls >= 0 && cls < C, "class %d is not below C = %d", cls, C);
    if (hausdorff) SG_DL_REFUSE(alpha > 0.0 && alpha <= 4.0, "Hausdorff exponent: 0 < alpha <= 4 (got %g)", alpha);      // a NaN fails the comparison
    const bool softmax = mode == SGAN_SEGHEAD_SOFTMAX;
    A.z = logits; A.ld = ld; A.npix = npix; A.C = C; A.mode = mode; A.cls = cls;
    A.label = softmax ? static_cast<const int64_t*>(label_or_target) : nullptr;
    A.t = softmax ? nullptr : static_cast<const float*>(label_or_target);
    A.tld = tld;
    A.tmap = t_sdsq; A.pmap = hausdorff ? p_sdsq : nullptr;
    A.boundary = boundary ? 1 : 0; A.hausdorff = hausdorff ? 1 : 0;
    A.alpha = hausdorff ? alpha : 2.0;
    A.state = nullptr; A.loss_b = A.loss_h = nullptr; A.part = nullptr; A.ticket = nullptr;
    A.gout_b = A.gout_h = nullptr; A.d = nullptr; A.dld = 0;
    return SGAN_OK;
}

static int dl_blocks(int32_t npix) {
    const int blocks = sg_cdiv(npix, SG_DL_THREADS);
    return blocks > SG_DL_BLOCKS ? SG_DL_BLOCKS : blocks;
}

static inline bool dl_row4(int ld) { return ld == 4 || ld == 8 || ld == 12 || ld == 16; }

extern "C" int sgan_dist_loss_forward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                                      int32_t tld, int32_t cls, const int32_t* t_sdsq, const int32_t* p_sdsq, int32_t boundary,
                                      int32_t hausdorff, double alpha, double* state, float* loss_boundary, float* loss_hausdorff,
                                      void* workspace, void* stream) {
    DlArgs A;
    if (int rc = dl_common(A, logits, ld, npix, C, mode, label_or_target, tld, cls, t_sdsq, p_sdsq, boundary, hausdorff, alpha)) return rc;
    SG_DL_REFUSE(state && loss_boundary && loss_hausdorff && workspace, "null pointer");
    SG_DL_REFUSE(((uintptr_t)state & 7) == 0, "state not 8-byte aligned");
    SG_DL_REFUSE(((uintptr_t)workspace & 7) == 0, "workspace of SGAN_DISTLOSS_WS_BYTES (8-byte aligned) required");
    A.state = state; A.loss_b = loss_boundary; A.loss_h = loss_hausdorff;
    A.part = static_cast<double*>(workspace);
    A.ticket = reinterpret_cast<unsigned*>(A.part + 2 * SG_DL_BLOCKS);
    // the sigmoid form reads one float of the row: it has no use for the vector form
    const bool vec = mode == SGAN_SEGHEAD_SOFTMAX && dl_row4(ld) && dl_al16(logits);
    dl_launch<true>(vec ? ld : 0, dl_blocks(npix), (hipStream_t)stream, A);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_dist_loss_fwd_kernel";
    return SGAN_OK;
}

extern "C" int sgan_dist_loss_backward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target,
                                       int32_t tld, int32_t cls, const int32_t* t_sdsq, const int32_t* p_sdsq, int32_t boundary,
                                       int32_t hausdorff, double alpha, const float* gout_boundary, const float* gout_hausdorff,
                                       float* dlogits, int32_t dld, void* stream) {
    DlArgs A;
    if (int rc = dl_common(A, logits, ld, npix, C, mode, label_or_target, tld, cls, t_sdsq, p_sdsq, boundary, hausdorff, alpha)) return rc;
    SG_DL_REFUSE(dlogits, "null pointer");
    SG_DL_REFUSE(dld >= C, "gradient rows of %d for %d channels", dld, C);
    A.gout_b = gout_boundary; A.gout_h = gout_hausdorff; A.d = dlogits; A.dld = dld;
    // softmax: logits and gradient rows alike; sigmoid: the logit is one scalar load, the gradient rows alone decide
    const bool vec = dl_row4(dld) && dl_al16(dlogits) && (mode == SGAN_SEGHEAD_SIGMOID || (ld == dld && dl_al16(logits)));
    dl_launch<false>(vec ? dld : 0, dl_blocks(npix), (hipStream_t)stream, A);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_dist_loss_bwd_kernel";
    return SGAN_OK;
}
