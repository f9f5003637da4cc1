// Differentiable augmentation of discriminator inputs (include/sgan_hip.h, "differentiable augmentation"): the
// parameter draw, and the forward / backward transform of up to 8 padded NHWC images per call.  Streaming kernels: a lane moves one
// group of 4 stored channels (16 bytes) per step; a translated read stays 16-byte aligned because shifts are whole pixels.
#include "sgan_reduce.h"
#include "sgan_philox.h"

#define SG_DA_SLOTS 256       // partial sums (workgroups of the first launch) per job at most
#define SG_DA_CHUNK 1024      // groups per workgroup of the first launch at least: 4 per lane
#define SG_DA_MAX_BLOCKS 2048

// a refused call: the reason goes to sgan_last_error, the entry returns 1 and has launched nothing
#define SG_DA_REFUSE(cond, ...)                         \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

struct SgDaJob {
    const float* src;
    float* dst;
    int32_t H, W, C, G;      // G = Cs / 4 groups per pixel
    uint32_t mask;
    int32_t ncol;            // set bits of mask
    int32_t groups;          // H * W * G
    int32_t nb;              // workgroups of the first launch = slots used
};
struct SgDaArgs { SgDaJob job[SGAN_DIFFAUG_MAX_JOBS]; };
struct SgDaDraw { int32_t H[SGAN_DIFFAUG_MAX_JOBS], W[SGAN_DIFFAUG_MAX_JOBS], Sy[SGAN_DIFFAUG_MAX_JOBS], Sx[SGAN_DIFFAUG_MAX_JOBS],
                  ch[SGAN_DIFFAUG_MAX_JOBS], cw[SGAN_DIFFAUG_MAX_JOBS]; };

// ---- the draw: one workgroup, lane j makes record j ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sg_diffaug_draw_kernel(sgan_diffaug_rec* out, SgDaDraw d, int njobs, int policy, uint64_t seed,
                                                            uint64_t* offset, int advance) {
    const uint64_t off = offset ? offset[0] : 0;
    SG_SYNC();      // every lane has read the offset before lane 0 moves it
    if (threadIdx.x == 0 && offset && advance) offset[0] = off + 2ull * (uint64_t)njobs;
    const int j = threadIdx.x;
    if (j >= njobs) return;
    uint32_t w[8];
    const uint64_t c = off + 2ull * (uint64_t)j;
    sg_philox((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    sg_philox((uint32_t)(c + 1), (uint32_t)((c + 1) >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w + 4);
    sgan_diffaug_rec r;
    r.b = (policy & SGAN_DIFFAUG_BRIGHTNESS) ? (float)(w[0] >> 8) * (1.0f / 16777216.0f) - 0.5f : 0.f;      // exact in fp32
    r.a = (policy & SGAN_DIFFAUG_CONTRAST) ? (float)(w[1] >> 8) * (1.0f / 16777216.0f) + 0.5f : 1.f;
    r.ty = r.tx = 0;
    if (policy & SGAN_DIFFAUG_TRANSLATION) {
        r.ty = -d.Sy[j] + (int32_t)(w[2] % (uint32_t)(2 * d.Sy[j] + 1));
        r.tx = -d.Sx[j] + (int32_t)(w[3] % (uint32_t)(2 * d.Sx[j] + 1));
    }
    r.cy0 = r.cy1 = r.cx0 = r.cx1 = 0;
    if (policy & SGAN_DIFFAUG_CUTOUT) {
        const int H = d.H[j], W = d.W[j], ch = d.ch[j], cw = d.cw[j];
        const int oy = (int)(w[4] % (uint32_t)(H + 1 - (ch & 1))), ox = (int)(w[5] % (uint32_t)(W + 1 - (cw & 1)));
        r.cy0 = max(0, oy - ch / 2);
        r.cy1 = min(H, oy - ch / 2 + ch);
        r.cx0 = max(0, ox - cw / 2);
        r.cx1 = min(W, ox - cw / 2 + cw);
    }
    out[j] = r;
}

// K of the OUTPUT pixel (h, w) whose source is (h + ty, w + tx)
__device__ __forceinline__ bool sg_da_visible(const sgan_diffaug_rec& r, int h, int w, int H, int W) {
    const int sh = h + r.ty, sw = w + r.tx;
    const bool cut = h >= r.cy0 && h < r.cy1 && w >= r.cx0 && w < r.cx1;
    return !cut && sh >= 0 && sh < H && sw >= 0 && sw < W;
}

// ---- first launch of the contrast form: workgroup (b, j) leaves the fp64 sum of its share of job j in slot j * SG_DA_SLOTS + b.
// Forward: every colour element of x.  Backward: K(q) dy[q][c] over the colour channels, pixels with K = 0 not read.  A lane adds its
// elements in index order, the workgroup sums its lanes with sg_block_sum: the order depends on the shape alone.
template <bool BWD>
__global__ __launch_bounds__(256) void sg_diffaug_sum_kernel(SgDaArgs A, const sgan_diffaug_rec* recs, double* slots) {
    __shared__ double red[4];
    const SgDaJob J = A.job[blockIdx.y];
    if ((int)blockIdx.x >= J.nb) return;
    const sgan_diffaug_rec r = recs[blockIdx.y];
    double acc = 0.0;
    if (r.a != 1.f && J.ncol) {      // a == 1: the second launch does not read the slots' values
        const f32x4* src = (const f32x4*)J.src;
        for (int g = blockIdx.x * 256 + threadIdx.x; g < J.groups; g += J.nb * 256) {
            const int p = g / J.G, cg = g - p * J.G;
            const uint32_t bits = (J.mask >> (4 * cg)) & 15u;
            if (!bits) continue;
            if (BWD) {
                const int h = p / J.W, w = p - h * J.W;
                if (!sg_da_visible(r, h, w, J.H, J.W)) continue;
            }
            const f32x4 v = src[g];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((bits >> k) & 1u) acc += (double)v[k];
        }
    }
    const double s = sg_block_sum<4>(acc, red);
    if (threadIdx.x == 0) slots[blockIdx.y * SG_DA_SLOTS + blockIdx.x] = s;
}

// ---- the transform.  CONTRAST: the workgroup first sums its job's slots (lane t takes slot t, then sg_block_sum: a fixed order).
template <bool BWD, bool CONTRAST>
__global__ __launch_bounds__(256) void sg_diffaug_apply_kernel(SgDaArgs A, const sgan_diffaug_rec* recs, const double* slots) {
    __shared__ double red[4];
    const SgDaJob J = A.job[blockIdx.y];
    if ((int)blockIdx.x * 256 >= J.groups) return;
    sgan_diffaug_rec r = recs[blockIdx.y];
    float m = 0.f;      // forward: the mean; backward: (1 - a) S / n
    if (CONTRAST) {
        if (r.a != 1.f && J.ncol) {
            const double part = (int)threadIdx.x < J.nb ? slots[blockIdx.y * SG_DA_SLOTS + threadIdx.x] : 0.0;
            const double S = sg_block_sum<4>(part, red);
            const double n = (double)J.ncol * (double)J.H * (double)J.W;
            m = BWD ? (float)((1.0 - (double)r.a) * S / n) : (float)(S / n);
        }
    } else {
        r.a = 1.f;
    }
    const bool scale = r.a != 1.f, shift = !BWD && r.b != 0.f;
    const f32x4* src = (const f32x4*)J.src;
    f32x4* dst = (f32x4*)J.dst;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < J.groups; g += gridDim.x * 256) {
        const int p = g / J.G, cg = g - p * J.G;
        const int h = p / J.W, w = p - h * J.W;
        // forward: output pixel (h, w) shows source (h + ty, w + tx); backward: source pixel (h, w) was shown at output (h - ty, w - tx)
        const int qh = BWD ? h - r.ty : h, qw = BWD ? w - r.tx : w;
        const bool vis = qh >= 0 && qh < J.H && qw >= 0 && qw < J.W && sg_da_visible(r, qh, qw, J.H, J.W);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vis) {
            const int sp = BWD ? qh * J.W + qw : (h + r.ty) * J.W + (w + r.tx);
            v = src[(int64_t)sp * J.G + cg];
        }
        const uint32_t bits = (J.mask >> (4 * cg)) & 15u;
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = v[k];
            if (4 * cg + k >= J.C) {
                t = 0.f;      // padding channels: zeros whatever the source holds there
            } else if ((bits >> k) & 1u) {
                if (BWD) {
                    if (scale) t = fmaf(r.a, t, m);      // a pixel nobody saw still takes the mean's share
                } else if (vis) {
                    if (scale) t = fmaf(r.a, t - m, m);
                    if (shift) t = t + r.b;
                }
            }
            y[k] = t;
        }
        dst[g] = y;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t sgan_diffaug_workspace(int32_t njobs) {
    if (njobs < 1 || njobs > SGAN_DIFFAUG_MAX_JOBS) return -1;
    return (int64_t)njobs * SG_DA_SLOTS * (int64_t)sizeof(double);
}

extern "C" int sgan_diffaug_draw(sgan_diffaug_rec* params_dev, const int32_t* shapes, int32_t njobs, int32_t policy_bits, double rt, double rc,
                                 uint64_t seed, uint64_t* offset_dev, int32_t advance, void* stream) {
    SG_DA_REFUSE(params_dev && shapes, "sgan_diffaug_draw: null pointer");
    SG_DA_REFUSE(njobs >= 1 && njobs <= SGAN_DIFFAUG_MAX_JOBS, "sgan_diffaug_draw: njobs %d outside 1..%d", njobs, SGAN_DIFFAUG_MAX_JOBS);
    SG_DA_REFUSE(policy_bits >= 0 && policy_bits < 16, "sgan_diffaug_draw: unknown policy bits %d", policy_bits);
    SG_DA_REFUSE(rt >= 0.0 && rt <= 1.0 && rc >= 0.0 && rc <= 1.0, "sgan_diffaug_draw: ratios outside [0, 1]");      // a NaN fails both
    SgDaDraw d;
    memset(&d, 0, sizeof d);
    for (int j = 0; j < njobs; ++j) {
        const int H = shapes[2 * j], W = shapes[2 * j + 1];
        SG_DA_REFUSE(H >= 1 && H <= 32768 && W >= 1 && W <= 32768, "sgan_diffaug_draw: job %d shape %dx%d outside 1..32768", j, H, W);
        d.H[j] = H;
        d.W[j] = W;
        d.Sy[j] = (int)floor((double)H * rt + 0.5);
        d.Sx[j] = (int)floor((double)W * rt + 0.5);
        d.ch[j] = (int)floor((double)H * rc + 0.5);
        d.cw[j] = (int)floor((double)W * rc + 0.5);
    }
    hipLaunchKernelGGL(sg_diffaug_draw_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, params_dev, d, njobs, policy_bits, seed, offset_dev,
                       advance);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

static int sg_diffaug_args(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace, SgDaArgs* A,
                           int* max_groups, int* max_nb, const char* who) {
    SG_DA_REFUSE(jobs && params_dev, "%s: null pointer", who);
    SG_DA_REFUSE(njobs >= 1 && njobs <= SGAN_DIFFAUG_MAX_JOBS, "%s: njobs %d outside 1..%d", who, njobs, SGAN_DIFFAUG_MAX_JOBS);
    SG_DA_REFUSE(((uintptr_t)workspace & 7) == 0, "%s: workspace not 8-byte aligned", who);
    memset(A, 0, sizeof *A);
    *max_groups = *max_nb = 0;
    for (int j = 0; j < njobs; ++j) {
        const sgan_diffaug_job& s = jobs[j];
        SG_DA_REFUSE(s.src && s.dst && s.src != s.dst, "%s: job %d needs two different non-null tensors", who, j);
        SG_DA_REFUSE((((uintptr_t)s.src | (uintptr_t)s.dst) & 15) == 0, "%s: job %d tensors must be 16-byte aligned", who, j);
        SG_DA_REFUSE(s.H >= 1 && s.H <= 32768 && s.W >= 1 && s.W <= 32768, "%s: job %d shape %dx%d outside 1..32768", who, j, s.H, s.W);
        SG_DA_REFUSE(s.Cs >= 4 && s.Cs <= 32 && s.Cs % 4 == 0, "%s: job %d stored channels %d: a multiple of 4 in 4..32", who, j, s.Cs);
        SG_DA_REFUSE(s.C >= 1 && s.C <= s.Cs, "%s: job %d channels %d outside 1..%d", who, j, s.C, s.Cs);
        SG_DA_REFUSE(s.C == 32 || (s.colour_mask >> s.C) == 0, "%s: job %d colour mask 0x%x names a channel >= %d", who, j, s.colour_mask, s.C);
        SG_DA_REFUSE((int64_t)s.H * s.W * s.Cs < ((int64_t)1 << 31), "%s: job %d has 2^31 elements or more", who, j);
        SgDaJob& J = A->job[j];
        J.src = s.src; J.dst = s.dst; J.H = s.H; J.W = s.W; J.C = s.C; J.G = s.Cs / 4;
        J.mask = s.colour_mask;
        J.ncol = __builtin_popcount(s.colour_mask);
        J.groups = s.H * s.W * J.G;
        J.nb = sg_cdiv(J.groups, SG_DA_CHUNK);
        if (J.nb > SG_DA_SLOTS) J.nb = SG_DA_SLOTS;
        if (J.groups > *max_groups) *max_groups = J.groups;
        if (J.nb > *max_nb) *max_nb = J.nb;
    }
    return SGAN_OK;
}

template <bool BWD>
static int sg_diffaug_launch(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace, void* stream,
                             const char* who) {
    SgDaArgs A;
    int max_groups, max_nb;
    const int rc = sg_diffaug_args(jobs, njobs, params_dev, workspace, &A, &max_groups, &max_nb, who);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    int bx = sg_cdiv(max_groups, 256);
    if (bx > SG_DA_MAX_BLOCKS) bx = SG_DA_MAX_BLOCKS;
    if (workspace) {
        hipLaunchKernelGGL(sg_diffaug_sum_kernel<BWD>, dim3(max_nb, njobs), dim3(256), 0, st, A, params_dev, (double*)workspace);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL((sg_diffaug_apply_kernel<BWD, true>), dim3(bx, njobs), dim3(256), 0, st, A, params_dev, (const double*)workspace);
    } else {
        hipLaunchKernelGGL((sg_diffaug_apply_kernel<BWD, false>), dim3(bx, njobs), dim3(256), 0, st, A, params_dev, (const double*)nullptr);
    }
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_diffaug_multi_fwd(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace,
                                      void* stream) {
    return sg_diffaug_launch<false>(jobs, njobs, params_dev, workspace, stream, "sgan_diffaug_multi_fwd");
}

extern "C" int sgan_diffaug_multi_bwd(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace,
                                      void* stream) {
    return sg_diffaug_launch<true>(jobs, njobs, params_dev, workspace, stream, "sgan_diffaug_multi_bwd");
}
