/*
 * sgan_hip.h -- C ABI of libsgan_hip.so: hand-written CDNA4 (gfx950) kernels for the conv
 * generator / discriminator training hot path of phymhan/supervised-gan.
 *
 * The reference has no FFI: its hot path is the stock torch.nn modules built in
 * models/networks.py.  Each entry point below replaces the ATen operator family that one of
 * those modules resolves to; the citation names the reference line that instantiates it.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - tensors are NHWC, batch 1, fp32; the channel count `C` passed here is the STORED count,
 *     a multiple of 4 (logical channels are zero-padded up: 1,2,3 -> 4); `*_ld` is the element
 *     stride between pixels (>= C: lets a tensor be a channel slice of a wider concat buffer);
 *   - conv weights ("master layout") are [kh*kw][Cout][Cin] with Cout,Cin the STORED counts, for
 *     Conv2d and ConvTranspose2d alike (the Python side exposes them to state_dict() as strided
 *     views with the reference's logical shapes [Cout,Cin,kh,kw] / [Cin,Cout,kh,kw]);
 *   - per-channel statistics are double[2*C]: sum then sum-of-squares, accumulated with atomics
 *     into a buffer the caller zeroed;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - no entry point allocates, frees or synchronises: safe inside hipGraph capture;
 *   - return value: 0 = ok, <0 = error (see sgan_last_error()); nothing throws across the ABI.
 */
#ifndef SGAN_HIP_H
#define SGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGAN_OK 0
#define SGAN_ERR_INVALID (-1)
#define SGAN_ERR_UNSUPPORTED (-2)
#define SGAN_ERR_HIP (-3)

/* activation codes */
#define SGAN_ACT_NONE 0
#define SGAN_ACT_RELU 1
#define SGAN_ACT_LRELU 2
#define SGAN_ACT_TANH 3

/* conv kinds */
#define SGAN_CONV 0  /* nn.Conv2d            */
#define SGAN_CONVT 1 /* nn.ConvTranspose2d   */

/* Per-channel normalisation + activation applied to a tensor as it is READ by a kernel
 * ("normalise-on-load").  y = act( gamma * (x - mean) * rstd + beta ), mean/rstd derived in-kernel
 * from `stats` (biased variance, eps inside the sqrt).  stats == NULL: no normalisation, only act.
 * Replaces nn.InstanceNorm2d(affine=False) (models/networks.py:46-47), nn.BatchNorm2d in train
 * mode with batch 1 (models/networks.py:87,507,517), nn.ReLU / nn.LeakyReLU(0.2)
 * (models/networks.py:508,525,816,826,833). */
typedef struct sgan_norm_desc {
    const double* stats; /* [2*C] sum, sumsq of the tensor being read, or NULL */
    const float* gamma;  /* [C] or NULL (=1) */
    const float* beta;   /* [C] or NULL (=0) */
    int32_t count;       /* H*W of the tensor being read (statistics population) */
    float eps;
    int32_t act;         /* SGAN_ACT_NONE / RELU / LRELU */
    float slope;         /* LeakyReLU slope */
    int32_t sq_stride;   /* distance (in doubles) from sum[c] to sumsq[c]; 0 = C.  Lets `stats` point into the
                          * statistics of a wider concat buffer (U-Net skip: [up half | skip half]) */
    int32_t rep_stride;  /* 0: one copy of the statistics.  > 0: SGAN_STAT_REPLICAS copies, `rep_stride` doubles apart, whose SUM
                          * is the statistic: the producers spread their same-address fp64 atomics over the copies (workgroup b adds
                          * to copy b % SGAN_STAT_REPLICAS), every reader adds the copies up.  All copies start at zero. */
    const float* mean_rstd; /* [2*C] interleaved (mean_c, rstd_c), or NULL.  The finalised form of `stats` (sgan_norm_finalise_job): a kernel
                          * that finds it loads the pair of its channel instead of deriving it from the fp64 sums -- the same floats, bit for
                          * bit.  `stats` must still be given (it says that the tensor is normalised); sq_stride / rep_stride are not
                          * looked at by a reader of the table.  Only for statistics that are final: the backward pass of a training step */
} sgan_norm_desc;
#define SGAN_STAT_REPLICAS 8

/* Geometry of one Conv2d / ConvTranspose2d layer (square kernel, symmetric stride/pad). */
typedef struct sgan_conv_desc {
    int32_t kind;   /* SGAN_CONV or SGAN_CONVT */
    int32_t k, stride, pad;
    int32_t Hin, Win, Cin;    /* forward input  (stored channels) */
    int32_t Hout, Wout, Cout; /* forward output (stored channels) */
    /* Optional hint, 0 = unknown: how many of the stored channels carry data (the rest is the zero padding to a
     * multiple of 4 -- a 1-channel logits map or a 2-channel image is stored with 4).  Kernels may skip arithmetic on
     * channels beyond these counts: the padding channels of a result are then written as if their weights were zero
     * (which they are in every buffer the host mirror builds). */
    int32_t Cin_logical, Cout_logical;
    /* Arithmetic of the MFMA kernels (the dtype enum of the boundary).  Storage is fp32 in every mode.
     *   SGAN_MATH_F32    : v_mfma_f32_16x16x4_f32, bit-for-bit an fp32 fma chain (the parity mode);
     *   SGAN_MATH_BF16X3 : split 16-bit planes -- every fp32 operand x is cut into hi = rne16(x), lo = rne16(x - hi) and a
     *                      product is a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_{f16,bf16} with fp32 accumulation,
     *                      at 16/3 of the fp32 matrix rate.  The forward pass uses fp16 planes (11 + 11 bits; the packed
     *                      weights hold w * 2^10): measured 2e-7 .. 1e-6 per layer against fp64, the same as SGAN_MATH_F32.
     *                      Backward-data and backward-weight use bf16 planes (8 + 8 bits, the fp32 exponent range of
     *                      gradients): ~5e-6 per layer, inside the 1e-3 contract.  Needs the job's `w_packed` copy of the
     *                      weights (sgan_pack_weights) and fails without it; layers the split kernels do not cover (stored
     *                      channels not a multiple of 8 or under 16, maps under 256 pixels, 4-channel heads) run the fp32
     *                      kernels whatever this field says.
     *   SGAN_MATH_BF16X1 : one 16-bit plane, the speed mode (what torch.autocast trades): a product is hi(a) * hi(b) alone, one
     *                      MFMA instead of three, on the planes SGAN_MATH_BF16X3 uses -- forward fp16 of the activation x fp16 of
     *                      w * 2^10 (the hi half of `w_packed`); backward-data and backward-weight bf16, or fp16 of dout * 2^s where
     *                      `dout_amax` is given.  Storage, accumulation, statistics and everything outside the conv products stay
     *                      fp32.  ~2^-9 (bf16) / 2^-12 (fp16) relative per operand.  Covers exactly the layers SGAN_MATH_BF16X3
     *                      covers (same packed copies, same fallbacks to the exact-fp32 kernels).
     *   Operand domain of the two 16-bit modes, as the MAXIMUM MAGNITUDE of an operand (from a CPU model of this arithmetic on a
     *   32 -> 64 k4 layer, tests/plane_model.py; the kernels follow that model at every scale below to within fp32 accumulation,
     *   tests/test_hip_plane_range.py; each low edge is one power of two inside the last one that passes):
     *     activation as it leaves the normalise / activate-on-load prologue (fp16 planes, UNSCALED: forward, and backward-weight
     *       with `dout_amax`): 1e-3 contract for max|a| in [2^-11, 65504], fp32-equivalent for [2^-2, 65504]; any |a| > 65504
     *       (65520 and up) makes the result non-finite.  Post-normalisation values are of order 1; a layer that loads with an
     *       activation but no norm (the second PatchGAN conv) is inside only while its input is.
     *     weights (fp16 planes of w * 2^10: forward, and backward-data with `dout_amax`): 1e-3 for max|w| in [2^-22, 2^5],
     *       fp32-equivalent for [2^-12, 2^5]; |w| >= 64 makes the result non-finite.
     *     gradients: with `dout_amax` (fp16 planes of dout * 2^s, |s| <= 100) 1e-3 for max|dout| in [2^-112, 2^115],
     *       fp32-equivalent for [2^-102, 2^115]; without it (bf16 planes) ~5e-6 over the same range.
     *   Under a low edge accuracy falls off by 2x per power of two (the lo plane, then the hi plane, go subnormal); nothing is
     *   rerouted.  The 1e-3 contract covers SGAN_MATH_BF16X3 on either kind of plane and SGAN_MATH_BF16X1 on fp16 planes (~3e-4);
     *   SGAN_MATH_BF16X1 on bf16 planes is ~2.5e-3 of the result at every scale. */
    int32_t math;
} sgan_conv_desc;
#define SGAN_MATH_F32 0
#define SGAN_MATH_BF16X3 1
#define SGAN_MATH_BF16X1 2

const char* sgan_version(void);
const char* sgan_last_error(void);
/* name of the kernel template instantiation the calling thread's last sgan_conv_* call launched
 * (matches the name rocprofv3 reports) -- lets a benchmark attribute time and flops per kernel */
const char* sgan_last_kernel(void);
/* what that name leaves out, for the kernels of the layers with a 4-stored-channel side and the exact-fp32 MFMA kernels; other launches leave it as it was, so read
 * it right after the call it belongs to: "NB2 RB4 EPI gy1" (sg_conv_c4_kernel), "NR2 BKC1" (sg_conv_small_n_kernel),
 * "nsplit 3,1" per problem (sg_wgrad_thin_kernel), "DK0 RB4 nsplit 1" (sg_bwd_thin_pair_kernel), "tiles 12" (sg_conv_scatter4_kernel);
 * and for the exact-fp32 MFMA kernels: "ks8 KW2 PRO1" (sg_igemm_kernel: the K split that ran, wave groups per workgroup, prologue;
 * " noslab" appended when a planned split found no workspace and ran unsplit), "PRO0 per4 nsplit 13,4,1" (sg_wgrad_kernel: prologue,
 * 32-pixel chunks per workgroup the split aims at, pixel split per problem);
 * and for the split 16-bit-plane kernels (F16: 1 = fp16 planes, 0 = bf16 planes): "ks8 PRO1 F161" (sg_igemm3_kernel; " noslab" as
 * above), "AIT2 KW2 PRO0 F161" (sg_igemm3p_kernel: patch form 2 / 4 / 6 = up to 128 / up to 256 patch pixels / stride-2 parity planes,
 * wave groups per workgroup), "PRO0 F160 per4 nsplit 13,4,2" (sg_wgrad3_kernel), "DV3 WV1 ks4 F160 WPRO1 nsplit 2,3"
 * (sg_bwd_fused_kernel: backward-data body 1 / 2 / 3 / 5 / 6 and backward-weight body 1 / 2 as in sgan_fused.hip, the K split of the
 * backward-data half, the planes it was actually formed from -- a published maximum on a body other than 6 runs on bf16 planes and
 * reads F160 --, the backward-weight prologue, its pixel split per problem) */
const char* sgan_last_variant(void);
int sgan_stat_replicas(void);     /* SGAN_STAT_REPLICAS of the built library: statistics arenas must hold this many copies */
/* The explicit device of the boundary (SURVEY 8b "Threading": backward is called from autograd worker threads that did not
 * choose a device).  Launches go to the device their stream belongs to and HIP wants the calling thread's current device to be
 * that one: a host thread that has not set it calls sgan_set_device(sgan_stream_device(stream)) once before its first entry
 * point.  (torch's autograd engine does this for its own workers; the Python binding therefore never calls these.) */
int sgan_set_device(int32_t device_id);
int sgan_stream_device(void* stream, int32_t* device_id);

/* ---- optional per-launch timing (diagnostics; single-threaded; do not enable during graph capture) ----
 * While enabled, every main conv kernel launch (implicit-GEMM / small-N / backward-weight; not the split-K
 * epilogue) is bracketed by two HIP events recorded on the launch stream from inside the library.  After a
 * device synchronise, record i (0 <= i < sgan_profile_count(), launch order) yields the kernel's name as
 * rocprofv3 reports it and its duration.  sgan_profile_enable() also clears the records. */
int sgan_profile_enable(int on);
int sgan_profile_count(void);
int sgan_profile_mark(void* stream); /* records an empty bracket named "null": the events' own cost, to subtract */
int sgan_profile_read(int i, const char** name, float* ms);

/* ---- Conv2d / ConvTranspose2d: forward ------------------------------------------------------
 * out = conv(act(norm(in)), w) + bias ; optionally out = tanh(out) ; optionally accumulates the
 * per-channel sum / sumsq of the (pre-tanh) result into out_stats.
 * Replaces: nn.ConvTranspose2d k4 s2 p1 (models/networks.py:502,516,523,529),
 *           nn.Conv2d k4 s2 p2 / k4 s1 p2 (models/networks.py:815,824,831,835),
 *           nn.Conv2d k4 s2 p1 (models/networks.py:356,385), nn.Conv2d k3 s1 p1 (:686,752,774),
 *           nn.Tanh (models/networks.py:540).
 *
 * Workspace (forward and backward-data): deep reductions on small grids are split over K; the fp32
 * partial tiles live in a caller-owned scratch buffer.  Call with workspace_bytes == -1 (nothing is
 * launched) to get the recommended size in KiB as the return value (0 = none); passing NULL / a smaller
 * buffer is allowed and simply disables the split. */
int sgan_conv_fwd(const sgan_conv_desc* d, const float* in, int32_t in_ld, const sgan_norm_desc* in_norm,
                  const float* w, const float* bias, float* out, int32_t out_ld, int32_t out_act,
                  double* out_stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- backward-data ---------------------------------------------------------------------------
 * din = conv_bwd_data(dout, w), then multiplied by act'(norm(x)) of the forward tensor `x` at the
 * same positions (x_norm describes how the forward consumer read x; x == NULL: plain dgrad).
 * With x_norm->stats != NULL it also accumulates the two InstanceNorm/BatchNorm backward sums
 * bwd_sums[0..C) = sum(dY), bwd_sums[C..2C) = sum(dY * xhat) (caller-zeroed).  The result is dY
 * (gradient w.r.t. the normalised-affine value); sgan_norm_bwd_apply() turns it into dX.
 * Replaces: convolution_backward (input grad) + LeakyReLU/ReLU backward of the autograd graph
 * built by FCGANModel.backward_D / backward_G (models/fcgan_model.py:146-176). */
int sgan_conv_dgrad(const sgan_conv_desc* d, const float* dout, int32_t dout_ld, const float* w,
                    float* din, int32_t din_ld, const float* x, int32_t x_ld, const sgan_norm_desc* x_norm,
                    double* bwd_sums, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- grouped launches -----------------------------------------------------------------------------
 * Up to 8 independent problems of the SAME layer type (kind, k, stride, pad, stored channels) in ONE kernel
 * launch, each with its own tensors, weights and spatial size -- the matching layer of the three
 * multi-scale discriminators on the fake and on the real batch (models/fcgan_model.py:150-159) is one
 * launch instead of six.  Semantics per job are exactly those of the single-problem entry points (which
 * are the n == 1 case).  All jobs must agree on the activation codes of their norm descriptors. */
typedef struct sgan_conv_fwd_job {
    const sgan_conv_desc* d;
    const float* in; int32_t in_ld; const sgan_norm_desc* in_norm;
    const float* w; const float* bias;
    float* out; int32_t out_ld;
    double* out_stats;
    int32_t out_stats_sq_stride;  /* distance from sum[n] to sumsq[n] in out_stats; 0 = Cout */
    const void* w_packed;         /* SGAN_MATH_BF16X3 / _BF16X1: the `packed_fwd` copy of `w` (sgan_pack_weights), same element offset; else NULL */
    int32_t out_stats_rep_stride; /* > 0: out_stats is the first of SGAN_STAT_REPLICAS copies this far apart (sgan_norm_desc.rep_stride) */
} sgan_conv_fwd_job;
typedef struct sgan_conv_dgrad_job {
    const sgan_conv_desc* d;
    const float* dout; int32_t dout_ld;
    const float* w;
    float* din; int32_t din_ld;
    const float* x; int32_t x_ld; const sgan_norm_desc* x_norm;
    double* bwd_sums;
    int32_t bwd_sums_sq_stride;   /* distance from s1[n] to s2[n] in bwd_sums; 0 = Cin */
    int32_t accumulate;           /* 1: din += result (a tensor with two forward consumers, e.g. a U-Net skip) */
    int32_t w_transposed;         /* 1: `w` is the transposed master copy [kh*kw][Cin_s][Cout_s] (sgan_transpose_weights): the
                                   * reduction channel (Cout) is then contiguous and backward-data stages its weights with
                                   * 16-byte LDS stores like the forward pass */
    const void* w_packed;         /* SGAN_MATH_BF16X3 / _BF16X1: the `packed_bwd` copy of the weights (sgan_pack_weights); else NULL */
    int32_t bwd_sums_rep_stride;  /* > 0: bwd_sums is the first of SGAN_STAT_REPLICAS copies this far apart */
    const float* dout_amax;       /* device scalar max|dout| (sgan_norm_bwd_apply_multi publishes it) or NULL.  With it (and w_packed_f16)
                                   * SGAN_MATH_BF16X3 runs backward-data on fp16 planes of dout * 2^s, s from the exponent of the maximum:
                                   * 11 + 11 significant bits, an fp32-equivalent product like the forward pass.  Without: bf16 planes (8 + 8) */
    const void* w_packed_f16;     /* the `packed_bwd_f16` copy of the weights (sgan_pack_weights); NULL: bf16 planes */
} sgan_conv_dgrad_job;
typedef struct sgan_conv_wgrad_job {
    const sgan_conv_desc* d;
    const float* in; int32_t in_ld; const sgan_norm_desc* in_norm;
    const float* dout; int32_t dout_ld;
    float* dw; float* dbias;
    const float* dout_amax;       /* as sgan_conv_dgrad_job.dout_amax: with it backward-weight runs on fp16 planes (dout scaled), else bf16 */
} sgan_conv_wgrad_job;
int sgan_conv_fwd_grouped(const sgan_conv_fwd_job* jobs, int32_t n, int32_t out_act, void* workspace,
                          int64_t workspace_bytes, void* stream);
int sgan_conv_dgrad_grouped(const sgan_conv_dgrad_job* jobs, int32_t n, void* workspace, int64_t workspace_bytes,
                            void* stream);
int sgan_conv_wgrad_grouped(const sgan_conv_wgrad_job* jobs, int32_t n, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* One launch for a layer's backward-data AND backward-weight (split-bf16 mode): the two halves of aten::convolution_backward
 * the reference's autograd runs for every conv in netD / netG backward (models/networks.py:502-529, 815-835 are the layers;
 * models/fcgan_model.py:131-152 the backward calls).  Same jobs as the two grouped entry points above, same results; the
 * workgroups of both share one grid so the chip is not left half idle twice.  Returns SGAN_OK when launched, 1 when this layer
 * is not covered by the fused kernel (the caller then issues the two grouped calls; nothing was written), < 0 on error.
 * dgrad_math: SGAN_MATH_* of the backward-data half, or -1 for the descriptors' own (the two job lists usually point at the
 * same descriptors, and backward-data into a layer without a normalisation runs exact fp32 next to a split-bf16
 * backward-weight: DESIGN.md R2.3); the backward-weight half must be SGAN_MATH_BF16X3 or SGAN_MATH_BF16X1.  A SGAN_MATH_BF16X1
 * backward-weight half fuses with a SGAN_MATH_BF16X1 or SGAN_MATH_BF16X3 backward-data half; a SGAN_MATH_BF16X1 backward-data half
 * beside a SGAN_MATH_BF16X3 backward-weight half answers 1. */
int sgan_conv_bwd_fused(const sgan_conv_dgrad_job* djobs, int32_t nd, const sgan_conv_wgrad_job* wjobs, int32_t nw,
                        int32_t dgrad_math, void* stream);
/* The same with a workspace: a pair whose backward-data half is a deep reduction on a small map (generator 256 -> 128 at 32 x 32, the
 * inner U-Net levels) keeps its split-K inside the fused launch -- the partial tiles go to `workspace`, a second kernel sums them and
 * runs the backward-data epilogue.  workspace_bytes == -1: query, returns the KiB the pair wants (0: none) and launches nothing.
 * Without enough workspace such a pair answers 1 (the caller issues the two grouped calls), as sgan_conv_bwd_fused does. */
int sgan_conv_bwd_fused_ws(const sgan_conv_dgrad_job* djobs, int32_t nd, const sgan_conv_wgrad_job* wjobs, int32_t nw,
                           int32_t dgrad_math, void* workspace, int64_t workspace_bytes, void* stream);

/* A layer with a 4-channel side (the generator's output ConvTranspose2d(ngf, 2), models/networks.py:528-533; the first PatchGAN conv
 * Conv2d(2, ndf) in a generator update, :815-817): its backward-data and backward-weight launches in ONE grid
 * (sg_bwd_thin_pair_kernel).  Same job lists as sgan_conv_dgrad_grouped / sgan_conv_wgrad_grouped, same results.  Returns 1 when the
 * pair is not one of the two shapes (the caller issues the two grouped calls). */
int sgan_conv_bwd_thin_pair(const sgan_conv_dgrad_job* djobs, int32_t nd, const sgan_conv_wgrad_job* wjobs, int32_t nw, void* stream);

/* ---- class-weighted cross-entropy on logits, softmax over channels (NHWC maps, <= 16 classes) ---------------------------
 * sgan_ce_fwd:  loss = sum_p w[y_p] (logsumexp(z_p) - z_p[y_p]) / sum_p w[y_p];  y_p = label[p] (int64 map) or const_label when label
 *               is NULL; class_w NULL = unit weights; labels outside [0, C) are skipped (torch's ignore_index).  `acc` (2 doubles) and
 *               `ticket` (1 uint32) are caller-owned scratch that must be ZERO on entry; acc keeps the two sums for sgan_ce_bwd.
 * sgan_ce_bwd:  dlogits = gout[0] * w[y_p] * (softmax(z_p) - onehot(y_p)) / sum w   (padding channels of dlogits: zeros).
 * Replaces: nn.CrossEntropyLoss in GANLossMultiClass (models/networks.py:188-202), CrossEntropyLoss2d = NLLLoss2d(log_softmax)
 * (models/loss.py:6-12) of the segmentation trainers.
 * sgan_softmax_fwd / _bwd: p = softmax over the C logical channels; dz = p * (dp - sum_c dp_c p_c).  Replaces F.softmax(logit, 1)
 * (models/segm_model.py:155-160). */
int sgan_ce_fwd(const float* logits, int32_t ld, int32_t npix, int32_t C, const int64_t* label, int32_t const_label,
                const float* class_w, double* acc, uint32_t* ticket, float* loss_out, void* stream);
int sgan_ce_bwd(const float* logits, int32_t ld, int32_t npix, int32_t C, const int64_t* label, int32_t const_label,
                const float* class_w, const double* acc, const float* gout, float* dlogits, int32_t dld, void* stream);
int sgan_softmax_fwd(const float* z, int32_t ld, int32_t npix, int32_t C, float* p, int32_t pld, void* stream);
int sgan_softmax_bwd(const float* dp, int32_t dpld, const float* p, int32_t pld, int32_t npix, int32_t C, float* dz, int32_t dzld,
                     void* stream);

/* ---- sigmoid over channels and weighted BCE (`--use_sigmoid_ss`, models/segm_model.py:155-160,216-236; <= 16 channels) --------
 * sgan_sigmoid_nhwc_fwd / _bwd: p = sigmoid(z) over the C logical channels (padding channels of p: zeros); dz = dp * p (1 - p).
 * sgan_bce_weighted_fwd: loss = mean over pixels and channels of w(pix) * BCE(p_c, t_c) (torch's log clamp at -100), with
 *               w = 1 + sum_{i < nw} t_i * (class_w[i] - 1); nw = 0: unweighted.  `workspace`: SGAN_BCE_WEIGHTED_WS_BYTES of 8-byte
 *               aligned device scratch, ZERO on first use; the ticket at its end is left at zero (no fill per call).
 * sgan_bce_weighted_bwd: dp = gout[0] * w * (p - t) / max(p (1 - p), 1e-12) / (C * npix)   (padding channels of dp: zeros).
 * Replaces torch.sigmoid, the narrow / mul / add loop that builds the weight map, and F.binary_cross_entropy(weight=). */
#define SGAN_BCE_WEIGHTED_WS_BYTES 1024
int sgan_sigmoid_nhwc_fwd(const float* z, int32_t ld, int32_t npix, int32_t C, float* p, int32_t pld, void* stream);
int sgan_sigmoid_nhwc_bwd(const float* dp, int32_t dpld, const float* p, int32_t pld, int32_t npix, int32_t C, float* dz, int32_t dzld,
                          void* stream);
int sgan_bce_weighted_fwd(const float* p, int32_t pld, const float* t, int32_t tld, int32_t npix, int32_t C, const float* class_w,
                          int32_t nw, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
int sgan_bce_weighted_bwd(const float* p, int32_t pld, const float* t, int32_t tld, int32_t npix, int32_t C, const float* class_w,
                          int32_t nw, const float* gout, float* dp, int32_t dpld, void* stream);

/* ---- the loss section of a segmentation step with no discriminator (`--which_model_netD None`, models/segm_model.py:203-228) ----
 * sgan_seg_head: ONE pass over the [npix][ld] logits (C <= 16 logical channels) writes the prediction p, the loss and, unless
 *               `dlogits` is NULL, d loss / d logits for an upstream gradient of 1 (padding channels of p and dlogits: zeros).
 *   SGAN_SEGHEAD_SOFTMAX: `label_or_target` is the int64 label map; p = softmax(z);
 *               loss = sum_p w[y_p] (logsumexp(z_p) - z_p[y_p]) / norm[0];  dlogits = w[y_p] (p - onehot(y_p)) / norm[0]
 *               (sgan_softmax_fwd + sgan_ce_fwd + sgan_ce_bwd with gout = 1).  class_w NULL = unit weights, else nw >= C of them;
 *               labels outside [0, C) contribute nothing.  `norm`: device float, sum_p w[y_p] (sgan_label_weight_sum); 0 -> loss 0.
 *   SGAN_SEGHEAD_SIGMOID: `label_or_target` is the float target map [npix][tld]; p = sigmoid(z);  w = 1 + sum_{i < nw} t_i (class_w[i] - 1);
 *               loss = mean over pixels and channels of w * BCE(p, t) (torch's log clamp at -100);
 *               dlogits = w (p - t) / max(p (1 - p), 1e-12) * p (1 - p) / (C * npix)
 *               (sgan_sigmoid_nhwc_fwd + sgan_bce_weighted_fwd + sgan_bce_weighted_bwd + sgan_sigmoid_nhwc_bwd with gout = 1); `norm` unused.
 *   Valid only while the loss is the one consumer of p: a gradient that arrives at p from elsewhere is not in dlogits.
 * sgan_label_weight_sum: out[0] = sum_p class_w[label_p] (fp64 accumulation) over the labels in [0, C); class_w NULL: their count.
 * `workspace` (both): SGAN_SEGHEAD_WS_BYTES of 8-byte aligned device scratch, ZERO on first use, owned by one stream at a time and
 * left zeroed by every call (no fill per call).  The sums are taken in a fixed order: equal inputs give equal bits.
 * Both return 1 (not covered, nothing launched) for C > 16 or a NULL required pointer.
 * sgan_seg_head_pw / sgan_pixel_weight_sum: the same two with a per-pixel term in the weight (the border term of the U-Net loss,
 *   sgan_border_weight): w_p = (class_w ? class_w[y_p] : 1) + pixel_add[p] (one fp32 add) for labels in [0, C), `pixel_add` a dense
 *   float [npix] map; any other label contributes nothing to either.  sgan_pixel_weight_sum: out[0] = sum_p w_p.  sgan_seg_head_pw,
 *   softmax only: loss = sum_p w_p (logsumexp(z_p) - z_p[y_p]) / norm[0];  dlogits = w_p (p - onehot(y_p)) / norm[0];  norm 0 -> loss 0.
 *   Workspace, fixed summation order, padding channels and the return of 1 (here also for a NULL pixel_add or norm) as above.  With
 *   pixel_add all zero both give the bits of the entries above. */
#define SGAN_SEGHEAD_WS_BYTES 8192
#define SGAN_SEGHEAD_SOFTMAX 0
#define SGAN_SEGHEAD_SIGMOID 1
int sgan_label_weight_sum(const int64_t* label, int32_t npix, int32_t C, const float* class_w, float* out, void* workspace, void* stream);
int sgan_seg_head(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                  const float* class_w, int32_t nw, const float* norm, float* p_out, int32_t pld, float* dlogits, int32_t dld,
                  float* loss_out, void* workspace, void* stream);
int sgan_pixel_weight_sum(const int64_t* label, int32_t npix, int32_t C, const float* class_w, const float* pixel_add, float* out,
                          void* workspace, void* stream);
int sgan_seg_head_pw(const float* logits, int32_t ld, int32_t npix, int32_t C, const int64_t* label, const float* class_w, int32_t nw,
                     const float* pixel_add, const float* norm, float* p_out, int32_t pld, float* dlogits, int32_t dld, float* loss_out,
                     void* workspace, void* stream);

/* ---- backward pass of a one-channel stride-1 head (the PatchGAN logits conv, models/networks.py:832-835) in one launch: the job
 * lists of sgan_conv_dgrad_grouped and sgan_conv_wgrad_grouped for the SAME pass (wjobs may be NULL: input gradient only).  Returns 1
 * when the layer is not of that type (Conv2d, stride 1, k <= 4, stored Cout 4 / logical 1, Cin >= 64, no `accumulate`): the caller
 * then issues the two generic calls.  Exact fp32. */
int sgan_conv_head_bwd(const sgan_conv_dgrad_job* djobs, const sgan_conv_wgrad_job* wjobs, int32_t n, void* stream);

/* ---- transposed weight copy for backward-data ---------------------------------------------------
 * flat_t[off + tap][ci][co] = flat[off + tap][co][ci] for every conv segment (bias / affine ranges of the flat
 * parameter buffer are not touched).  Run after each optimizer step on the nets whose backward-data is needed. */
typedef struct sgan_wt_seg { int64_t off; int32_t taps, cout, cin; } sgan_wt_seg;
int sgan_transpose_weights(const float* flat, float* flat_t, const sgan_wt_seg* segs, int32_t n /* <= 64 */, void* stream);

/* ---- packed weight copies (the reference keeps one weight tensor per layer, models/networks.py:502-529,815-835; the
 * kernels read it in three derived forms) ------------------------------------------------------------------------
 * For every conv segment of the flat parameter buffer (same element offsets in every copy):
 *   flat_t     [tap][ci][co] fp32                          transposed master copy (as sgan_transpose_weights), or NULL
 *   packed_fwd [tap][co][ci/8]{8 x bf16 hi | 8 x bf16 lo}  split-bf16 rows for the forward pass   (cin  % 8 == 0), or NULL
 *   packed_bwd [tap][ci][co/8]{8 x bf16 hi | 8 x bf16 lo}  split-bf16 rows for backward-data      (cout % 8 == 0), or NULL
 *   packed_bwd_f16: the same rows as fp16 planes of w * 2^10 (like packed_fwd, which holds fp16 planes of w * 2^10 too): what
 *                   backward-data reads when the gradient's maximum is known (sgan_conv_dgrad_job.dout_amax), or NULL
 * hi = bf16(x) (round to nearest even), lo = bf16(x - hi).  A copy occupies 4 bytes per weight like the master.  Segments
 * whose channel count does not divide are left untouched in that copy (such layers run the fp32 kernels).  Run after each
 * optimizer step / checkpoint load, before the next forward. */
int sgan_pack_weights(const float* flat, float* flat_t, void* packed_fwd, void* packed_bwd, void* packed_bwd_f16,
                      const sgan_wt_seg* segs, int32_t n /* <= 64 */, void* stream);

/* ---- backward-weight ---------------------------------------------------------------------------
 * dw += act(norm(in))^T (x) dout over all pixels (master layout), dbias += sum_pixels dout.
 * Accumulates (atomics) into caller-owned gradient buffers.
 * `workspace` (same protocol as sgan_conv_fwd: workspace_bytes == -1 returns the KiB needed) lets the thin-layer
 * kernel (stored Cin == 4 or Cout == 4) combine its pixel splits in two stages instead of with contended atomics;
 * optional -- without it the result is the same, only slower.
 * Replaces: convolution_backward (weight / bias grad). */
int sgan_conv_wgrad(const sgan_conv_desc* d, const float* in, int32_t in_ld, const sgan_norm_desc* in_norm,
                    const float* dout, int32_t dout_ld, float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ---- InstanceNorm / BatchNorm(batch 1) backward, in place ------------------------------------
 * dy[p][c] <- gamma_c * rstd_c * ( dy - s1_c/M - xhat * s2_c/M ), xhat = (x - mean_c) * rstd_c.
 * dgamma += s2, dbeta += s1 when non-NULL.  M = npix.
 * Replaces: native_batch_norm_backward of nn.InstanceNorm2d / nn.BatchNorm2d. */
int sgan_norm_bwd_apply(float* dy, int32_t dy_ld, const float* x, int32_t x_ld, int32_t npix, int32_t C,
                        const sgan_norm_desc* x_norm, const double* bwd_sums, int32_t bwd_sums_sq_stride /* 0 = C */,
                        float* dgamma, float* dbeta, void* stream);

/* Several independent tensors in one launch (the matching layer of grouped discriminator chains). */
typedef struct sgan_norm_bwd_job {
    float* dy; int32_t dy_ld;
    const float* x; int32_t x_ld;
    int32_t npix, C;
    const sgan_norm_desc* x_norm;
    const double* bwd_sums; int32_t bwd_sums_sq_stride;
    float* dgamma; float* dbeta;
    int32_t bwd_sums_rep_stride;   /* > 0: bwd_sums is the first of SGAN_STAT_REPLICAS copies this far apart (summed on read) */
    float* amax_out;               /* NULL, or a device scalar that starts at 0: max|dy| of the result is stored there (an atomic max on the
                                    * bit pattern) -- the `dout_amax` of the backward-data / backward-weight calls that read dy next */
} sgan_norm_bwd_job;
int sgan_norm_bwd_apply_multi(const sgan_norm_bwd_job* jobs, int32_t n /* 1..8 */, void* stream);

/* ---- BatchNorm running statistics (momentum update, unbiased variance), n layers per launch --
 * Replaces the running_mean / running_var side effect of nn.BatchNorm2d.forward in train mode. */
typedef struct sgan_bn_running_desc {
    const double* stats;
    float* running_mean;
    float* running_var;
    int64_t* num_batches_tracked; /* device int64 incremented by one, or NULL */
    int32_t C;
    int32_t count;     /* H*W */
    int32_t sq_stride; /* distance from a channel's sum to its sum of squares inside `stats`; 0 = C (wider when `stats`
                          is a slice of a concatenated tensor's statistics, or C is not a multiple of 4) */
    int32_t rep_stride; /* > 0: `stats` is the first of SGAN_STAT_REPLICAS copies this far apart (summed on read) */
} sgan_bn_running_desc;
int sgan_bn_running_update(const sgan_bn_running_desc* layers, int32_t n, float momentum, void* stream);

/* ---- Gaussian pre-filter + stride pick of the multi-scale discriminators ----------------------
 * out[y][x][c] = sum_{ky,kx} g[c][ky][kx] * in[y*s + ky - pad][x*s + kx - pad][c], where g is read
 * from the diagonal of the reference's dense [C,C,k,k] weight (w_diag_stride = element stride
 * between g[c] and g[c+1]).  Only strided outputs and diagonal channels are computed.
 * Replaces: gauss_filter = Conv2d(C,C,4*sigma+1,pad 2*sigma) + AvgPool2d(1, stride s)
 * (models/networks.py:807-813). */
int sgan_gauss_down_fwd(const float* in, int32_t in_ld, int32_t H, int32_t W, int32_t C, int32_t Creal,
                        const float* g, int32_t g_chan_stride, int32_t k, int32_t pad, int32_t s,
                        float* out, int32_t out_ld, int32_t Ho, int32_t Wo, void* stream);
int sgan_gauss_down_bwd(const float* dout, int32_t dout_ld, int32_t Ho, int32_t Wo, int32_t C, int32_t Creal,
                        const float* g, int32_t g_chan_stride, int32_t k, int32_t pad, int32_t s,
                        float* din, int32_t din_ld, int32_t H, int32_t W, int32_t accumulate /* din += instead of = */,
                        void* stream);

/* Several pre-filters in one launch (the multi-scale discriminators filter one image at scale 2 and at scale 4;
 * models/fcgan_model.py:86-93 builds one NLayerDiscriminator per --scale_factor entry).  Forward: n <= 4 independent jobs.
 * Backward: the jobs must share `image` (the image gradient): it receives the SUM of their contributions
 * (accumulate != 0: added to what it holds). */
typedef struct sgan_gauss_job {
    float* image; int32_t image_ld, H, W;    /* full-resolution side: read by fwd, written by bwd */
    float* down; int32_t down_ld, Ho, Wo;    /* filtered + strided side: written by fwd, read by bwd */
    const float* g; int32_t g_chan_stride, k, pad, s;
} sgan_gauss_job;
int sgan_gauss_down_multi_fwd(const sgan_gauss_job* jobs, int32_t n, int32_t C, int32_t Creal, void* stream);
int sgan_gauss_down_multi_bwd(const sgan_gauss_job* jobs, int32_t n, int32_t C, int32_t Creal, int32_t accumulate, void* stream);

/* ---- GAN loss on a logits map (channel 0 of an NHWC-4 tensor) --------------------------------
 * mode 0: BCE(sigmoid(x), t) with torch's log clamp at -100 (GANLoss, --no_lsgan);
 * mode 1: MSE(x, t) (lsgan, no sigmoid).  loss_out[0] = mean loss; p_out (optional) = sigmoid(x).
 * p_out shares `ld` with the logits: p_out[i * ld] is written, so it is a map of the logits' own pixel stride.
 * The backward writes dlogits[p][0] = gout[0] * dloss/dx, other stored channels 0.
 * Replaces: nn.Sigmoid (models/networks.py:836-837) + nn.BCELoss / nn.MSELoss inside GANLoss
 * (models/networks.py:160-163,183-185). */
int sgan_gan_loss_fwd(const float* logits, int32_t ld, int32_t npix, float target, int32_t mode,
                      float* loss_out, float* p_out, void* stream);
int sgan_gan_loss_bwd(const float* logits, int32_t ld, int32_t npix, float target, int32_t mode,
                      const float* gout, float* dlogits, int32_t dld, void* stream);

/* ---- every GAN-loss term of one backward pass at once ----------------------------------------------
 * total = sum_i weight_i * loss_i over up to 8 logits maps, loss_i as sgan_gan_loss_fwd computes it;
 * each_out[i] = loss_i (for logging).  A forward job with a `dlogits` buffer also gets dlogits_i = weight_i * dloss_i/dx, the
 * gradient for an upstream gradient of 1 (the trainers call backward() on `total` itself); the backward entry point writes
 * dlogits_i = gout * weight_i * dloss_i/dx for any other upstream gradient.
 * Replaces the per-discriminator GANLoss calls plus the scalar arithmetic the trainers wrap around them:
 * (loss_D_fake + loss_D_real) * 0.5 and sum_i lambda_i * loss_i (models/fcgan_model.py:150-176). */
typedef struct sgan_gan_loss_job {
    const float* logits; int32_t ld; int32_t npix;
    float target; float weight;
    float* dlogits; int32_t dld;   /* forward: optional (unit-gradient result); backward: required */
} sgan_gan_loss_job;
/* `workspace`: SGAN_GAN_LOSS_WS_BYTES of 8-byte aligned device scratch, ZERO on first use and owned by one stream at a time: the
 * terms are reduced by several workgroups each, the last one to arrive (a ticket counter at the end of the scratch) finishes
 * and leaves the counter at zero again -- one launch, no fill per call. */
#define SGAN_GAN_LOSS_WS_BYTES 2048
int sgan_gan_loss_multi_fwd(const sgan_gan_loss_job* jobs, int32_t n, int32_t mode, float* each_out, float* total_out,
                            void* workspace, int64_t workspace_bytes, void* stream);
int sgan_gan_loss_multi_bwd(const sgan_gan_loss_job* jobs, int32_t n, int32_t mode, const float* gout, void* stream);

/* ---- finalised normalisation statistics (sgan_norm_desc.mean_rstd) ----------------------------------------------------
 * One job turns the fp64 (sum, sum of squares) of one tensor -- `sq_stride` and `rep_stride` as in sgan_norm_desc -- into
 * mean_rstd[2 c] = mean_c, mean_rstd[2 c + 1] = rstd_c (2*C floats, 8-byte aligned) with the expression every kernel uses on
 * load: entry c holds, bit for bit, what a kernel reading `stats` derives for channel c.
 * sgan_gan_loss_multi_fwd_fin is sgan_gan_loss_multi_fwd with up to SGAN_NORM_FIN_MAX such jobs carried by extra workgroups of
 * the SAME launch: the loss of a pass runs after the last forward launch of the pass and before its first backward launch, the
 * one place where the statistics are final and not yet read again.  The statistics must be complete when the launch starts
 * (stream order).  nfin == 0 is sgan_gan_loss_multi_fwd.
 * sgan_norm_mean_rstd_probe (diagnostics, tests): out[2 c], out[2 c + 1] = what a kernel reading tensor `d` derives for channel c
 * (one workgroup; from `d->mean_rstd` when that is given, else from `d->stats`). */
typedef struct sgan_norm_finalise_job {
    const double* stats; int32_t C; int32_t count; float eps; int32_t sq_stride; int32_t rep_stride;
    float* mean_rstd;
} sgan_norm_finalise_job;
#define SGAN_NORM_FIN_MAX 48
int sgan_gan_loss_multi_fwd_fin(const sgan_gan_loss_job* jobs, int32_t n, int32_t mode, float* each_out, float* total_out,
                                void* workspace, int64_t workspace_bytes, const sgan_norm_finalise_job* fin, int32_t nfin,
                                void* stream);
int sgan_norm_mean_rstd_probe(const sgan_norm_desc* d, int32_t C, float* out, void* stream);

/* ---- every factored-discriminator GAN-loss term of one backward pass at once -----------------------------
 * Term i multiplies two discriminator maps before the criterion (models/twostage_factD_model.py:256-296,352-383, util.mul):
 *   a1 = SIG1 ? sigmoid(l1) : l1  [h1, w1]      a2 = SIG2 ? sigmoid(l2) : l2  [H2, W2]      (channel 0 of NHWC maps)
 *   u  = up == 2 ? bilinear x2 of a1 (align_corners = False, the taps of sgan_bilinear_up2_fwd) : a1          [hu, wu]
 *   q  = u reflection-padded to [H2, W2] with left = floor(dW / 2), right = dW - left, bottom = floor(dH / 2), top = dH - bottom
 *   p  = q * a2;  loss_i = mean(MSE ? (p - target_i)^2 : BCE(p, target_i) with torch's log clamp at -100)
 *   total = sum_i weight_i * loss_i;  each_out[i] = loss_i.
 * A forward job with a `dl1` and / or `dl2` buffer also gets d total / d l1, d total / d l2 for an upstream gradient of 1 (other
 * stored channels 0); the backward entry point writes them for gout[0].  Either buffer may be NULL (a detached side).  The
 * gradients are gathered, without float atomics: the same inputs give the same bits.
 * Returns 1 and writes nothing ("not covered": the caller keeps its own composition) unless n <= 8, up is 1 or 2, hu <= H2,
 * wu <= W2, every pad is smaller than the padded dimension of u (torch's reflect rule), and BCE comes with SIG1 and SIG2 both
 * set (a raw score times a probability can leave [0, 1]).
 * Replaces, per term: two nn.Sigmoid, nn.Upsample, F.pad(reflect), the product, the target fill, nn.BCELoss / nn.MSELoss and
 * the sums and lambda factors around them, forward and backward. */
#define SGAN_FACTD_SIG1 1
#define SGAN_FACTD_SIG2 2
#define SGAN_FACTD_MSE 4
typedef struct sgan_factd_loss_job {
    const float* l1; int32_t ld1; int32_t h1; int32_t w1;
    const float* l2; int32_t ld2; int32_t H2; int32_t W2;
    int32_t up;
    float target; float weight;
    float* dl1; int32_t dld1;      /* optional, forward and backward */
    float* dl2; int32_t dld2;
} sgan_factd_loss_job;
/* `workspace`: SGAN_FACTD_LOSS_WS_BYTES of 8-byte aligned device scratch, ZERO on first use and owned by one stream at a time;
 * the ticket counter at its end is left at zero, as with SGAN_GAN_LOSS_WS_BYTES -- one launch, no fill per call. */
#define SGAN_FACTD_LOSS_WS_BYTES 2048
int sgan_factd_loss_multi_fwd(const sgan_factd_loss_job* jobs, int32_t n, int32_t mode, float* each_out, float* total_out,
                              void* workspace, int64_t workspace_bytes, void* stream);
int sgan_factd_loss_multi_bwd(const sgan_factd_loss_job* jobs, int32_t n, int32_t mode, const float* gout, void* stream);

/* ---- standalone nn.Sigmoid on channel 0 of a logits map (models/networks.py:836-837) --------
 * Only needed when a caller wants the probability map itself; the GAN loss above consumes logits.
 * Every pixel stride (ld, pld, dpld, dxld) is >= 1; the whole pld / dxld floats of a pixel are written (channel 0, then zeros). */
int sgan_sigmoid_fwd(const float* x, int32_t ld, int32_t npix, float* p, int32_t pld, void* stream);
int sgan_sigmoid_bwd(const float* dp, int32_t dpld, const float* p, int32_t pld, int32_t npix, float* dx,
                     int32_t dxld, void* stream);

/* ---- U-Net up path: normalise (+ dropout) (+ additive Gaussian noise) into a concat slice --------------
 * t[p][c] = ((u[p][c] - mean_c) * rstd_c * gamma_c + beta_c) * (mask ? mask[p][c] : 1) + (noise ? sigma * noise[p][c] : 0)
 * (gamma = 1, beta = 0 without an affine: InstanceNorm; with one: norm_layer = BatchNorm2d -> nn.Dropout, networks.py:516-521)
 * mask holds 0 or 1/(1-p) (nn.Dropout(0.5) => 0 or 2).  Replaces norm_layer + nn.Dropout + the `y + noise` of
 * UnetSkipConnectionBlock (models/networks.py:387-403,414-419); `t` is written straight into the up half
 * of the concat buffer the next ConvTranspose2d reads (torch.cat, :417-419, never materialises).
 * Backward, first pass: dt <- dt * mask in place and bwd_sums += (sum dt, sum dt * uhat); then
 * sgan_norm_bwd_apply(dt, u, ...) finishes the normalisation backward. */
int sgan_norm_apply_fwd(const float* u, int32_t u_ld, const sgan_norm_desc* u_norm, const float* mask, const float* noise,
                        float sigma, float* t, int32_t t_ld, int32_t npix, int32_t C, void* stream);
int sgan_norm_apply_bwd_sums(float* dt, int32_t dt_ld, const float* mask, const float* u, int32_t u_ld,
                             const sgan_norm_desc* u_norm, double* bwd_sums, int32_t npix, int32_t C, void* stream);
/* mask[i] = uniform(Philox(seed, *offset_dev + i)) < p ? 0 : 1/(1-p); advances *offset_dev (nn.Dropout). */
int sgan_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, uint64_t* offset_dev, int32_t advance, void* stream);

/* ---- nn.ReflectionPad2d in front of a conv (resnet generators: models/networks.py:232,258 ReflectionPad2d(3) + Conv k7;
 * :282-300 ReflectionPad2d(1) + Conv k3 inside every ResnetBlock) -------------------------------------------------------
 * out [H + 2 pad][W + 2 pad][C] = mask * act(norm(x)) gathered at the reflected positions (what the reference normalises,
 * activates and drops out BEFORE it pads); the conv that follows takes `out` with pad 0 and no in_norm.  pad == 0 just
 * materialises mask * act(norm(x)).  `mask` is dense [H][W][C] (nn.Dropout: 0 or 1 / (1 - p)) or NULL.
 * Backward: din [H][W][C] = act'(norm(x)) * mask * (sum of dout over the <= 4 padded positions that mirror the pixel);
 * with x_norm->stats it also accumulates bwd_sums (sum din, sum din * xhat) for sgan_norm_bwd_apply, like sgan_conv_dgrad.
 * x == NULL: a plain fold (the padded tensor was the input itself). */
int sgan_pad_reflect_fwd(const float* x, int32_t x_ld, int32_t H, int32_t W, int32_t C, const sgan_norm_desc* x_norm,
                         const float* mask, int32_t pad, float* out, int32_t out_ld, void* stream);
int sgan_pad_reflect_bwd(const float* dout, int32_t dout_ld, int32_t H, int32_t W, int32_t C, int32_t pad, const float* x,
                         int32_t x_ld, const sgan_norm_desc* x_norm, const float* mask, float* din, int32_t din_ld,
                         double* bwd_sums, int32_t bwd_sums_sq_stride, void* stream);

/* ---- BCELoss on rescaled tanh outputs (two-stage trainers): loss = mean BCE((x + 1) / 2, (t + 1) / 2) over npix * C
 * with torch's -100 log clamp; g = dloss/dx for a unit upstream gradient (backward: dx = gout * g, sgan_scale).
 * Replaces: torch.nn.BCELoss()((x + 1) / 2, (t + 1) / 2) at models/twostage_cycle_model.py:398-403. */
/* `workspace` (this function and sgan_l1w_fwd): SGAN_IMAGE_LOSS_WS_BYTES of 8-byte aligned device scratch (uninitialised is
 * fine) for the per-workgroup partial sums a second kernel finishes. */
#define SGAN_IMAGE_LOSS_WS_BYTES 2048
int sgan_bce01_fwd(const float* x, int32_t x_ld, const float* t, int32_t t_ld, int32_t npix, int32_t C, float* loss_out,
                   float* g, int32_t g_ld, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- CRN building blocks (models/networks.py:642-794) --------------------------------------------
 * sgan_bilinear_up2_fwd: nn.Upsample(scale_factor=2, mode='bilinear') (align_corners = False) of an [H, W, C] tensor
 * into [2H, 2W, C], accumulating the (sum, sumsq) statistics of the result for the InstanceNorm that follows it
 * (CrnUpsampleBlock :741-746).  sgan_bilinear_up2_bwd is its adjoint (din [H, W, C] from dout [2H, 2W, C]).
 * sgan_avgpool_pyramid_fwd: the six label maps AvgPool2d(2^(s+1)) (label), s = 0..5, of
 * CascadedRefinementNetwork.forward (:709-731) in one launch (4 stored channels; H, W divisible by 64);
 * sgan_avgpool_pyramid_bwd: dlabel (+)= sum_s upsample(dlevels[s]) / 4^(s+1) (NULL levels are skipped). */
int sgan_bilinear_up2_fwd(const float* in, int32_t in_ld, int32_t H, int32_t W, int32_t C, float* out, int32_t out_ld,
                          double* out_stats, int32_t out_stats_sq_stride, void* stream);
int sgan_bilinear_up2_bwd(const float* dout, int32_t dout_ld, int32_t H, int32_t W, int32_t C, float* din, int32_t din_ld,
                          void* stream);
int sgan_avgpool_pyramid_fwd(const float* label, int32_t ld, int32_t H, int32_t W, float* const* levels,
                             const int32_t* level_ld, void* stream);
int sgan_avgpool_pyramid_bwd(const float* const* dlevels, const int32_t* level_ld, int32_t H, int32_t W, float* dlabel,
                             int32_t ld, int32_t accumulate, void* stream);

/* ---- weighted L1 (cgan): loss = lambda * mean(|x - y| * w), w = 1 + sum_i ((a_i + 1)/2) * (weights_i - 1) over the
 * first nweights channels of the label image `a` (w = 1 when a == NULL; with nweights == 0, `a` is the weight map
 * itself, one value per pixel).  Also writes g = dloss/dx (unscaled by
 * the incoming gradient); the backward is dx = gout * g.  Replaces WeightedL1Loss (models/networks.py:205-214)
 * and the weight-map construction in CGANModel.backward_G (models/cgan_model.py:196-207). */
int sgan_l1w_fwd(const float* x, int32_t x_ld, const float* y, int32_t y_ld, int32_t npix, int32_t C,
                 const float* a, int32_t a_ld, const float* weights_dev, int32_t nweights, float lambda,
                 float* loss_out, float* g, int32_t g_ld, void* workspace, int64_t workspace_bytes, void* stream);
int sgan_scale(const float* gout, const float* g, float* dx, int64_t n, void* stream);   /* dx = gout[0] * g */

/* ---- elementwise helpers ---------------------------------------------------------------------
 * tanh backward: dx = dy * (1 - y*y)                                   (nn.Tanh, networks.py:540)
 * strided gather into NHWC with zero channel padding (layout boundary of the module API).  `src` of sgan_to_nhwc may also
 * be PINNED (page-locked, device-mapped) HOST memory: the gather kernel is then the host-to-device copy of the batch
 * (the transforms.ToTensor() -> .cuda() step of the reference's loop, train.py:25-29), queued with the step's kernels. */
int sgan_tanh_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* out = act(a + b) over n contiguous floats (n % 4 == 0), act = SGAN_ACT_TANH or SGAN_ACT_NONE: `nn.Tanh()(x + y)`, the
 * --use_residual tail of ResnetGenerator.forward / UnetGenerator.forward (models/networks.py:268, :367).  Backward:
 * sgan_tanh_bwd(dout, out) is the gradient of both addends. */
int sgan_add_act_fwd(const float* a, const float* b, float* out, int64_t n, int32_t act, void* stream);
int sgan_to_nhwc(const float* src, int64_t sc, int64_t sh, int64_t sw, int32_t H, int32_t W, int32_t Creal,
                 float* dst, int32_t dst_ld, int32_t Cstore, void* stream);

/* ---- the (label, image) pair of the conditional discriminators -------------------------------------
 * torch.cat((real_A, fake_B), 1) (models/cgan_model.py:162,172,187; twostage_cycle_model.py) of two NHWC buffers, written as the
 * padded NHWC buffer the discriminator reads (channels Ca + Cb .. Cstore-1 zero), and its backward: channels [c0, c0 + C) of the
 * pair's gradient as a padded NHWC buffer of their own. */
int sgan_concat_nhwc(const float* a, int32_t a_ld, int32_t Ca, const float* b, int32_t b_ld, int32_t Cb, int64_t npix,
                     float* dst, int32_t dst_ld, int32_t Cstore, void* stream);
int sgan_slice_nhwc(const float* src, int32_t src_ld, int32_t c0, int32_t C, int64_t npix, float* dst, int32_t dst_ld,
                    int32_t Cstore, void* stream);

/* ---- input pipeline tail (data/base_dataset.py:17-55, data/aligned_dataset.py:31-42) ------------
 * From a decoded (and, if asked, resized: sgan_image_resize) RGB image `img` [H0][W0][3] uint8 already in device memory: crop the n x n window at
 * (x0, y0) (transforms.RandomCrop / the aligned dataset's offsets) -> horizontal flip (RandomHorizontalFlip) -> rotate by
 * 90 deg * rot counter-clockwise (__rotate: PIL's exact transpose path for square images) -> ToTensor (/255) -> Normalize(0.5, 0.5),
 * written as an NHWC fp32 buffer [n][n][Cstore >= 3] (extra channels zero).  The random draws stay with the caller. */
int sgan_image_prep(const unsigned char* img, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t n, int32_t flip, int32_t rot,
                    float* dst, int32_t dst_ld, int32_t Cstore, void* stream);

/* ---- elastic input pipeline tail (not in the reference: the random elastic deformation of the U-Net baseline, Ronneberger et al.
 * 2015, section 3.1) ---------------------------------------------------------------------------------
 * sgan_image_prep with the address it gathers from displaced by a smooth field; util.elastic_field / util.elastic_prep are the NumPy
 * restatement.  `ctrl` is [G + 3][G + 3][2] fp32 in device memory, (dx, dy) in source pixels, 1 <= G <= 13; control point (r, s) sits
 * at crop coordinate ((s - 1) n / G, (r - 1) n / G).  For crop coordinate (u, v) -- u the column, BEFORE flip and rotation -- and per
 * axis: a = u G, cell i = a / n, t = (float)(a % n) / (float)n (integers and one correctly rounded division).  The field at (u, v) is
 * the Catmull-Rom (a = -0.5) tensor product of control points [j .. j + 3][i .. i + 3] in fp32 (weights of the four points at t:
 * -t (1 - t)^2 / 2, (1 - t)(1 + t - 1.5 t^2), t (0.5 + 2 t - 1.5 t^2), -t^2 (1 - t) / 2), each component clamped to +-127; `field_out`
 * (may be NULL) receives these floats as [n][n][2] indexed (v, u).  Then q = (int)rintf(field * 256) of the very float written, X =
 * (x0 + u) 256 + qx, Y = (y0 + v) 256 + qy, and integers only: a channel whose bit in `nearest_mask` (bit c = channel c of RGB) is
 * clear is sampled bilinearly, ix = X >> 8, fx = X & 255 (likewise y),
 *     ((256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11 + 32768) >> 16,
 * a channel whose bit is set takes the pixel at ((X + 128) >> 8, (Y + 128) >> 8).  Every index is mirrored into the image without
 * repeating the edge (period 2 (W0 - 1), any number of folds; W0 == 1 -> 0): the whole image is addressable, not only the window.
 * The value then takes sgan_image_prep's /255, (v - 0.5) / 0.5, flip / rot mapping and zero padding channels.  All-zero `ctrl` is
 * sgan_image_prep bit for bit.  Refused like sgan_image_prep, and for G outside 1..13, ctrl == NULL, or an image side above 2^22.
 * One 16-byte store per pixel when Cstore == 4, dst_ld is a multiple of 4 and dst is 16-byte aligned.  The random draws stay with
 * the caller. */
int sgan_image_prep_elastic(const unsigned char* img, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t n, int32_t flip, int32_t rot,
                            const float* ctrl, int32_t G, int32_t nearest_mask, float* dst, int32_t dst_ld, int32_t Cstore,
                            float* field_out /* may be NULL */, void* stream);

/* ---- photometric augmentation of a prepared crop (not in the reference: the "gray value variations" of the U-Net baseline and the
 * blur / gamma / contrast / noise / missing-data transforms of the EM pipelines) --------------------------------------------------
 * Out of place: `src` -> `dst`, both padded NHWC fp32 [H][W][Cstore] with values in [-1, 1] (what sgan_image_prep* writes) and their
 * own pixel strides.  Bit c of `channel_mask` marks channel c as an image channel (as in `nearest_mask`); the other channels -- the
 * labels, the padding -- are copied bit for bit.  util.photo_ref / util.photo_bounds are the NumPy restatement.  The host draws the
 * parameters; the entry reads `*rec_host` before it returns and hands the record to the kernel by value.  Per masked channel, in
 * this order, a stage whose parameter is neutral being SKIPPED, not computed (the all-neutral call copies every bit):
 *   1 blur      separable Gaussian of radius R (0 = neutral, <= SGAN_PHOTO_MAX_R, <= min(H, W) - 1), taps w[0 .. R]; rows first, then
 *               columns; indices mirrored into the crop without repeating the edge.  A pass is acc = w[0] x0, then for k = 1 .. R
 *               acc = fmaf(w[k], x(-k) + x(+k), acc); the row pass is rounded to fp32 once.
 *   2 gamma     (1 = neutral, 0.5 .. 2) u = clamp(fmaf(0.5, s, 0.5), 0, 1), u = powf(u, gamma), s = fmaf(2, u, -1)
 *   3 contrast, brightness   (contrast == 1 and brightness == 0 = neutral, contrast > 0) s = fmaf(contrast, s, 2 brightness)
 *   4 noise     (noise == NULL or sigma_n == 0 = neutral, sigma_n >= 0) s = fmaf(sigma_n, noise[j][h][w], s), `noise` a dense
 *               [popcount(channel_mask)][H][W] fp32 buffer (j counts the masked channels upwards) that the caller filled, e.g. with
 *               sgan_normal_fill: the kernel holds no random number generator
 *   5 clamp     to [-1, 1], only when stage 2, 3 or 4 ran
 *   6 occlusion nbox <= SGAN_PHOTO_MAX_BOX boxes, rows [box_y0, box_y1) x columns [box_x0, box_x1) clipped to the crop (empty boxes
 *               allowed): every masked channel becomes box_value; a later box wins.
 * One workgroup per 32 x 32 tile; the tile and its R-pixel halo are staged in LDS once, the row pass goes to a second LDS buffer.  No
 * atomics, the same bits on every run.  One 16-byte load and store per pixel when Cstore == 4, both strides are multiples of 4, both
 * pointers 16-byte aligned and at most 3 channels are masked; a scalar path otherwise.
 * Returns 1, the reason in sgan_last_error and nothing launched, for: a null src, dst or record; H, W < 1 or above 2^22; Cstore < 1
 * or a stride below it; src and dst overlapping; R outside 0 .. min(SGAN_PHOTO_MAX_R, min(H, W) - 1); gamma outside [0.5, 2];
 * contrast <= 0; sigma_n < 0; any non-finite parameter (the taps 0 .. R included); nbox outside 0 .. SGAN_PHOTO_MAX_BOX; a mask bit
 * at or above Cstore. */
#define SGAN_PHOTO_MAX_R 12
#define SGAN_PHOTO_MAX_BOX 4
typedef struct sgan_photo_rec {
    int32_t R;       /* blur radius; 0: no blur */
    float w[13];     /* w[0 .. R]: the centre tap and one side of the symmetric kernel (SGAN_PHOTO_MAX_R + 1 entries) */
    float gamma;
    float contrast;
    float brightness;
    float sigma_n;
    int32_t nbox;
    int32_t box_y0[4], box_y1[4], box_x0[4], box_x1[4];      /* SGAN_PHOTO_MAX_BOX entries each */
    float box_value[4];
} sgan_photo_rec;
int sgan_image_photo(const float* src, int32_t src_ld, float* dst, int32_t dst_ld, int32_t H, int32_t W, int32_t Cstore,
                     int32_t channel_mask, const sgan_photo_rec* rec_host, const float* noise /* may be NULL */, void* stream);

/* ---- Image.resize in front of the crop (data/base_dataset.py:19-21 transforms.Scale(.., BILINEAR), :43-50 __scale_width;
 * data/aligned_dataset.py:25 AB.resize((2 loadSize, loadSize), BICUBIC)) --------------------------
 * `src` [H][W][C] uint8 (C <= 4, interleaved) -> `dst` [Ho][Wo][C] uint8, both in device memory, bit-exact with Pillow's 8-bit
 * two-pass resampler (Resample.c): horizontal pass then vertical pass, filter support stretched by the down-scale factor, taps
 * normalised in double and rounded to 22-bit fixed point, each pass rounded and clipped to 8 bits.  `filter` uses Pillow's numbers.
 * `ws` is scratch of at least sgan_image_resize_workspace() bytes (the intermediate image and the two tap tables). */
#define SGAN_RESAMPLE_BILINEAR 2
#define SGAN_RESAMPLE_BICUBIC 3
int64_t sgan_image_resize_workspace(int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t filter);
int sgan_image_resize(const unsigned char* src, int32_t H, int32_t W, int32_t C, unsigned char* dst, int32_t Ho, int32_t Wo,
                      int32_t filter, void* ws, int64_t ws_bytes, void* stream);

/* ---- Adam over up to 64 contiguous fp32 segments in one launch --------------------------------
 * torch.optim.Adam default form (models/fcgan_model.py:98-109):
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * `state_dev` points at 16 bytes of device memory owned by the optimizer: int32 step counter t
 * (starts at 0) followed by two kernel-private floats.  A 1-thread prep launch does t += 1 and
 * derives the bias corrections in fp64, the streaming launch applies them -- so a captured
 * hipGraph replays with the right t.  `lr_dev` points at a device float (the LR schedule writes it). */
typedef struct sgan_adam_seg {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
} sgan_adam_seg;
int sgan_adam_multi(const sgan_adam_seg* segs, int32_t nseg, const float* lr_dev, float beta1, float beta2,
                    float eps, int32_t* state_dev, void* stream);

/* ---- The whole optimizer step of ONE flat arena segment in one launch: Adam (as sgan_adam_multi, same `state_dev` layout plus a ticket
 * word state_dev[3] that must start at 0) and the three derived weight copies of sgan_pack_weights for the conv weight ranges
 * `segs` inside the segment (offsets relative to `p`, sorted, disjoint; flat_t / packed_fwd / packed_bwd use the same offsets; any may be
 * NULL).  zero_grads != 0: the consumed gradients are overwritten with zeros.
 * Replaces: torch.optim.Adam.step() + zero_grad() (models/fcgan_model.py:98-109,182-191) and the weight re-layout that follows it. */
int sgan_adam_pack(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2, float eps,
                   int32_t* state_dev, float* flat_t, void* packed_fwd, void* packed_bwd, void* packed_bwd_f16, const sgan_wt_seg* segs,
                   int32_t nseg, int32_t zero_grads, void* stream);

/* ---- Zero up to 64 device buffers in one launch (the statistics arenas of a training step).  bytes[i] and ptrs[i]: multiples of 16.
 * Replaces: the aten fill launches behind torch.zeros / Tensor.zero_(). */
int sgan_zero_multi(void* const* ptrs, const int64_t* bytes, int32_t n, void* stream);

/* ---- SGD over the same segment table: buf = momentum * buf + g ; p -= lr * buf  (torch.optim.SGD with dampening 0, no Nesterov,
 * no weight decay; `m` of a segment is the momentum buffer, NULL / momentum 0 = plain gradient descent; `v` is ignored).
 * The reference's trainers are hard-wired to Adam (options/train_options.py:30 parses --optimizer and nobody reads it); this
 * is the second update rule of the boundary for callers that do read it. */
int sgan_sgd_multi(const sgan_adam_seg* segs, int32_t nseg, const float* lr_dev, float momentum, void* stream);

/* ---- Exponential moving average of parameters over up to 64 contiguous fp32 segments in one streaming launch:
 *     shadow += (1 - d_t) * (p - shadow),   d_t = decay (warmup == 0)  or  min(decay, (1 + t) / (10 + t)) (warmup != 0)
 * in fp32, one fmaf(1 - d_t, p - shadow, shadow) per element; `p` is only read.  `state_dev` points at 16 bytes of device memory
 * owned by the caller, Adam's convention: state_dev[0] is the number of updates made (starts at 0); a 1-thread prep launch does
 * t = state_dev[0] + 1, stores it (saturating at 2^30) and leaves 1 - d_t, derived in fp64, as a float in a kernel-private word;
 * the streaming launch reads that word -- so a captured hipGraph replays with the right t.
 * `shadow` and `p` of a segment need 4-byte alignment only and may be misaligned differently (ranges inside an arena).
 * decay == 1 leaves shadow bit-identical; decay == 0 without warm-up makes it bit-equal to p.  nseg == 0 or every n == 0: nothing
 * is averaged and the update still counts.  Refused, with nothing launched: nseg outside 0..64, a NULL pointer with n > 0, n < 0,
 * decay outside [0, 1], shadow and p of a segment overlapping (shadow == p included).
 * Replaces: nothing in the reference, which evaluates the last iterate. */
typedef struct sgan_ema_seg {
    float* shadow;
    const float* p;
    int64_t n;
} sgan_ema_seg;
int sgan_ema_multi(const sgan_ema_seg* segs, int32_t nseg, float decay, int32_t warmup, int32_t* state_dev, void* stream);

/* ---- N(0,1) fill (Philox4x32-10 + Box-Muller), counter-based -----------------------------------
 * Replaces: noise_.normal_(0, 1) (models/fcgan_model.py:126-127).  `offset_dev` is a device uint64
 * the kernels read; with advance != 0 it is moved on by ceil(n / 4) afterwards (graph-replay safe).  Fills with different
 * seeds are independent streams, so a net that draws several tensors per forward pass reads one offset (advance = 0) and
 * moves it once with sgan_rng_advance. */
int sgan_normal_fill(float* dst, int64_t n, uint64_t seed, uint64_t* offset_dev, int32_t advance, void* stream);
/* The same values as sgan_normal_fill on a contiguous [C][H][W] tensor, written where the generator reads them: element (c, h, w)
 * at dst[(h * W + w) * Cs + c] of a padded NHWC buffer (channels C .. Cs-1 are not touched: zero them once). */
int sgan_normal_fill_nhwc(float* dst, int32_t C, int32_t H, int32_t W, int32_t Cs, uint64_t seed, uint64_t* offset_dev,
                          int32_t advance, void* stream);
/* Two latents of the same shape drawn back to back (dst_a first; the values two sgan_normal_fill_nhwc calls give, the stream offset
 * advanced past both) by one single-block launch that also zeroes `zero` (zero_bytes, a multiple of 16, may be 0): the generator pass
 * that opens with two latents (FCGANModel.sample_noise_and_prefetch: the reference's sample_noise() of one step, fcgan_model.py:192-193,
 * and forward() of the next, :179) needs its statistics arena cleared at the same point.  <= 65536 values per latent. */
int sgan_normal_fill_nhwc_pair(float* dst_a, float* dst_b, int32_t C, int32_t H, int32_t W, int32_t Cs, uint64_t seed,
                               uint64_t* offset_dev, void* zero, int64_t zero_bytes, void* stream);
int sgan_rng_advance(uint64_t* offset_dev, uint64_t by, void* stream);

/* ---- L-BFGS advance (latent reconstruction): torch.optim.LBFGS(lr, max_iter, max_eval, tolerance_grad, tolerance_change,
 * history_size, line_search_fn=None).step(closure) as a state machine that consumes ONE closure evaluation per call.
 * Replaces: optim.LBFGS([noise], lr=0.1).step(closure) x 50 of models/fcgan_model.py:278-302.
 * Each call takes (loss[j], grad[j]) evaluated at the current x[j] of every problem j < J and runs torch's step() logic forward to the
 * point where torch would call the closure again: a fresh step() when the last one ended (phase START), or the evaluation after a move
 * (phase AFTER_MOVE).  x is updated in place.  A problem whose n_steps step() calls have finished is `done` and left untouched.
 * Nothing is read back: the call is capturable.  One workgroup per problem; vectors fp32, dot products accumulated in fp64.
 * State (one sgan_lbfgs_state per problem, device memory): the host fills the hyperparameters, zeroes everything else and sets
 * h_diag = 1; the kernel owns the rest.  Buffers (device, fp32, rows of n): d [J][n], prev_grad [J][n], hist_s / hist_y
 * [J][history_cap][n], hist_rho [J][history_cap]; x rows x_ld apart, grad rows g_ld apart, loss [J]; history_size <= history_cap. */
#define SGAN_LBFGS_MAX_PROBLEMS 8
#define SGAN_LBFGS_MAX_HISTORY 1024
#define SGAN_LBFGS_PHASE_START 0
#define SGAN_LBFGS_PHASE_AFTER_MOVE 1
/* last_exit: why the last finished step() ended */
#define SGAN_LBFGS_EXIT_NONE 0
#define SGAN_LBFGS_EXIT_OPT_START 1    /* max|g| <= tolerance_grad at the step's first evaluation */
#define SGAN_LBFGS_EXIT_GTD 2          /* g . d > -tolerance_change: no move */
#define SGAN_LBFGS_EXIT_MAX_ITER 3     /* the max_iter-th move (not re-evaluated) */
#define SGAN_LBFGS_EXIT_MAX_EVAL 4     /* evaluations of this step >= max_eval */
#define SGAN_LBFGS_EXIT_OPT_COND 5     /* max|g| <= tolerance_grad after a move */
#define SGAN_LBFGS_EXIT_SMALL_STEP 6   /* max|d t| <= tolerance_change */
#define SGAN_LBFGS_EXIT_NO_PROGRESS 7  /* |loss - prev_loss| < tolerance_change */
typedef struct sgan_lbfgs_state {
    /* hyperparameters (host) */
    float lr;
    float tolerance_grad;
    double tolerance_change;
    int32_t max_iter;
    int32_t max_eval;
    int32_t history_size;
    int32_t n_steps;        /* step() calls to run; then the problem is done */
    /* counters: torch's state['func_evals'], state['n_iter'], finished step() calls */
    int32_t func_evals;
    int32_t n_iter;
    int32_t steps;
    int32_t phase;          /* SGAN_LBFGS_PHASE_* of the NEXT evaluation */
    int32_t done;
    int32_t iter_in_step;   /* step()'s local n_iter */
    int32_t evals_in_step;  /* step()'s current_evals */
    int32_t hist_len;       /* (s, y, rho) pairs in the ring */
    int32_t hist_head;      /* ring slot of the oldest pair */
    int32_t last_exit;      /* SGAN_LBFGS_EXIT_* */
    int32_t n_skipped;      /* memory updates skipped (y . s <= 1e-10) */
    int32_t reserved0;
    /* scalars carried across evaluations and step() calls */
    float t;
    float h_diag;
    double prev_loss;
    int32_t reserved[8];
} sgan_lbfgs_state;         /* 128 bytes */
int sgan_lbfgs_advance(sgan_lbfgs_state* state, int32_t J, int64_t n, float* x, int64_t x_ld, const float* grad, int64_t g_ld,
                       const float* loss, float* d, float* prev_grad, float* hist_s, float* hist_y, float* hist_rho,
                       int32_t history_cap, void* stream);

/* ---- segmentation metrics on the device (accum_accs of the segmentation trainers: nothing comes back to the host per step) ---
 * Replaces: util.compute_Rand_F_scores (skimage.measure.label + a pixel loop, util/util.py:86-128) and the confusion matrix of
 * compute_current_accuracy (models/segm_model.py:309-331) of the reference.
 * Every entry takes `dev_err`, one caller-owned int32 in device memory, zeroed by the caller: a kernel that has to give up (a bounded
 * loop ran out, the pair table is full, a label is out of range) sets it nonzero and goes on without the offending pixel; the
 * caller looks at it when it reads the results.  No kernel loops without a bound.
 *
 * sgan_ccl_label: the 8-connected components of the NON-wall pixels of one H x W plane; a pixel is wall when x > 0.5 (a NaN is not
 *   wall).  Pixel (y, x) is read at plane[(y * W + x) * pix_stride], so channel 0 of an NHWC map is labelled where it lies.
 *   labels (int32 [H * W]): 0 for a wall pixel, else 1 + (smallest raster index y * W + x of the pixel's component): independent of
 *   scheduling, and numbered in scipy.ndimage.label's / skimage.measure.label's order.  H * W < 2^30.
 *   Three launches: union-find per 64 x 16 tile in LDS; the links that cross a tile border (corners included) by atomicMin on the
 *   label array; one pass that replaces every parent by its root.
 * sgan_rand_f_workspace: bytes of the workspace sgan_rand_f_accumulate needs for an H x W pair (< 0: bad shape).
 * sgan_rand_f_accumulate: from two label maps in sgan_ccl_label's form (t = truth, s = prediction) the exact integers
 *   A2 = sum_i a_i^2 (a_i: pixels of truth region i), B2 = sum_j b_j^2 (b_j: pixels of prediction region j inside some truth region),
 *   AB2 = sum_ij c_ij^2 (c_ij: pixels in truth region i and prediction region j), aux = pixels of a truth region on prediction wall;
 *   then in fp64  prec = (AB2 + aux) / (B2 + aux), rec = (AB2 + aux) / A2, F = 2 / (1 / prec + 1 / rec)  (NaN when A2 == 0 or
 *   B2 + aux == 0), which is util.compute_Rand_F_scores with the common 1 / n^2 cancelled; acc[0] += F, acc[1] += 1 (acc: 2 doubles,
 *   caller-owned, running sum and image count).  sums_out (4 int64: A2, B2, AB2, aux) and f_out (1 double) are optional.
 *   The workspace is caller-owned scratch; the call's own first launch zeroes it, so it may hold anything on entry, and one
 *   workspace serves any number of calls on one stream.  Counts are atomic adds indexed by label; the pair counts live in an
 *   open-addressing table of >= 2 H W slots with a probe bounded at SGAN_RAND_F_MAX_PROBE; a wave holds 64 pixels of a row and
 *   adds each key it meets once (runs collapsed, then equal keys merged across the wave).  The squares are summed as (c + n)^2 - c^2 at each add, in 64-bit integers: exact in any order.
 * sgan_vinfo_workspace: bytes of the workspace sgan_vinfo_accumulate needs: the layout of sgan_rand_f_workspace, unchanged, and 32
 *   bytes behind it (< 0: bad shape).
 * sgan_vinfo_accumulate: the information-theoretic score that goes with the Rand F-score (V^Info of the ISBI-2012 segmentation
 *   challenge), from the same label maps under the same conventions (truth wall left out, a pixel of a truth region on prediction
 *   wall is a segment of its own), and from the SAME counting pass: zero, the count kernel of sgan_rand_f_accumulate, one reduction
 *   over the counters it leaves in the workspace, one final thread.  With m = sum_i a_i and, over nonzero counts, natural log,
 *     SA = sum_i a_i ln a_i,  SB = sum_j b_j ln b_j,  SAB = sum_ij c_ij ln c_ij   (singletons add 1 ln 1 = 0):
 *     H_T = ln m - SA / m,  H_S = ln m - SB / m,  H_ST = ln m - SAB / m,  I = H_S + H_T - H_ST clamped to [0, min(H_S, H_T)],
 *     VInfo = 2 I / (H_S + H_T),  split = I / H_S,  merge = I / H_T.
 *   Degenerate cases come from the exact integers: m == 0 gives NaN; H_T is 0 iff A2 == m^2; H_S is 0 iff (aux == 0 and B2 == m^2)
 *   or m == 1; both 0: VInfo = 1; one of them 0: VInfo = 0; split / merge are NaN when their own denominator is 0.
 *   acc[0] += VInfo, acc[1] += 1.  acc_rand (optional, 2 doubles): acc_rand[0] += the Rand F-score of the pair, acc_rand[1] += 1 --
 *   the value sgan_rand_f_accumulate adds, bit for bit (the same integers through the same expression).  parts_out (optional, 11
 *   doubles): SA, SB, SAB, aux, m, H_S, H_T, I, VInfo, split, merge of this pair.  Workspace, dev_err, stream and capture as
 *   sgan_rand_f_accumulate.  m and aux are exact; SA, SB, SAB are fp64 sums in an order that depends on scheduling (one wave-level
 *   shuffle reduction, one fp64 atomic add per workgroup and sum), so they repeat to rounding (~H W 2^-53 relative), not to the bit.
 * sgan_confusion_accumulate: conf[truth * k + pred] += 1 per pixel, conf int64 [k * k], caller-owned.  pred = argmax over the C
 *   logical channels (C <= 16) of x at pixel stride x_ld; truth = label[p] (int64 map) when label is given, else the argmax of y in
 *   the same way.  add_background: class C = 1 - min(1, sum_c v_c) (fp32, summed in channel order) is appended to both channel
 *   maps before the argmax and k = C + 1, else k = C.  Ties go to the first maximum and a NaN counts as the maximum, as in
 *   torch.argmax.
 * sgan_thin_workspace: bytes of the workspace sgan_thin needs for an H x W plane (< 0: bad shape).
 * sgan_thin: Guo-Hall thinning of the wall pixels of one plane to one-pixel lines, as skimage.morphology.thin performs it (the border
 *   thinning of the ISBI-2012 scores: compute_Rand_F_scores(..., do_thin=True), util/util.py:99-101 of the reference; util.thin is
 *   the host restatement the kernel is tested against).  The plane is read as sgan_ccl_label reads it (pixel stride, wall when
 *   x > 0.5, a NaN is not wall); out is a dense float [H * W] plane of 0.0 / 1.0, so sgan_ccl_label(out, 1, ...) labels the thinned
 *   map.  An iteration is two sub-iterations, each deciding every wall pixel from one snapshot of its 8 neighbours (outside the
 *   image = 0); max_num_iter <= 0 means "until nothing changes".  iters_out (optional, one int32 in device memory) receives the number
 *   of iterations that deleted something.
 *   Nothing is read back and nothing is decided on the host: a call enqueues a sequence of launches that depends on (H, W,
 *   max_num_iter) only -- init, ceil(iterations / 8) tile launches of up to 8 iterations each (a 32 x 32 core with a 16-pixel halo
 *   in LDS), emit -- so it can be captured in a hipGraph and replayed on data that needs any other number of iterations.  Per-iteration
 *   deletion counters in the workspace carry convergence: a tile launch whose predecessor deleted nothing returns at once.
 *   "Until nothing changes" is budgeted at min(H, W) / 2 + 2 iterations (an all-wall plane needs min(H, W) / 2 + 1), and a larger
 *   max_num_iter is cut to the budget; if the budget's last iteration still deleted something, *dev_err gets bit 16 and out holds
 *   the state reached.  The result is integers: the same bits on every run.  Workspace, dev_err and stream as sgan_rand_f_accumulate;
 *   the call's first launch initialises what it uses.  H * W < 2^30 and H <= 65535 * 32 (one grid row per 32 image rows); both entries
 *   refuse any other shape. */
#define SGAN_RAND_F_MAX_PROBE 1024
int sgan_ccl_label(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* labels, int32_t* dev_err, void* stream);
int64_t sgan_rand_f_workspace(int32_t H, int32_t W);
int sgan_rand_f_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, void* workspace,
                           int64_t workspace_bytes, double* acc, int64_t* sums_out, double* f_out, int32_t* dev_err, void* stream);
int64_t sgan_vinfo_workspace(int32_t H, int32_t W);
int sgan_vinfo_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, void* workspace,
                          int64_t workspace_bytes, double* acc, double* acc_rand, double* parts_out, int32_t* dev_err, void* stream);
int sgan_confusion_accumulate(const float* x, int32_t x_ld, int32_t C, const int64_t* label, const float* y, int32_t y_ld,
                              int32_t add_background, int64_t npix, int64_t* conf, int32_t* dev_err, void* stream);
int64_t sgan_thin_workspace(int32_t H, int32_t W);
int sgan_thin(const float* plane, int64_t pix_stride, int32_t H, int32_t W, float* out, int32_t max_num_iter, void* workspace,
              int64_t workspace_bytes, int32_t* iters_out, int32_t* dev_err, void* stream);

/* ---- object-level scores on the device: detection F1, average precision, SEG and panoptic quality ----------------------------------
 * What the cell-segmentation literature reports beside Rand and VInfo: how many cells were found, at which overlap, and how well
 * the found ones fit (F1 at IoU 0.5; the average precision over IoU 0.5 .. 0.95 of DSB-2018 / StarDist's matching_dataset; the
 * Cell Tracking Challenge's SEG; panoptic quality).  util.object_match_counts is the NumPy / scipy restatement these entries are
 * tested against, util.object_scores derives the four scores.
 *
 * Inputs: two H x W label maps in sgan_ccl_label's form, t the truth and s the prediction: 0 is wall, any other value is 1 + the
 *   region's smallest raster index.
 * Counts: unlike the Rand count, areas are WHOLE areas.  a_i = all pixels of truth region i, those on prediction wall included;
 *   b_j = all pixels of prediction region j, those on truth wall included; c_ij = pixels in both; u_ij = a_i + b_j - c_ij.
 * Small objects: min_area >= 1.  A region with area < min_area, on either side, is treated as absent: it is not counted and cannot
 *   be matched.  No other region's area changes.  N_t = truth regions with a_i >= min_area, N_s = prediction regions with
 *   b_j >= min_area.
 * Matches at threshold k = 0 .. 9, tau_k = (10 + k) / 20: TP_k = number of pairs (i, j) that both pass min_area and satisfy
 *   20 c_ij > (10 + k) u_ij.  The comparison is strict and is done in 64-bit integers; no floating-point comparison decides a match.
 *   For an IoU above 1/2 the matching is unique (c_ij > u_ij / 2 means more than half of a_i and more than half of b_j, and two
 *   disjoint regions cannot both hold more than half of a third), so no assignment problem is solved and every count is exact.
 * Float sums: SIoU = sum of c_ij / u_ij (fp64) over the pairs counted in TP_0.  Over the pairs with both sides >= min_area and
 *   2 c_ij > a_i (at most one j per i), SEGn is their number and SSEG the sum of c_ij / u_ij.
 * Accumulators, caller-owned on the device, zeroed by the caller once, pooled over a dataset as matching_dataset pools them:
 *   acc_i, int64[SGAN_OBJ_COUNTS]: [SGAN_OBJ_TP0 + k] += TP_k, [SGAN_OBJ_NT] += N_t, [SGAN_OBJ_NS] += N_s, [SGAN_OBJ_IMAGES] += 1,
 *     [SGAN_OBJ_SEGN] += SEGn, [14] = [15] = 0;
 *   acc_f, double[SGAN_OBJ_SUMS]: [SGAN_OBJ_SIOU] += SIoU, [SGAN_OBJ_SSEG] += SSEG.
 *   counts_out (int64[16]) and sums_out (double[2]), both optional, receive this pair's contribution alone.
 * Scores, derived on the host from the pooled numbers when the accumulators are read; a score whose denominator is 0 reads 0:
 *   ObjF1 = 2 TP_0 / (N_t + N_s),  ObjAP = mean over k of TP_k / (N_t + N_s - TP_k),  SEG = SSEG / N_t,  PQ = SIoU / ((N_t + N_s) / 2).
 * Exactness: the integers are identical on every run and in every scheduling order.  SIoU and SSEG are fp64 sums of at most N_t
 *   terms in (0, 1], in an order that depends on scheduling: they repeat to rounding (N_t 2^-52 relative), not to the bit, as
 *   VInfo's sums.
 *
 * sgan_object_match_workspace: bytes of the workspace sgan_object_match_accumulate needs for an H x W pair (< 0: bad shape).
 * sgan_object_match_accumulate: four launches whose grids depend on (H, W) only, nothing read back and nothing decided on the
 *   host, so the call captures into a hipGraph and replays on any other pair of maps (min_area is a launch argument, frozen with
 *   the capture).  Zero; a counting pass that is sgan_rand_f_accumulate's (a wave holds 64 pixels of a row, runs collapsed, equal
 *   keys merged across the wave, the pair table with its probe bounded at SGAN_RAND_F_MAX_PROBE) with every non-wall prediction
 *   pixel counted and no square sums; an evaluation pass over the per-label counters and the pair-table slots (16-byte loads, the
 *   two areas of a pair looked up through its key, ten integer comparisons, the fp64 terms reduced in the wave and the workgroup,
 *   one set of atomics per workgroup into a staging block in the workspace); one final thread that adds the staging block to the
 *   accumulators and writes the optional outputs.  Workspace, dev_err (bit 2 = pair table full, bit 4 = label out of range, the
 *   offending pixel left out) and stream as sgan_rand_f_accumulate; the call initialises what it uses.  Shapes as
 *   sgan_rand_f_accumulate.  Null required pointers, min_area < 1 and a short workspace are refused before any launch. */
#define SGAN_OBJ_COUNTS 16
#define SGAN_OBJ_TP0 0
#define SGAN_OBJ_NT 10
#define SGAN_OBJ_NS 11
#define SGAN_OBJ_IMAGES 12
#define SGAN_OBJ_SEGN 13
#define SGAN_OBJ_SUMS 2
#define SGAN_OBJ_SIOU 0
#define SGAN_OBJ_SSEG 1
int64_t sgan_object_match_workspace(int32_t H, int32_t W);
int sgan_object_match_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, int32_t min_area, void* workspace,
                                 int64_t workspace_bytes, int64_t* acc_i, double* acc_f, int64_t* counts_out, double* sums_out,
                                 int32_t* dev_err, void* stream);

/* ---- boundary scores on the device: exact Euclidean distance transform, boundary F-measure, Hausdorff distance, ASSD ----------------
 * Where the predicted wall lies relative to the true one, which the region scores above do not see: the boundary F-measure at a
 * pixel tolerance (BSDS500's F in its distance-threshold form, `bfscore`; not the bipartite correspondPixels matching), the Hausdorff
 * distance and the average symmetric surface distance (GlaS and the medical challenges).  util.edt_sq and util.boundary_counts are
 * the NumPy restatements these entries are tested against, util.boundary_scores derives the scores.
 *
 * sgan_edt_workspace: bytes of the workspace sgan_edt_sq needs for an H x W plane (< 0: bad shape).
 * sgan_edt_sq: the exact squared Euclidean distance transform.  The plane is read as sgan_ccl_label reads it, pixel (y, x) at
 *   plane[(y * W + x) * pix_stride]; a pixel is wall when its value is > 0.5 (a NaN and an exact 0.5 are not wall).
 *   dsq[y * W + x] = min over the wall pixels (y', x') of (y - y')^2 + (x - x')^2, an exact int32: 0 on a wall pixel, -1 everywhere
 *   when the plane has no wall pixel (the convention of sgan_border_weight's d1sq), the same bits on every run.
 *   Shapes: H, W <= 32768 and H W < 2^30, so that (H - 1)^2 + (W - 1)^2 < 2^31.  Anything else, a null pointer, a pixel stride < 1
 *   and a short or misaligned (16 bytes) workspace return 1 with sgan_last_error set and nothing launched.
 *   Four launches whose grids depend on (H, W) only, nothing read back and nothing decided on the host, so the call captures into a
 *   hipGraph and replays on any other plane: a counter zeroed; the wall bits of every segment of 32 rows of every column as one
 *   mask word, and the number of wall pixels added to the counter; per (column, segment) the vertical distance g to the column's
 *   nearest wall pixel, the nearest wall row outside the segment looked up in the other segments' masks (nearest first, at most
 *   H / 32 each way); per row dsq = min over x' of (x - x')^2 + g(y, x')^2, g^2 staged in LDS 2048 columns at a time, each thread
 *   scanning outward from its own x until r^2 >= its best so far (exact; bounded by W), a longer row walked in chunks nearest first.
 *   A plane without a wall is decided from the counter on the device.  The workspace may hold anything on entry.
 *   dev_err is accepted like every metric entry's (required, not null); this entry sets no bit of it.
 *
 * sgan_boundary_workspace: bytes of the workspace sgan_boundary_accumulate needs for an H x W pair (< 0: bad shape).
 * sgan_boundary_accumulate: t_dsq and s_dsq are sgan_edt_sq outputs of the truth and of the predicted plane.
 *   Wall pixels: a pixel is a wall pixel of a map where that map's own dsq is 0.  A predicted wall pixel p has distance^2 t_dsq[p]
 *     to the truth; a truth wall pixel has s_dsq[p] to the prediction.  -1 (the other map has no wall) is "not defined".
 *   Bins: the bin of a distance^2 d is k = ceil(sqrt(d)), decided in integers: (k - 1)^2 < d <= k^2 for k = 0 .. 30; bin 31 holds
 *     d > 900 and d = -1.  For an integer tolerance theta <= 30, "within theta" is therefore bin <= theta <=> d <= theta^2, exactly.
 *   acc_i, int64[SGAN_BND_COUNTS], caller-owned on the device, zeroed by the caller once, pooled over a dataset:
 *     [0 .. 31] += histogram of the predicted wall pixels by bin;  [32 .. 63] += histogram of the truth wall pixels by bin;
 *     [64] += N_s, the predicted wall pixels;  [65] += N_t, the truth wall pixels;  [66] += 1 (images);
 *     [67] += 1 when both maps have wall (Hausdorff defined);  [68] += predicted wall pixels with a defined distance;
 *     [69] += truth wall pixels with a defined distance;  [70] = max over all images of the largest distance^2 on the predicted
 *     side;  [71] the same on the truth side;  the remaining entries are 0.
 *   acc_f, double[SGAN_BND_SUMS]: [0] += sum of sqrt(d) over the predicted wall pixels with a defined distance;  [1] += the same
 *     over the truth wall pixels;  [2] += this image's Hausdorff distance sqrt(max of the two sides' largest d), when defined;  [3] = 0.
 *   counts_out (int64[80]) and sums_out (double[4]), both optional, receive this pair's contribution alone, [70] and [71] holding
 *     this pair's maxima.
 *   Scores, derived on the host from the pooled numbers (util.boundary_scores); a score whose denominator is 0 reads 0:
 *     BoundP = sum_{k <= theta} acc_i[k] / N_s,  BoundR = sum_{k <= theta} acc_i[32 + k] / N_t,  BoundF = 2 P R / (P + R),
 *     HausD = acc_f[2] / acc_i[67],  ASSD = (acc_f[0] + acc_f[1]) / (acc_i[68] + acc_i[69]).
 *   Exactness: the integers are exact (64-bit adds, an integer max) and identical in every scheduling order.  The fp64 sums are sums
 *     of n correctly rounded square roots: within n 2^-52 relative of the exact sum.
 *   Two launches whose grids depend on (H, W) only, nothing read back: a grid-stride count pass whose workgroups gather histograms
 *   and counters in LDS and store them, with their two fp64 sums, in a slot of their own in the workspace; one workgroup that adds
 *   the slots in slot order, decides "Hausdorff defined", adds to the accumulators and writes the optional outputs.  The workspace
 *   may hold anything on entry.  dev_err as sgan_edt_sq: required, no bit set.  H W < 2^30.  Null required pointers, a bad shape and a
 *   short workspace are refused before any launch: return 1, the reason in sgan_last_error. */
#define SGAN_BND_BINS 32
#define SGAN_BND_COUNTS 80
#define SGAN_BND_SUMS 4
int64_t sgan_edt_workspace(int32_t H, int32_t W);
int sgan_edt_sq(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* dsq, void* workspace, int64_t workspace_bytes,
                int32_t* dev_err, void* stream);
int64_t sgan_boundary_workspace(int32_t H, int32_t W);
int sgan_boundary_accumulate(const int32_t* t_dsq, const int32_t* s_dsq, int32_t H, int32_t W, void* workspace, int64_t workspace_bytes,
                             int64_t* acc_i, double* acc_f, int64_t* counts_out, double* sums_out, int32_t* dev_err, void* stream);

/* ---- cleaning the prediction: disk closing, speck removal and small-cell filling of a wall map before it is scored ----------------
 * What every pipeline that reports the scores above does to its thresholded wall map first: close pin-hole gaps in the membrane
 * (one missing wall pixel merges two cells), drop wall specks inside cells, fill regions too small to be a cell.
 * util.clean_wall is the NumPy / scipy restatement these entries are tested against.
 *
 * The plane is read as sgan_ccl_label reads it: pixel (y, x) at plane[(y * W + x) * pix_stride], wall when x > 0.5 (a NaN and an
 * exact 0.5 are not wall).  Three stages in this order, each skipped when its parameter is 0, all in integers:
 *   1. close, close_rsq >= 1 (a squared Euclidean radius):  D = {p : 0 <= edt_sq(wall)(p) <= close_rsq};
 *      wall1 = {p : edt_sq(~D)(p) > close_rsq, or ~D is empty}.  Only pixels inside the image take part: the dilation counts the
 *      outside as free and the erosion counts it as wall, so the closing never eats the wall at the image border and wall1 contains
 *      wall; an empty wall stays empty.  With the disk {dy^2 + dx^2 <= close_rsq} this is scipy.ndimage.binary_dilation(border_value
 *      = 0) followed by binary_erosion(border_value = 1).
 *   2. specks, min_wall >= 1:  the 8-connected components of wall1 with fewer than min_wall pixels become free: wall2.
 *   3. small cells, min_cell >= 1:  the 8-connected components of ~wall2 with fewer than min_cell pixels become wall: out.
 *   out is a dense float [H * W] plane of 0.0 / 1.0, which sgan_ccl_label, sgan_thin and sgan_edt_sq read as it lies; it may not
 *   alias the plane.  With all three parameters 0 it is the thresholded plane.
 *   acc (optional, int64[SGAN_CLEAN_COUNTS], caller-owned on the device, zeroed by the caller once, pooled over a dataset):
 *     [0] += pixels set by the closing;  [1] += wall components removed;  [2] += wall pixels removed;  [3] += cells filled;
 *     [4] += cell pixels filled;  [5] += 1 (images).  Exact integers, identical in every scheduling order.
 *
 * sgan_clean_workspace: bytes of the workspace sgan_clean_wall needs for an H x W plane (< 0: bad shape).
 * sgan_clean_wall: the launch sequence depends on (H, W) and on which of the three parameters are nonzero, on nothing else; nothing
 *   is read back and nothing is decided on the host, so the call captures into a hipGraph and replays on any other plane.
 *   Closing: sgan_edt_sq, a threshold pass that writes the complement of D, sgan_edt_sq of that, a threshold pass that writes wall1
 *   (and its complement when stage 2 follows) and counts the pixels the input did not have.  Each area filter: sgan_ccl_label (of
 *   the complement plane for the specks, whose free components are the wall's), the count table zeroed, a count pass that adds
 *   every pixel to count[label - 1] -- the label IS 1 + the component's smallest raster index, so it indexes an int32 [H W] table
 *   directly; a wave merges its 64 pixels by label with ballots and issues one atomic per distinct label -- and an apply pass that
 *   writes the filtered plane and counts the components (at their root pixel) and pixels that changed side.  Without a stage, one
 *   pass copies the thresholded plane.
 *   The workspace (16-byte aligned) may hold anything on entry.  dev_err as sgan_ccl_label: required; bit 1 from the labelling, bit 4
 *   for a label out of range.  Shapes as sgan_edt_sq: H, W <= 32768 and H W < 2^30.  Returns 1, the reason in sgan_last_error and
 *   nothing launched, for a null required pointer (acc alone is optional), a bad shape, a pixel stride < 1, a negative parameter,
 *   close_rsq > 4096, out == plane, and a short or misaligned workspace. */
#define SGAN_CLEAN_COUNTS 6
int64_t sgan_clean_workspace(int32_t H, int32_t W);
int sgan_clean_wall(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t close_rsq, int32_t min_wall, int32_t min_cell,
                    float* out, int64_t* acc, void* workspace, int64_t workspace_bytes, int32_t* dev_err, void* stream);

/* ---- splitting merged cells at wall gaps: a core-seeded flood of the free space and a cut where two floods meet -------------------
 * One gap in a wall merges two cells into one component.  A closing only mends gaps narrower than its disk; this stage cuts a gap of
 * any length at its neck, as long as the neck is narrower than the cells on either side: the distance transform of the free space,
 * one marker per "core" (where the distance to the wall is large), the markers grown back, a wall set where two markers meet.
 * util.split_cells is the NumPy / scipy restatement these entries are tested against.  All integers.
 *
 * The plane is read as sgan_ccl_label reads it: pixel (y, x) at plane[(y * W + x) * pix_stride], wall when x > 0.5 (a NaN and an
 * exact 0.5 are not wall).  Parameters: split_rsq in 1 .. 4096, a squared Euclidean radius; max_rounds in 1 .. 4096.
 *   1. d = edt_sq(wall).  A plane without wall (d == -1 everywhere) has no core: out is the empty wall map.
 *   2. Cores: core = {p free : d(p) >= split_rsq}; its 8-connected components, each labelled 1 + its smallest raster index.
 *   3. Flood: g(p) = the length of the shortest 8-connected path through free pixels from the free pixel p to a core pixel (0 on a
 *      core).  If g(p) <= max_rounds, L(p) = the smallest core label among the core components at geodesic distance exactly g(p) from
 *      p; otherwise, and on the wall, L(p) = 0.  This is max_rounds synchronous rounds of "an unlabelled free pixel takes the smallest
 *      label among its 8 labelled neighbours of the round before", so it does not depend on scheduling.
 *   4. Cut: a free pixel p with L(p) != 0 becomes wall when one of its neighbours E, SW, S, SE inside the image has L(q) != 0 and
 *      L(q) != L(p).  Every 8-adjacent pair falls under this rule for one of its members: afterwards no two free 8-adjacent pixels
 *      carry different nonzero labels.  A cell without a core, a cell with one core and what the budget did not reach are never cut.
 *   5. out = wall | cut, a dense float [H * W] plane of 0.0 / 1.0, which sgan_ccl_label, sgan_thin, sgan_edt_sq and sgan_clean_wall
 *      read as it lies; it may not alias the plane.
 *   acc (optional, int64[SGAN_SPLIT_COUNTS], caller-owned on the device, zeroed by the caller once, pooled over a dataset):
 *     [0] += core components;  [1] += cut pixels set;  [2] += free pixels with L != 0;  [3] += rounds that labelled at least one
 *     pixel;  [4] += 1 if round max_rounds still labelled something (the budget was hit);  [5] += 1 (images).  Exact integers,
 *     identical in every scheduling order.
 *
 * sgan_split_workspace: bytes of the workspace sgan_split_cells needs for an H x W plane (< 0: bad shape).
 * sgan_split_cells: the launch sequence depends on (H, W, max_rounds) only; nothing is read back and nothing is decided on the host,
 *   so the call captures into a hipGraph and replays on a plane that needs any other number of rounds.  sgan_edt_sq; a threshold
 *   pass that writes the core plane and zeroes the round counters; sgan_ccl_label of it; ceil(max_rounds / 8) flood launches of up
 *   to 8 rounds each (a 48 x 32 core with an 8-pixel halo of int32 labels in LDS, two label planes ping-ponged between launches);
 *   one cut-and-emit pass that also finishes the counters.  Per-round "labelled something" counters in the workspace carry
 *   convergence: a flood launch whose predecessor's last round labelled nothing returns at once.  No floating point after the
 *   threshold; atomics only on integer counters and flags.
 *   The workspace (16-byte aligned) may hold anything on entry.  dev_err as sgan_clean_wall: required; bit 1 from the labelling, and
 *   bit 64 when round max_rounds still labelled something -- out is then still the map defined above, for that budget.  Shapes as
 *   sgan_edt_sq.  Returns 1, the reason in sgan_last_error and nothing launched, for a null required pointer (acc alone is
 *   optional), a bad shape, a pixel stride < 1, split_rsq or max_rounds outside 1 .. 4096, out == plane, and a short or misaligned
 *   workspace. */
#define SGAN_SPLIT_COUNTS 6
int64_t sgan_split_workspace(int32_t H, int32_t W);
int sgan_split_cells(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t split_rsq, int32_t max_rounds, float* out,
                     int64_t* acc, void* workspace, int64_t workspace_bytes, int32_t* dev_err, void* stream);

/* ---- topology scores on the device: windowed Betti errors and clDice ------------------------------------------------------------
 * Whether the predicted wall has the topology of the true one, which neither the region nor the boundary scores say: the Betti
 * error of the membrane-segmentation literature (the absolute difference in the number of wall components and of enclosed cells,
 * window by window) and clDice, the centre-line Dice (Shit et al. 2021), with the library's Guo-Hall thinning for its skeletons.
 * util.betti_window and util.topo_counts are the NumPy / scipy restatements this entry is tested against, util.topo_scores derives
 * the scores.
 *
 * Planes: t (truth) and s (prediction) are read as sgan_ccl_label reads its plane, pixel (y, x) at t[(y * W + x) * t_ld]; a pixel is
 *   wall when its value is > 0.5 (a NaN and an exact 0.5 are not wall).  t_thin and s_thin are dense [H * W] planes, the sgan_thin
 *   outputs of t and s; each may be null, and the two counters of a null side are then left alone (counts_out: 0).
 * Windows: wh = min(window, H) by ww = min(window, W) pixels, at the origins oy = 0, stride, 2 stride, ... while oy + wh <= H and
 *   likewise in x; a strip at the bottom or the right that no full window covers is not scored.  8 <= window <= 64 and
 *   1 <= stride <= window.
 * Betti numbers of a window, everything outside the window counting as free:
 *   b0 = the number of 8-connected components of its wall pixels;
 *   b1 = the number of 4-connected components of its free pixels that own no pixel of the window's edge (the enclosed cells).
 *   Then b0 - b1 = (Q1 - Q3 - 2 Qd) / 4, Gray's bit-quad count for 8-connectivity over the window padded with one free ring.
 * acc_i, int64[SGAN_TOPO_COUNTS], caller-owned on the device, zeroed by the caller once, pooled over a dataset:
 *   [0] += windows;  [1] += sum over the windows of |b0(S) - b0(T)|;  [2] += the same of b1;  [3] += sum of b0(S);  [4] += sum of b0(T);
 *   [5] += sum of b1(S);  [6] += sum of b1(T);  [7] += pixels of s_thin (skel_s);  [8] += those of them that are wall in t;
 *   [9] += pixels of t_thin (skel_t);  [10] += those of them that are wall in s;  [11] += 1 (images).
 *   counts_out (int64[SGAN_TOPO_COUNTS], optional) receives this pair's contribution alone.
 * Scores, derived on the host from the pooled integers (util.topo_scores); a score whose denominator is 0 reads 0:
 *   Betti0Err = [1] / [0],  Betti1Err = [2] / [0],  Tprec = [8] / [7],  Tsens = [10] / [9],  clDice = 2 Tprec Tsens / (Tprec + Tsens).
 * Exactness: integers only, 64-bit atomic adds: the same bits in every scheduling order.
 * Launches: one workgroup per (window, map) stages the window's wall bits in LDS, labels wall (8-connected) and free (4-connected)
 *   pixels in one union-find forest in LDS, counts the roots and writes (b0, b1) to the workspace; a grid-stride launch sums them;
 *   with a thinned plane a grid-stride launch over the pixels counts the skeletons.  The grids depend on (H, W, window, stride)
 *   alone, nothing is read back, no workgroup waits for another: the call captures into a hipGraph and replays on any other pair.
 *   Every loop of the labelling is bounded by the window's 4096 nodes; a window whose loop ran out sets bit SGAN_TOPO_ERR_BIT of
 *   dev_err and contributes nothing.  The workspace may hold anything on entry; 16-byte aligned.
 * sgan_topo_workspace_bytes: bytes of that workspace (< 0: a window or stride that is not covered, or a bad shape).
 * Returns 1 ("not covered"), the reason in sgan_last_error and nothing launched, for a window outside 8 .. 64 or a stride outside
 *   1 .. window, and likewise for a null required pointer (t_thin, s_thin and counts_out are optional), a shape outside
 *   H, W <= 32768 and H W < 2^30, a pixel stride < 1 and a short or misaligned workspace. */
#define SGAN_TOPO_COUNTS 12
#define SGAN_TOPO_SKEL_S 7
#define SGAN_TOPO_IMAGES 11
#define SGAN_TOPO_ERR_BIT 256
int64_t sgan_topo_workspace_bytes(int32_t H, int32_t W, int32_t window, int32_t stride);
int sgan_topo_accumulate(const float* t, int64_t t_ld, const float* s, int64_t s_ld, const float* t_thin, const float* s_thin, int32_t H,
                         int32_t W, int32_t window, int32_t stride, void* workspace, int64_t workspace_bytes, int64_t* acc_i,
                         int64_t* counts_out, int32_t* dev_err, void* stream);

/* ---- whole-image inference: overlap tiles with blended seams, averaged over the 8 flips and rotations (not in the reference, whose
 * test_ss.py scores one crop; the overlap-tile strategy of Ronneberger et al. 2015, section 2) ------------------------------------
 * util.tile_plan / tile_window / prep_tile_ref / blend_tiles_ref are the NumPy restatement.  Per axis of length L: the
 * padded domain is -M .. L + M - 1, mirrored into the image without repeating the edge; tiles of side T start at -M, -M + S, ... and
 * the last at L + M - T; the integer window of a tile is w(i) = clamp(min(i + 1, T - i) - M, 0, R), zero in the margin M, a ramp of R
 * pixels, then flat; a pass has the D4 element (flip, rot) of sgan_image_prep: horizontal flip, then rot x 90 degrees counter-clockwise.
 *
 * sgan_image_prep_tile: sgan_image_prep whose h x w window at (x0, y0) may reach up to H0 - 1 / W0 - 1 pixels outside the image (indices
 *   reflected) and may be rectangular (then rot == 0).  The same bits as sgan_image_prep for a square window inside the image.  One
 *   16-byte store per pixel when Cstore == 4, dst_ld is a multiple of 4 and dst is 16-byte aligned.
 * sgan_tile_blend: one pass.  `logits` is the generator's raw output for the tile at (x0, y0) under (flip, rot), [T][T][ld] NHWC with C <= 4
 *   logical channels; p = softmax over the C channels (mode SGAN_SEGHEAD_SOFTMAX, sgan_softmax_fwd's expression) or the sigmoid of each
 *   (SGAN_SEGHEAD_SIGMOID, sgan_sigmoid_nhwc_fwd's).  For every pixel (Y, X) of the H x W `canvas` that the window shows with weight
 *   w = w(Y - y0) w(X - x0) > 0: canvas[Y][X][c] = fmaf(w, p_c at the tile pixel that shows (Y, X), canvas[Y][X][c]).  Plain loads and
 *   stores: a canvas pixel has one writer per launch, the stream orders the launches.  The caller zeroes the canvas before the first pass.
 * sgan_tile_finish: prob = canvas / (float)(n_tta Wy[Y] Wx[X]) and logp = logf(max(prob, FLT_MIN)), n_tta 1 or 8; Wy [H], Wx [W] int32
 *   in device memory (util.tile_plan).  Padding channels of both outputs are written as zeros.
 * logits, canvas, prob, logp: pixel stride a multiple of 4 floats, 16-byte aligned.  Refused (status, nothing launched): C outside 1..4,
 *   R outside 1..64, M < 0 or 2 M >= T, M > min(H, W) - 1, T > min(H, W) + 2 M, an origin outside -M .. L + M - T, a rotated rectangle,
 *   a window one reflection cannot fold back, a null pointer, a side above 2^22. */
int sgan_image_prep_tile(const unsigned char* img, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t h, int32_t w, int32_t flip,
                         int32_t rot, float* dst, int32_t dst_ld, int32_t Cstore, void* stream);
int sgan_tile_blend(const float* logits, int32_t ld, int32_t C, int32_t mode, int32_t x0, int32_t y0, int32_t T, int32_t M, int32_t R,
                    int32_t flip, int32_t rot, float* canvas, int32_t canvas_ld, int32_t H, int32_t W, void* stream);
int sgan_tile_finish(const float* canvas, int32_t canvas_ld, int32_t H, int32_t W, int32_t C, const int32_t* Wy, const int32_t* Wx,
                     int32_t n_tta, float* prob, int32_t prob_ld, float* logp, int32_t logp_ld, void* stream);

/* ---- differentiable augmentation of discriminator inputs (DiffAugment, Zhao et al. 2020; not in the reference, which trains its
 * discriminators on the bare crops) ---------------------------------------------------------------------------------------------------
 * util.diffaug_params / diffaug_ref / diffaug_bwd_ref are the NumPy fp64 restatement.  One image x[H][W][Cs] (padded
 * NHWC fp32, C logical channels) and one 32-byte record sgan_diffaug_rec {b, a, ty, tx, cy0, cy1, cx0, cx1}:
 *     m = mean of x over all pixels and the colour channels (the set bits of colour_mask), an fp64 sum in a fixed order, rounded once
 *     K(h, w) = 0 inside the cutout cy0 <= h < cy1, cx0 <= w < cx1, 0 where (h + ty, w + tx) lies outside the image, else 1
 *     y[h][w][c] = K(h, w) g_c(x[h + ty][w + tx][c]),  g_c(v) = a (v - m) + m + b on a colour channel, v on any other, 0 for c >= C
 *   evaluated as t = v - m, u = fmaf(a, t, m) (skipped when a == 1), u + b (skipped when b == 0): the identity record copies bits.
 *   Backward, n = colour channels x H x W, S = the sum of K(q) dy[q][c] over every q and colour c (fp64, fixed order):
 *     dx[p][c] = fmaf(a, K(p - t) dy[p - t][c], (float)((1 - a) S / n)) on a colour channel when a != 1, K(p - t) dy[p - t][c] otherwise
 *   Pixels with K = 0 are never read.  One 16-byte access per lane per group of 4 stored channels; no atomics: the same input and
 *   record give the same bits on every run.
 *
 * sgan_diffaug_draw: one record per job into params_dev from Philox4x32-10 under `seed`: job j takes the blocks at counters
 *   offset + 2 j (words w0..w3) and offset + 2 j + 1 (w4, w5), c2 = 0 -- whatever the policy, so that switching one operation off
 *   does not move the others.  policy_bits: SGAN_DIFFAUG_TRANSLATION | _CUTOUT | _BRIGHTNESS | _CONTRAST.
 *     b = (w0 >> 8) 2^-24 - 0.5 (else 0);  a = (w1 >> 8) 2^-24 + 0.5, one fp32 addition (else 1);  Sy = floor(H rt + 0.5), ty = -Sy + w2 mod (2 Sy + 1), tx
 *     from w3 and W (else 0);  ch = floor(H rc + 0.5), oy = w4 mod (H + 1 - ch mod 2), cy0 = max(0, oy - ch / 2), cy1 = min(H, oy - ch / 2
 *     + ch), cx0 / cx1 from w5 and W (else the empty rectangle 0, 0, 0, 0).  shapes: {H, W} per job, host memory.
 *   One launch of one workgroup; `offset_dev` (a device uint64, NULL = 0) is read by the kernel and with advance != 0 moved on by
 *   2 njobs, so a captured hipGraph draws afresh on every replay (sgan_normal_fill's convention).
 * sgan_diffaug_multi_fwd / _bwd: every job {src, dst, H, W, C, Cs, colour_mask} of a step stage in one call; job j reads record j of
 *   params_dev (written by sgan_diffaug_draw or by the caller).  For _bwd src is dy and dst is dx.
 *   workspace == NULL: the contrast-free form, ONE launch; the record's `a` is not read and taken as 1 (the caller's policy has no
 *   contrast).  Otherwise sgan_diffaug_workspace(njobs) bytes of device memory, 8-byte aligned, any content: TWO launches, the first
 *   leaves every workgroup's partial fp64 sum in a slot of its own, the second sums a job's slots in a fixed order and transforms.
 * Refused (status 1, nothing launched or written): njobs outside 1..8, a null or 16-byte-misaligned src / dst, src == dst, H or W
 *   outside 1..32768, Cs not a multiple of 4 or outside 4..32, C outside 1..Cs, a colour_mask bit at or above C, H W Cs >= 2^31, rt or
 *   rc outside [0, 1], unknown policy bits, a null params_dev. */
#define SGAN_DIFFAUG_TRANSLATION 1
#define SGAN_DIFFAUG_CUTOUT 2
#define SGAN_DIFFAUG_BRIGHTNESS 4
#define SGAN_DIFFAUG_CONTRAST 8
#define SGAN_DIFFAUG_MAX_JOBS 8
typedef struct sgan_diffaug_rec {
    float b, a;
    int32_t ty, tx, cy0, cy1, cx0, cx1;
} sgan_diffaug_rec;
typedef struct sgan_diffaug_job {
    const float* src;
    float* dst;
    int32_t H, W, C, Cs;
    uint32_t colour_mask;
} sgan_diffaug_job;
int64_t sgan_diffaug_workspace(int32_t njobs);
int sgan_diffaug_draw(sgan_diffaug_rec* params_dev, const int32_t* shapes, int32_t njobs, int32_t policy_bits, double rt, double rc,
                      uint64_t seed, uint64_t* offset_dev, int32_t advance, void* stream);
int sgan_diffaug_multi_fwd(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace, void* stream);
int sgan_diffaug_multi_bwd(const sgan_diffaug_job* jobs, int32_t njobs, const sgan_diffaug_rec* params_dev, void* workspace, void* stream);

/* ---- region statistics on the device (shape features of generated against real images: shape_stats.py) --------------------------
 * The reference's paper judges a generator by shape features of its cells and mitochondria; its repository holds only MATLAB that
 * loads precomputed features (experiments/plots).  These entries measure every region of a label map; util.region_table is the
 * NumPy / scipy restatement they are tested against, util.region_props derives the regionprops-style features from the rows.
 *
 * sgan_region_stats_workspace: bytes of the workspace sgan_region_stats needs for an H x W map (< 0: bad shape).
 * sgan_region_stats: appends one row of SGAN_REGION_COLS int64 per region of `labels` (a map in sgan_ccl_label's form: 0 = wall, else
 *   1 + the region's smallest raster index) to `table` (caller-owned, `capacity` rows), starting at row cursor[0].  cursor is 2 int32
 *   in device memory, {rows used, images done}, zeroed by the caller once.  Rows are in ascending order of the region's root raster
 *   index: row cursor[0] + k - 1 is region k of scipy.ndimage.label(free, structure=np.ones((3, 3))).  The call ends by adding the
 *   number of rows written to cursor[0] and 1 to cursor[1].  Columns, with x = column and y = row of a pixel, all exact:
 *      0      area in pixels
 *      1..4   xmin, xmax, ymin, ymax (inclusive)
 *      5..9   sum x, sum y, sum x^2, sum y^2, sum x y over the region's pixels
 *      10     boundary pixels: pixels of the region with at least one of their 4 neighbours not in it (outside the image: not in it)
 *      11     root raster index (label - 1)
 *      12     image ordinal (cursor[1] at entry)
 *      13     exposed edges: the (pixel, N/S/E/W) pairs whose neighbour is not in the region
 *      14,15  0
 *   If the regions do not all fit into `capacity`, the lowest-ranked ones that fit are written, cursor[0] becomes capacity, *dev_err
 *   gets bit 32 and the ordinal still advances.  A map that is not in sgan_ccl_label's form (a label outside 0 .. H W, a label whose
 *   root does not carry it, more roots than ceil(H / 2) ceil(W / 2)) gets bit 4 and the offending pixels are left out; no access
 *   leaves the buffers.
 *   Nothing is read back and nothing is decided on the host: five launches whose grids depend on (H, W) only -- root flags counted
 *   per block of 1024 pixels, one workgroup that scans the block counts and copies the cursor, the exclusive prefix sum over the
 *   flags (a region's dense rank) with each root initialising its own staging row, the counting pass, emit -- so the call can be
 *   captured in a hipGraph and replayed on maps with any other number of regions.  In the counting pass a workgroup holds 64 x 4
 *   pixels: a wave merges its 64 pixels by label (a segmented reduction: counts by ballot, the coordinate sums by one butterfly),
 *   the four waves merge in an LDS table, and the workgroup adds each region it met to the region's staging row once, in 64-bit
 *   integer atomics -- the same integers in any order.  The staging table lives in the workspace, indexed by dense rank, so
 *   initialisation does not depend on capacity.  Workspace, dev_err and stream as sgan_rand_f_accumulate; the call initialises what
 *   it uses.  H * W < 2^30 as sgan_ccl_label, and H, W <= 65536 so that the second-order sums stay below 2^62; both entries refuse
 *   any other shape.  Null pointers, capacity < 1 and a short workspace are refused before any launch. */
#define SGAN_REGION_COLS 16
int64_t sgan_region_stats_workspace(int32_t H, int32_t W);
int sgan_region_stats(const int32_t* labels, int32_t H, int32_t W, int64_t* table, int32_t capacity, int32_t* cursor, void* workspace,
                      int64_t workspace_bytes, int32_t* dev_err, void* stream);

/* ---- border weight: the per-pixel term of the U-Net loss (Ronneberger et al. 2015, eq. 2) on the device ---------------------------
 * w(p) = w_class[y_p] + w0 exp(-(d1(p) + d2(p))^2 / (2 sigma^2)), d1 and d2 the distances from p to the nearest and the second-nearest
 * cell: the term that makes a wall squeezed between two different cells expensive to miss.  The trainer's crops are cut, flipped and
 * rotated on the device, so the cells of a crop exist only there; util.border_weight_map is the NumPy restatement this is tested against.
 *
 * sgan_border_weight: `labels` is an H x W map in sgan_ccl_label's form (0 = wall, anything else = a cell id).  For a wall pixel p and
 *   a cell L let m_L(p) be the smallest dy^2 + dx^2 over the pixels of L inside the image with dy^2 + dx^2 <= radius^2.  d1sq(p) and
 *   d2sq(p) are the two smallest m_L(p) over DISTINCT L (equal when two cells are equally near), -1 where fewer than one / two cells
 *   are in range: exact integers, the same whichever order the pixels are met in.  bmap(p) = w0 expf(-(sqrtf(d1sq) + sqrtf(d2sq))^2 /
 *   (2 sigma^2)) where both exist, else 0.0f.  A pixel that is not wall gets bmap 0 and d1sq = d2sq = -1.  The cut at `radius` is part
 *   of the definition: with radius = ceil(4 sigma) the dropped terms are below w0 e^-8.  bmap is a dense float [H * W] plane, d1sq and
 *   d2sq are optional (NULL) int32 [H * W] planes.
 *   One launch, whose grid depends on (H, W) and whose LDS on radius only: a workgroup holds a 32 x 32 core and a radius-pixel halo of
 *   labels in LDS ((32 + 2 radius)^2 int32, 36 KB at radius 32; outside the image = wall) and every wall pixel of the core scans the disc,
 *   nearest rows first, until no further row can change its pair.  Nothing is read back, so the call captures into a hipGraph and
 *   replays on any other map.  A label < 0 is treated as wall and sets bit 4 of *dev_err (optional; as sgan_rand_f_accumulate's).
 *   Returns 1, having launched nothing, for NULL labels or bmap, H or W < 1, H * W >= 2^30, radius outside [1, 32] or sigma <= 0. */
int sgan_border_weight(const int32_t* labels, int32_t H, int32_t W, int32_t radius, float w0, float sigma, float* bmap, int32_t* d1sq,
                       int32_t* d2sq, int32_t* dev_err, void* stream);

/* ---- sliced Wasserstein distance between two image sets (generated against real images: swd.py) ------------------------------------
 * Karras et al. 2018 ("Progressive growing of GANs", section 5): per level of a Laplacian pyramid, N 7 x 7 patches of each set are
 * normalised per channel by the set's own mean and standard deviation, projected onto J unit directions, sorted, and compared;
 * the level's score is the mean over the directions of mean_i |sA_i - sB_i|.  util.lap_pyramid_ref, swd_descriptors_ref,
 * swd_normalise_ref and swd_ref are the NumPy restatements these entries are tested against.  Every entry only enqueues, uses no
 * atomic, sums in an order fixed by the launch shape (the same bits on every run), and refuses null pointers, short workspaces and
 * uncovered shapes before any launch (a negative status, the reason in sgan_last_error).
 *
 * sgan_lap_pyramid: one step on C planar float32 planes (plane c of a tensor starts c * rows * ld floats after plane 0; ld = the row
 *   pitch in floats).  `fine` is C x H x W, H and W even and >= 4.  The filter is g = outer(b, b), b = [1 4 6 4 1] / 16, and the border
 *   is mirrored without repeating the edge (d c b | a b c d | c b a, scipy's mode='mirror').
 *   mode SGAN_LAP_DOWN: out (C x H/2 x W/2) = the 5 x 5 correlation of `fine` with g at the even sites; `coarse` is not read.
 *   mode SGAN_LAP_UP_SUB: out (C x H x W) = fine - up, up = the correlation with 4 g of `coarse` (C x H/2 x W/2) placed on the even
 *   sites of a zero plane: a Laplacian level from a Gaussian level and the next one.  out is a buffer of its own.
 * sgan_swd_gather: copies the P 7 x 7 patches of one image's level (img: C x H x W planar with row pitch ld, C <= 3) whose top-left
 *   corners pos (int32 [P][3]: image, y, x as util.swd_draw gives them; the image column is not read) names into rows
 *   [row0, row0 + P) of desc (float32 [rows][C * 49], order [c][dy][dx]; rows <= 16384), exactly, and adds the image's per-channel
 *   sum and sum of squares of the copied values to acc (double [2 C]: C sums, then C sums of squares; zeroed by the caller once per
 *   set).  One workgroup owns a channel and the calls of a stream follow each other, so acc grows in image order.  A position outside
 *   [0, H - 7] x [0, W - 7] sets bit 128 of *dev_err (required; as the metric entries') and its row is zero-filled; nothing is read
 *   out of bounds.
 * sgan_swd_workspace: bytes of scratch sgan_swd_distances needs (< 0: a shape it does not cover).
 * sgan_swd_distances: out[j] (double [J]) = sum_i |sA_i - sB_i| / N for direction j of dirs (float32 [J][K]), sA and sB the sorted
 *   projections of the N rows of descA and descB (float32 [N][K]).  A value x of channel c is normalised on load as
 *   float32(float32(x - m32) * r32) with mean = sum / count, var = max(sumsq / count - mean^2, 0), m32 = float32(mean),
 *   r32 = float32(1 / sqrt(var)) or 0 where var is 0 (count = 49 N; statsA, statsB: double [2 C] in sgan_swd_gather's layout; every step
 *   rounded once in fp64, util.swd_stats_from_sums).  Projections are fp32 FMA chains over k; each direction's two projections are
 *   sorted by one bitonic network in LDS, padded with +inf to a power of two (2 x 64 KiB at N = 16384); the differences are summed in
 *   fp64.  Covered: 1 <= N <= 16384, K in {49, 98, 147}, 1 <= J <= 4096; anything else is refused.  variant SGAN_SWD_SPLIT: a
 *   projection pass writes [2][min(J, 512)][N] floats to the workspace and a sort pass (one workgroup per direction) reads them,
 *   512 directions at a time; SGAN_SWD_FUSED: the sort workgroups project their own rows and the workspace is not touched;
 *   SGAN_SWD_AUTO: the split form.  The workspace is 16-byte aligned and may hold anything on entry. */
#define SGAN_LAP_DOWN 0
#define SGAN_LAP_UP_SUB 1
#define SGAN_SWD_AUTO 0
#define SGAN_SWD_SPLIT 1
#define SGAN_SWD_FUSED 2
int sgan_lap_pyramid(int32_t mode, const float* fine, int64_t fine_ld, const float* coarse, int64_t coarse_ld, int32_t C, int32_t H,
                     int32_t W, float* out, int64_t out_ld, void* stream);
int sgan_swd_gather(const float* img, int64_t ld, int32_t C, int32_t H, int32_t W, const int32_t* pos, int32_t P, float* desc,
                    int32_t row0, int32_t rows, double* acc, int32_t* dev_err, void* stream);
int64_t sgan_swd_workspace(int32_t N, int32_t K, int32_t J);
int sgan_swd_distances(const float* descA, const float* descB, const double* statsA, const double* statsB, const float* dirs, int32_t N,
                       int32_t K, int32_t J, double* out, void* workspace, int64_t workspace_bytes, int32_t variant, void* stream);

/* ---- precision, recall, density, coverage of a generated set against a real one (swd.py --prd_k) --------------------------------------
 * Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) in the descriptor space of the
 * sliced Wasserstein score: balls around every row whose radius is the distance to its k-th nearest neighbour in its own set.  BOTH
 * sets are normalised by ONE set's statistics (the real set's), on load and exactly as sgan_swd_distances does it:
 * float32(float32(x - m32) * r32) from `stats` (double [2 C], sgan_swd_gather's layout) with count = 49 * the rows of the set the
 * statistics describe.  d2(x, y) is the squared Euclidean distance of two normalised rows.  util.knn_radii_ref, prd_rows_ref and
 * prd_scores_ref are the float64 NumPy yardsticks.  Every entry only enqueues, uses no atomic (a workgroup owns 64 query rows, walks
 * every reference column and finishes its rows itself: the same bits on every run), and refuses null pointers, short workspaces and
 * uncovered shapes before any launch (a negative status, the reason in sgan_last_error; no output is touched).
 * Covered: 1 <= N, Nq, Nr <= 16384, K in {49, 98, 147}, 1 <= k <= 8, group >= 1, k <= N - group.
 *
 * sgan_prd_workspace: bytes of scratch the two passes need for Nq query and Nr reference rows (< 0: a shape they do not cover);
 *   sgan_knn_radii takes sgan_prd_workspace(N, N, K).  16-byte aligned; it may hold anything on entry.
 * sgan_knn_radii: desc float32 [N][K]; count = 49 N.  Rows of one image follow each other, `group` rows each (the last group may be
 *   short), and the neighbours of row i exclude every row j with j / group == i / group; group = 1 excludes the row alone.
 *   rad[i] = the k-th smallest d2(x_i, x_j) over the admitted j (equal values each count), nn1[i] = the smallest.
 * sgan_prd_rows: descQ float32 [Nq][K], descR float32 [Nr][K], radR float32 [Nr]; count = 49 Nr (in swd.py both sets have N rows).
 *   cnt[i] = #{j : d2(q_i, r_j) <= radR[j]}, nn_d2[i] = min_j d2(q_i, r_j), nn_idx[i] = the smallest j that attains it.
 * variant: two forms of d2.  SGAN_PRD_DIRECT: diff = fl(q_k - r_k), then an FMA chain over k ascending; error per pair <=
 *   gamma_{K+2} d2 (gamma_n = n u / (1 - n u), u = 2^-24).  SGAN_PRD_GRAM: d2 = max(fl(n_q + n_r) - 2 q.r, 0) in one FMA, q.r by the
 *   exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the row norms n as fp32 FMA chains written to the workspace by a pre-pass; error per
 *   pair <= gamma_{K+3} (n_q + n_r + 2 sum_k |q_k r_k|).  On integer descriptors below 2^24 / K in square both are exact.
 *   SGAN_PRD_AUTO: the gram form, the faster one at N = 16384, K = 147.
 * sgan_prd_finish: out4 (int64 [4]) = #{cntB > 0} (precision hits), #{cntA > 0} (recall hits), sum cntB (density = / (k N)),
 *   #{nn_d2_A[i] <= radA[i]} (coverage hits: the nearest generated row of each real row against that row's own radius), from two
 *   sgan_prd_rows passes -- B against A with radA, A against B with radB -- of N rows each.  Exact integers; the caller divides. */
#define SGAN_PRD_AUTO 0
#define SGAN_PRD_DIRECT 1
#define SGAN_PRD_GRAM 2
int64_t sgan_prd_workspace(int32_t Nq, int32_t Nr, int32_t K);
int sgan_knn_radii(const float* desc, const double* stats, int32_t N, int32_t K, int32_t k, int32_t group, float* rad, float* nn1, void* ws,
                   int64_t ws_bytes, int32_t variant, void* stream);
int sgan_prd_rows(const float* descQ, const float* descR, const double* stats, const float* radR, int32_t Nq, int32_t Nr, int32_t K,
                  int32_t* cnt, float* nn_d2, int32_t* nn_idx, void* ws, int64_t ws_bytes, int32_t variant, void* stream);
int sgan_prd_finish(const int32_t* cntB, const int32_t* cntA, const float* nn_d2_A, const float* radA, int32_t N, int64_t* out4,
                    void* stream);

/* ---- soft-clDice: the differentiable centre-line Dice as a loss term (Shit et al., CVPR 2021; not in the reference) ----------------
 * The loss whose hard form the "topology scores" above report as clDice.  util.soft_cldice_ref is the NumPy fp64 restatement
 * (DESIGN.md R29).  On one plane X [H][W] of values in [0, 1]:
 *   erode(X)(y, x)  = min of X over the in-image pixels of the plus neighbourhood, taken in the order centre, up, left, right, down;
 *   dilate(X)(y, x) = max over the in-image pixels of the 3 x 3 box, centre first, then row-major;
 *   the gradient of a min or max goes entirely to the first pixel in that order that attains it.
 *   I_0 = X, I_{j+1} = erode(I_j) for j = 0 .. K;  delta_j = max(I_j - dilate(I_{j+1}), 0), derivative 0 at 0;
 *   S_0 = delta_0, S_j = S_{j-1} + delta_j (1 - S_{j-1});  the soft skeleton is S(X) = S_K.
 * With the probability plane P and the binary truth T:  A = sum S(P) T, B = sum S(P), C = sum S(T) P, D = sum S(T),
 *   Tprec = (A + 1) / (B + 1), Tsens = (C + 1) / (D + 1), L = 1 - 2 Tprec Tsens / (Tprec + Tsens).
 *
 * Planes: an input plane is read at x[y * rs + x * ps] (row and pixel stride in floats: a channel of an NHWC buffer, a window of a
 *   wider map); skeletons, dp and the planes of the workspace are dense [H * W].
 * sgan_cldice_workspace_bytes: bytes of the workspace for H x W and K = iters: the K + 2 planes I_j of sgan_soft_skeleton and, with
 *   with_backward != 0, the K + 3 planes more of sgan_cldice_backward (< 0: iters outside 1 .. 16 or a bad shape).  4-byte aligned;
 *   it may hold anything on entry.
 * sgan_soft_skeleton: I_0 .. I_{K+1} into the workspace (bits of the input: min rounds nothing) and S_K into skel.  K + 2 launches.
 * sgan_cldice_finish: sp = S(P), st = S(T).  The four sums in fp64, in an order fixed by the shape; state (double
 *   [SGAN_CLDICE_STATE_BYTES / 8], zeroed by the caller once, left ready for the next call) receives [0..3] A, B, C, D, [4] L,
 *   [5] gA, [6] gB with d L / d S(P)(x) = gA T(x) + gB, and [7] gC with the direct term d L / d P(x) = gC S(T)(x); loss_out = (float)L.
 *   One launch of at most 64 workgroups; the last to arrive finishes.
 * sgan_cldice_backward: dp = gout (gC S(T) + the gradient of sum_x (gA T(x) + gB) S(P)(x) through the skeleton chain), from the I_j
 *   sgan_soft_skeleton left in the SAME workspace and the state of sgan_cldice_finish; gout: a device float, null = 1.  The chain
 *   runs in reverse as gather launches: a pixel collects from the <= 9 dilate and <= 5 erode windows that contain it, each
 *   window's selection recomputed from I_j.  No atomics and no saved indices: the same bits on every run.  K + 3 launches.
 * Nothing is read back, nothing is allocated, every grid depends on (H, W) and the launch count on K alone: the calls capture into a
 * hipGraph.  Returns 1 ("not covered"), the reason in sgan_last_error and nothing launched, for iters outside 1 .. 16, a null
 * pointer, a shape outside H, W <= 32768 and H W < 2^30, a pixel stride < 1, a row stride below (W - 1) ps + 1 and a short or
 * misaligned workspace. */
#define SGAN_CLDICE_MAX_ITERS 16
#define SGAN_CLDICE_STATE_BYTES 4096
int64_t sgan_cldice_workspace_bytes(int32_t H, int32_t W, int32_t iters, int32_t with_backward);
int sgan_soft_skeleton(const float* x, int64_t x_rs, int64_t x_ps, int32_t H, int32_t W, int32_t iters, float* skel, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sgan_cldice_finish(const float* sp, const float* t, int64_t t_rs, int64_t t_ps, const float* st, const float* p, int64_t p_rs,
                       int64_t p_ps, int32_t H, int32_t W, double* state, float* loss_out, void* stream);
int sgan_cldice_backward(const float* t, int64_t t_rs, int64_t t_ps, const float* st, const double* state, const float* gout, int32_t H,
                         int32_t W, int32_t iters, float* dp, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Lovasz-softmax: the Lovasz extension of the Jaccard loss as a loss term (Berman, Triki, Blaschko, CVPR 2018; not in the
 * reference) ----  util.lovasz_ref is the NumPy fp64 restatement.  For every listed class c of the prediction
 * p [C][H][W] (fp32 in [0, 1], read at p[c * cs + y * rs + x * ps]: class, row and pixel stride in floats, so NCHW, a window of a
 * wider buffer or the channels of an NHWC buffer) against the index label [H][W] (int64, dense), N = H W:
 *   fg_i = (label_i == c), G = sum fg; a class with G = 0 is absent and takes no part ("classes = present");
 *   e_i = |fg_i - p_i(c)| in fp32; pi orders the pixels by e descending, ties by the pixel index i = y W + x ascending (a total
 *   order: the sort key ((0xFFFFFFFF - bits(e)) << 32) | (i << 1) | fg is unique);
 *   c_k = foreground among the first k + 1 sorted pixels, I_k = G - c_k, U_k = G + (k + 1 - c_k) in exact integers;
 *   g_k = 1 / U_k if sorted pixel k is foreground, else I_k / (U_k (U_k - 1)) (0 where I_k = 0): one fp64 division;
 *   L_c = sum_k e_pi(k) g_k in fp64, in an order fixed by the shape.
 * L = the mean of L_c over the m present listed classes, rounded to fp32 once; 0 if m = 0.
 * d L / d p_pi(k)(c) = gout * sign(p - fg) * g_k / m (sign(0) = 0), exactly 0 on absent and unlisted classes.
 *
 * The workspace (8-byte aligned; it may hold anything on entry), with P = max(4096, 2^ceil(log2 N)) and nb = ceil(N / 1024), in
 * this order: the state, SGAN_LOVASZ_STATE_BYTES: doubles [0] L, [1] m, [2 + j] L_c of the j-th listed class (0 if absent),
 * [10 + j] its scale 1 / m (0 if absent), and at byte 192 the int32 G of the listed classes; g, double [n][N], by sorted position;
 * the sorted keys, uint64 [n][P]; the block sums, double [n][nb]; pi, int32 [n][N] (the pixel index of sorted position k);
 * the block counts, int32 [n][nb]; rounded up to 8 bytes.
 * sgan_lovasz_workspace_bytes: its size (< 0, "not covered": H or W < 1, H W > 2^20, n outside 1 .. 8).
 * sgan_lovasz_forward: a bitonic sorting network on the keys (chunks of 4096 in LDS, the wider strides in global memory), an
 *   integer scan as count / offsets / apply launches, the weights and the ordered fp64 sums, the finish.  classes: n distinct class
 *   indices below C, on the HOST, read during the call.  loss_out: a device float.  The launches depend on (H, W, n) only.
 * sgan_lovasz_backward: dp [C][H][W], dense, from the workspace the forward left and the same p: every listed plane is scattered
 *   through pi (each pixel once), every other plane zeroed; gout: a device float, null = 1.  One launch.
 * No floating-point atomics, no workgroup waits on another, nothing is read back or allocated: the calls capture into a hipGraph and
 * give the same bits on every run.  Return 1, the reason in sgan_last_error and nothing launched, for "not covered" (as above), a
 * null pointer, classes that repeat or lie outside 0 .. C - 1 (C <= 64), a stride < 1 or rows that overlap, and a workspace that is
 * too small or misaligned. */
#define SGAN_LOVASZ_MAX_CLASSES 8
#define SGAN_LOVASZ_MAX_PIXELS (1 << 20)
#define SGAN_LOVASZ_STATE_BYTES 256
int64_t sgan_lovasz_workspace_bytes(int32_t H, int32_t W, int32_t n);
int sgan_lovasz_forward(const float* p, int64_t p_cs, int64_t p_rs, int64_t p_ps, const int64_t* label, const int32_t* classes, int32_t n,
                        int32_t C, int32_t H, int32_t W, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
int sgan_lovasz_backward(const float* p, int64_t p_cs, int64_t p_rs, int64_t p_ps, const int32_t* classes, int32_t n, int32_t C, int32_t H,
                         int32_t W, const float* gout, float* dp, const void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Segmentation loss terms: Tversky (soft Dice, focal-Tversky) and focal loss on the LOGITS (not in the reference) ----
 * util.seg_terms_ref is the NumPy fp64 restatement.  `logits` [npix][ld] fp32 with C <= 16 logical channels, read
 * where sgan_seg_head reads them; mode SGAN_SEGHEAD_SOFTMAX: `label_or_target` is the int64 label map, p = softmax(z), t_c = [y == c],
 * and a pixel whose label lies outside [0, C) adds to no sum and gets a zero gradient; SGAN_SEGHEAD_SIGMOID: the float target
 * [npix][tld] in [0, 1], p_c = sigmoid(z_c).
 *   Tversky over the n listed classes (`classes`: n distinct indices below C, on the HOST, read during the call; n = 0: term off):
 *     TP = sum p t, FP = sum p (1 - t), FN = sum (1 - p) t, in fp64 in an order fixed by npix;
 *     D = TP + alpha FP + beta FN + smooth, TI = (TP + smooth) / D, L_c = (1 - TI)^power, L_T = (1 / n) sum_c L_c;
 *     a class with D == 0 has L_c = 0 and no gradient; where 1 - TI == 0 the derivative is 0;
 *     G_c(t) = -(power / n) (1 - TI)^(power - 1) [t / D - (TP + smooth) (t (1 - beta) + alpha (1 - t)) / D^2];
 *     softmax: dz_k = p_k (G'_k - sum_j p_j G'_j), G'_j = G_j(t_j) on a listed channel, 0 elsewhere; sigmoid: dz_c = p_c (1 - p_c) G_c(t_c).
 *   Focal (`focal` != 0), class weights class_w (NULL: 1; softmax: nw >= C of them, sigmoid: the first nw <= C channels):
 *     softmax, pt = p_y, lp = z_y - logsumexp(z): L_F = sum w[y] (1 - pt)^gamma (-lp) / sum w[y],
 *       dz_k = w[y] / norm [gamma pt (1 - pt)^(gamma - 1) lp - (1 - pt)^gamma] (delta_ky - p_k), the first product left out where
 *       gamma == 0 or 1 - pt == 0; gamma = 0 is the class-weighted cross-entropy of sgan_seg_head;
 *     sigmoid: L_F = sum_{p, c} w_c [t (1 - p)^gamma softplus(-z) + (1 - t) p^gamma softplus(z)] / (C npix), dz its derivative.
 * sgan_seg_terms_forward: one launch.  Writes the state (SGAN_SEGTERMS_STATE_BYTES, doubles: [8 j + 0 .. 7] TP, FP, FN, D, TI, L_c,
 *   G_c(0), G_c(1) of the j-th listed class, zeros behind the n-th; [64] the focal numerator, [65] its norm, [66] L_T, [67] L_F) and
 *   both losses as device floats (0 for a term that is off).  `workspace`: SGAN_SEGTERMS_WS_BYTES of 8-byte aligned device scratch,
 *   ZERO on first use, owned by one stream at a time and left zeroed by every call.
 * sgan_seg_terms_backward: one launch, from the state the forward left and the same logits and label: dlogits [npix][dld] =
 *   gout_tversky * dL_T/dz + gout_focal * dL_F/dz, the upstream gradients device floats, NULL = that term is not taken; the padding
 *   channels dld > C are written as zeros.
 * The grid depends on npix only; no floating-point atomics, no workgroup waits on another, nothing is read back or allocated: both
 * calls capture into a hipGraph and give the same bits on every run.  Return 1, the reason in sgan_last_error and nothing launched:
 * C > 16, n outside 0 .. 8, both terms off, a listed class >= C or repeated, parameters outside alpha, beta >= 0, alpha + beta > 0,
 * smooth >= 0, 0 < power <= 4, 0 <= gamma <= 8, a NULL required pointer, rows shorter than C. */
#define SGAN_SEGTERMS_MAX_CLASSES 8
#define SGAN_SEGTERMS_STATE_BYTES 544
#define SGAN_SEGTERMS_WS_BYTES 106504
int sgan_seg_terms_forward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                           const int32_t* classes, int32_t n, double alpha, double beta, double smooth, double power, int32_t focal,
                           double gamma, const float* class_w, int32_t nw, double* state, float* loss_tversky, float* loss_focal,
                           void* workspace, void* stream);
int sgan_seg_terms_backward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                            const int32_t* classes, int32_t n, int32_t focal, double gamma, const float* class_w, int32_t nw,
                            const double* state, const float* gout_tversky, const float* gout_focal, float* dlogits, int32_t dld,
                            void* stream);

/* ---- Distance-map loss terms: boundary loss and Hausdorff loss of one class on the LOGITS (not in the reference) ----
 * What the boundary scores (BoundF, HausD, ASSD) rank, as a loss: the boundary loss of Kervadec et al. (MIDL 2019) and the
 * distance-transform Hausdorff loss HD_DT of Karimi & Salcudean (TMI 2019).  util.signed_edt_sq and util.dist_terms_ref are the NumPy
 * restatements.
 *
 * sgan_signed_edt_workspace: bytes of the workspace sgan_signed_edt_sq needs for an H x W plane (< 0: bad shape).
 * sgan_signed_edt_sq: the signed squared Euclidean distance map.  The plane is read exactly as sgan_edt_sq reads it, pixel (y, x) at
 *   plane[(y * W + x) * pix_stride]; a pixel is inside when its value is > 0.5 (a NaN and an exact 0.5 are outside).
 *   sdsq, int32 [H * W], exact: on an outside pixel +(the smallest dy^2 + dx^2 to an inside pixel), >= 1; on an inside pixel -(the
 *   smallest dy^2 + dx^2 to an outside pixel), <= -1; 0 everywhere when the plane has no inside pixel or no outside pixel, decided on
 *   the device from sgan_edt_sq's -1, nothing read back.  sgan_edt_sq of the plane into sdsq, a pass that writes the complement plane,
 *   sgan_edt_sq of that, a pass that combines the two: ten launches whose grids depend on (H, W) only, so the call captures into a
 *   hipGraph, replays on any other plane and gives the same bits on every run.  The workspace may hold anything on entry.  Shapes
 *   as sgan_edt_sq: H, W <= 32768 and H W < 2^30.  dev_err as sgan_edt_sq: required, no bit set.  A null pointer, a bad shape, a
 *   pixel stride < 1 and a short or misaligned (16 bytes) workspace return 1 with sgan_last_error set and nothing launched.
 *
 * The loss node.  `logits`, ld, npix, C, mode, `label_or_target` and tld as sgan_seg_terms_forward takes them (C <= 16 logical
 *   channels; SGAN_SEGHEAD_SOFTMAX: the int64 label map, SGAN_SEGHEAD_SIGMOID: the float target [npix][tld]).  One class `cls` < C:
 *   p = softmax(z)_cls or sigmoid(z_cls), computed in registers; g = [y == cls] or target_cls; N = npix.  A pixel whose label lies
 *   outside [0, C) adds to no sum and gets a zero gradient.  t_sdsq, p_sdsq: int32 [npix], the signed maps (sgan_signed_edt_sq) of
 *   the truth and of the thresholded prediction, both constants of the node; p_sdsq may be NULL when the Hausdorff term is off.
 *   Boundary (`boundary` != 0), s = t_sdsq: phi = sqrt(s) where s > 0, -(sqrt(-s) - 1) where s < 0, 0 where s == 0 (Kervadec's
 *     published level set);  L_B = sum phi p / N;  dL_B/dp = phi / N.
 *   Hausdorff (`hausdorff` != 0), 0 < alpha <= 4: F = |t_sdsq|^(alpha / 2) + |p_sdsq|^(alpha / 2), at alpha == 2 the exact integer
 *     |t_sdsq| + |p_sdsq| without a pow;  L_H = sum (p - g)^2 F / N;  dL_H/dp = 2 (p - g) F / N.
 *   To the logits, G = gout_boundary dL_B/dp + gout_hausdorff dL_H/dp: softmax dz_k = G p (delta_k,cls - p_k); sigmoid
 *     dz_cls = G p (1 - p), every other channel 0.  p in fp32, the terms and G in fp64, G rounded once, dz in fp32.
 * sgan_dist_loss_forward: one launch.  Writes the state (SGAN_DISTLOSS_STATE_BYTES, doubles: [0] sum phi p, [1] sum (p - g)^2 F,
 *   [2] N, [3] L_B, [4] L_H; [5 .. 7] not written; a sum of a term that is off is 0) and both losses as device floats (0 for a term
 *   that is off).  The fp64 sums are taken in an order fixed by npix.  `workspace`: SGAN_DISTLOSS_WS_BYTES of 8-byte aligned device
 *   scratch, ZERO on first use, owned by one stream at a time and left zeroed by every call.
 * sgan_dist_loss_backward: one launch, from the same logits, label and maps: dlogits [npix][dld] as above, the upstream gradients
 *   device floats, NULL = that term is not taken; the padding channels dld > C are written as zeros.
 * The grid depends on npix only; no floating-point atomics, no workgroup waits on another, nothing is read back or allocated: both
 * calls capture into a hipGraph and give the same bits on every run and in every row layout.  Return 1, the reason in
 * sgan_last_error and nothing launched: C > 16, cls outside [0, C), both terms off, alpha outside (0, 4] with the Hausdorff term on,
 * a NULL required pointer (p_sdsq with the Hausdorff term on), rows shorter than C, a misaligned state or workspace. */
#define SGAN_DISTLOSS_STATE_BYTES 64
#define SGAN_DISTLOSS_WS_BYTES 8200
int64_t sgan_signed_edt_workspace(int32_t H, int32_t W);
int sgan_signed_edt_sq(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* sdsq, void* workspace,
                       int64_t workspace_bytes, int32_t* dev_err, void* stream);
int sgan_dist_loss_forward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                           int32_t cls, const int32_t* t_sdsq, const int32_t* p_sdsq, int32_t boundary, int32_t hausdorff, double alpha,
                           double* state, float* loss_boundary, float* loss_hausdorff, void* workspace, void* stream);
int sgan_dist_loss_backward(const float* logits, int32_t ld, int32_t npix, int32_t C, int32_t mode, const void* label_or_target, int32_t tld,
                            int32_t cls, const int32_t* t_sdsq, const int32_t* p_sdsq, int32_t boundary, int32_t hausdorff, double alpha,
                            const float* gout_boundary, const float* gout_hausdorff, float* dlogits, int32_t dld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGAN_HIP_H */
