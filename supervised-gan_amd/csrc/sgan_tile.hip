// Whole-image inference (include/sgan_hip.h, "whole-image inference"): the data movement around the forward passes of
// the overlap-tile strategy with D4 averaging.  Three streaming kernels, one launch per stage, no LDS, no atomics:
//
//   prep    sgan_image_prep with reflected borders and rectangular windows: one thread per OUTPUT pixel, one 16-byte store each; the
//           three bytes it gathers come from the window pixel the D4 element maps it to, mirrored into the image.
//   blend   canvas[Y][X][c] += w(a) w(b) p_c, one thread per CANVAS pixel of the tile's non-zero window inside the image: a 16-byte
//           load and store of the canvas row, and a 16-byte gather of the logits at the tile pixel (i, j) that shows (Y, X).  A D4
//           element is a bijection of the tile, so within a launch a canvas pixel has one writer; launches are ordered by the stream,
//           so the sum has one order and the same bits on every run.  Under a rotation consecutive canvas pixels read logits T
//           pixels apart (the gather strides, the stores do not).
//   finish  P = canvas / (float)(n_tta Wy[Y] Wx[X]) and log max(P, FLT_MIN), 16 bytes in, two 16-byte stores out.
//
// The softmax and the sigmoid are the expressions of sgan_softmax_fwd (sg_ce_lse, sgan_ew.hip) and sgan_sigmoid_nhwc_fwd (sg_sigmoid),
// operation for operation: a plan of one tile with weight 1 returns their bits.
#include <float.h>

#include "sgan_reduce.h"

#define SG_TILE_MAXC 4
#define SG_TILE_MAX_RAMP 64
#define SG_TILE_MAX_DIM (1 << 22)      // image side: every index and every weight sum below stays far inside 32 bits

// index i of the padded domain -> the image, mirrored without repeating the edge; one fold is enough for -(L - 1) <= i <= 2 (L - 1)
__device__ __forceinline__ int sg_tile_reflect(int i, int L) {
    if (i < 0) i = -i;
    return i >= L ? 2 * (L - 1) - i : i;
}

// w(i) = clamp(min(i + 1, T - i) - M, 0, R)
__device__ __forceinline__ int sg_tile_window(int i, int T, int M, int R) {
    const int d = min(i + 1, T - i) - M;
    return d < 0 ? 0 : d > R ? R : d;
}

__global__ __launch_bounds__(256) void sg_image_prep_tile_kernel(const unsigned char* img, int H0, int W0, int x0, int y0, int h, int w,
                                                                 int flip, int rot, float* dst, int dst_ld, int Cstore, int vec) {
    const int64_t total = (int64_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % w), i = (int)(e / w);
        // sg_image_prep_kernel's mapping (rot != 0 only with h == w): R[i][j] = F[j][n-1-i] (rot 1), F[n-1-i][n-1-j] (2), F[n-1-j][i] (3)
        int a = i, b = j;
        if (rot == 1) { a = j; b = w - 1 - i; }
        else if (rot == 2) { a = h - 1 - i; b = w - 1 - j; }
        else if (rot == 3) { a = h - 1 - j; b = i; }
        if (flip) b = w - 1 - b;
        const unsigned char* px = img + ((int64_t)sg_tile_reflect(y0 + a, H0) * W0 + sg_tile_reflect(x0 + b, W0)) * 3;
        float v[3];
        for (int c = 0; c < 3; ++c) {
            v[c] = (float)px[c] / 255.f;            // ToTensor
            v[c] = (v[c] - 0.5f) / 0.5f;            // Normalize((.5,.5,.5), (.5,.5,.5)), sgan_image_prep's operation order: the same bits
        }
        float* o = dst + e * dst_ld;
        if (vec) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], 0.f};
        } else {
            for (int c = 0; c < Cstore; ++c) o[c] = c < 3 ? v[c] : 0.f;
        }
    }
}

extern "C" int sgan_image_prep_tile(const unsigned char* img, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t h, int32_t w,
                                    int32_t flip, int32_t rot, float* dst, int32_t dst_ld, int32_t Cstore, void* stream) {
    SGAN_CHECK(img && dst && H0 > 0 && W0 > 0 && h > 0 && w > 0, "bad argument");
    SGAN_CHECK(H0 <= SG_TILE_MAX_DIM && W0 <= SG_TILE_MAX_DIM && h <= SG_TILE_MAX_DIM && w <= SG_TILE_MAX_DIM, "a side above 2^22");
    SGAN_CHECK(x0 > -W0 && y0 > -H0 && (int64_t)x0 + w <= 2 * (int64_t)W0 - 1 && (int64_t)y0 + h <= 2 * (int64_t)H0 - 1,
               "window %d+%d x %d+%d reaches more than %d x %d - 1 pixels outside the image: one reflection cannot fold it back", x0, w, y0, h,
               W0, H0);
    SGAN_CHECK(rot >= 0 && rot <= 3 && Cstore >= 3 && dst_ld >= Cstore, "bad rot / channel count");
    SGAN_CHECK(rot == 0 || h == w, "a %d x %d window cannot be rotated (rot %d): rectangular windows take rot 0", h, w, rot);
    const int vec = Cstore == 4 && (dst_ld & 3) == 0 && ((uintptr_t)dst & 15) == 0;
    int blocks = sg_cdiv((int64_t)h * w, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sg_image_prep_tile_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, H0, W0, x0, y0, h, w, flip != 0, rot,
                       dst, dst_ld, Cstore, vec);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

// the canvas rectangle [Y0, Y0 + nY) x [X0, X0 + nX) is the tile's non-margin part inside the image
__global__ __launch_bounds__(256) void sg_tile_blend_kernel(const float* logits, int ld, int C, int mode, int x0, int y0, int T, int M, int R,
                                                            int flip, int rot, float* canvas, int canvas_ld, int W, int Y0, int X0, int nY,
                                                            int nX) {
    const int64_t total = (int64_t)nY * nX;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int Y = Y0 + (int)(e / nX), X = X0 + (int)(e % nX);
        const int a = Y - y0, b = X - x0;                      // window coordinates, before flip and rotation
        const int wgt = sg_tile_window(a, T, M, R) * sg_tile_window(b, T, M, R);
        if (wgt == 0) continue;
        // the tile pixel (i, j) that sg_image_prep_tile_kernel filled from (a, b): its mapping, inverted
        const int bf = flip ? T - 1 - b : b;
        int i = a, j = bf;
        if (rot == 1) { i = T - 1 - bf; j = a; }
        else if (rot == 2) { i = T - 1 - a; j = T - 1 - bf; }
        else if (rot == 3) { i = bf; j = T - 1 - a; }
        const f32x4 z4 = *reinterpret_cast<const f32x4*>(logits + ((int64_t)i * T + j) * ld);
        const float z[SG_TILE_MAXC] = {z4.x, z4.y, z4.z, z4.w};
        float p[SG_TILE_MAXC] = {0.f, 0.f, 0.f, 0.f};
        if (mode == SGAN_SEGHEAD_SOFTMAX) {                    // sg_ce_lse + sg_softmax_fwd_kernel
            float m = -3.4e38f;
            for (int c = 0; c < SG_TILE_MAXC; ++c)
                if (c < C) m = fmaxf(m, z[c]);
            float sum = 0.f;
            for (int c = 0; c < SG_TILE_MAXC; ++c)
                if (c < C) sum += expf(z[c] - m);
            const float lse = m + logf(sum);
            for (int c = 0; c < SG_TILE_MAXC; ++c)
                if (c < C) p[c] = expf(z[c] - lse);
        } else {
            for (int c = 0; c < SG_TILE_MAXC; ++c)
                if (c < C) p[c] = sg_sigmoid(z[c]);
        }
        f32x4* o = reinterpret_cast<f32x4*>(canvas + ((int64_t)Y * W + X) * canvas_ld);
        f32x4 acc = *o;
        const float wf = (float)wgt;                           // at most 64^2: exact
        acc.x = fmaf(wf, p[0], acc.x);
        acc.y = fmaf(wf, p[1], acc.y);
        acc.z = fmaf(wf, p[2], acc.z);
        acc.w = fmaf(wf, p[3], acc.w);
        *o = acc;
    }
}

extern "C" int sgan_tile_blend(const float* logits, int32_t ld, int32_t C, int32_t mode, int32_t x0, int32_t y0, int32_t T, int32_t M,
                               int32_t R, int32_t flip, int32_t rot, float* canvas, int32_t canvas_ld, int32_t H, int32_t W, void* stream) {
    SGAN_CHECK(logits && canvas && H > 0 && W > 0 && H <= SG_TILE_MAX_DIM && W <= SG_TILE_MAX_DIM, "bad argument");
    SGAN_CHECK(C >= 1 && C <= SG_TILE_MAXC && (mode == SGAN_SEGHEAD_SOFTMAX || mode == SGAN_SEGHEAD_SIGMOID), "1..%d channels, softmax or sigmoid",
               SG_TILE_MAXC);
    SGAN_CHECK(ld >= 4 && (ld & 3) == 0 && canvas_ld >= 4 && (canvas_ld & 3) == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)canvas & 15) == 0,
               "logits and canvas are padded NHWC: pixel strides a multiple of 4 floats, 16-byte aligned");
    SGAN_CHECK(T >= 1 && T <= SG_TILE_MAX_DIM && M >= 0 && 2 * (int64_t)M < T && R >= 1 && R <= SG_TILE_MAX_RAMP && rot >= 0 && rot <= 3,
               "tile %d, margin %d, ramp %d (1..%d), rot %d", T, M, R, SG_TILE_MAX_RAMP, rot);
    SGAN_CHECK(M <= H - 1 && M <= W - 1 && T <= (int64_t)H + 2 * M && T <= (int64_t)W + 2 * M, "tile %d with margin %d does not fit the %d x %d image", T,
               M, H, W);
    SGAN_CHECK(x0 >= -M && y0 >= -M && (int64_t)x0 + T <= (int64_t)W + M && (int64_t)y0 + T <= (int64_t)H + M,
               "tile origin (%d, %d) outside the padded domain", x0, y0);
    // rows / columns of the window with a non-zero weight, cut to the image: never empty (2 M < T, and the origin bounds above)
    const int Ya = max(0, y0 + M), Yb = min(H, y0 + T - M), Xa = max(0, x0 + M), Xb = min(W, x0 + T - M);
    SGAN_CHECK(Yb > Ya && Xb > Xa, "empty tile");
    int blocks = sg_cdiv((int64_t)(Yb - Ya) * (Xb - Xa), 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sg_tile_blend_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, ld, C, mode, x0, y0, T, M, R, flip != 0, rot,
                       canvas, canvas_ld, W, Ya, Xa, Yb - Ya, Xb - Xa);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

__global__ __launch_bounds__(256) void sg_tile_finish_kernel(const float* canvas, int canvas_ld, int H, int W, int C, const int32_t* Wy,
                                                             const int32_t* Wx, int n_tta, float* prob, int prob_ld, float* logp, int logp_ld) {
    const int64_t total = (int64_t)H * W;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int Y = (int)(e / W), X = (int)(e % W);
        const int64_t wsum = (int64_t)n_tta * Wy[Y] * Wx[X];      // util.tile_plan keeps it below 2^24: the conversion is exact
        const float den = (float)wsum;
        const f32x4 s = *reinterpret_cast<const f32x4*>(canvas + e * canvas_ld);
        const float sv[SG_TILE_MAXC] = {s.x, s.y, s.z, s.w};
        float p[SG_TILE_MAXC], l[SG_TILE_MAXC];
        for (int c = 0; c < SG_TILE_MAXC; ++c) {
            const bool on = c < C && wsum > 0;                     // a pixel no tile covers (a wrong plan) reads 0, not NaN
            p[c] = on ? sv[c] / den : 0.f;
            l[c] = c < C ? logf(fmaxf(p[c], FLT_MIN)) : 0.f;
        }
        *reinterpret_cast<f32x4*>(prob + e * prob_ld) = f32x4{p[0], p[1], p[2], p[3]};
        *reinterpret_cast<f32x4*>(logp + e * logp_ld) = f32x4{l[0], l[1], l[2], l[3]};
    }
}

extern "C" int sgan_tile_finish(const float* canvas, int32_t canvas_ld, int32_t H, int32_t W, int32_t C, const int32_t* Wy, const int32_t* Wx,
                                int32_t n_tta, float* prob, int32_t prob_ld, float* logp, int32_t logp_ld, void* stream) {
    SGAN_CHECK(canvas && Wy && Wx && prob && logp && H > 0 && W > 0 && H <= SG_TILE_MAX_DIM && W <= SG_TILE_MAX_DIM, "bad argument");
    SGAN_CHECK(C >= 1 && C <= SG_TILE_MAXC && (n_tta == 1 || n_tta == 8), "1..%d channels, 1 or 8 passes per tile", SG_TILE_MAXC);
    SGAN_CHECK(canvas_ld >= 4 && (canvas_ld & 3) == 0 && prob_ld >= 4 && (prob_ld & 3) == 0 && logp_ld >= 4 && (logp_ld & 3) == 0 &&
                   (((uintptr_t)canvas | (uintptr_t)prob | (uintptr_t)logp) & 15) == 0 && (((uintptr_t)Wy | (uintptr_t)Wx) & 3) == 0,
               "canvas, prob and logp are padded NHWC: pixel strides a multiple of 4 floats, 16-byte aligned");
    int blocks = sg_cdiv((int64_t)H * W, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sg_tile_finish_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, canvas, canvas_ld, H, W, C, Wy, Wx, n_tta, prob,
                       prob_ld, logp, logp_ld);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}
