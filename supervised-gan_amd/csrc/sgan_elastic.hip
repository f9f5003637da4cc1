// Elastic deformation of a training crop, fused into the tail of the input pipeline (include/sgan_hip.h, "elastic input pipeline
// tail"): sgan_image_prep with the address it gathers from displaced by a smooth random field.  (G + 3)^2 control vectors on a
// coarse grid over the crop, interpolated per pixel by the Catmull-Rom tensor product in fp32, clamped to +-127 source pixels and
// quantised to 1/256 pixel; from there on integers only: image channels are sampled bilinearly in 8.8 fixed point, label channels
// at the nearest pixel (a label stays a label), every index mirrored into the image.  util.elastic_field / util.elastic_prep are the
// NumPy restatement this is tested against.
//
// One thread per output pixel, one launch per item.  The control vectors (at most 256 (dx, dy) pairs, 2 KB) are staged in LDS once
// per workgroup; a wave covers 64 consecutive output pixels, which lie in one or two cells, so the 16 8-byte LDS reads of a thread
// are broadcasts.  The eight Catmull-Rom weights, the four bilinear weights and the mirrored addresses are computed once per thread
// and shared by the channels.  With Cstore == 4 a pixel leaves as one 16-byte store.
//
// The weights are written so that none of them is a difference of rounded quantities.  With t = rem / n and s = (n - rem) / n (TWO
// correctly rounded divisions of exact integers: 1 - t formed in fp32 would carry t's rounding relative to 1, not to 1 - t):
//     w0 = -t s^2 / 2,   w1 = s (s^2 + 3 s t + t^2 / 2),   w2 = t (t^2 + 3 s t + s^2 / 2),   w3 = -t^2 s / 2
// (the quadratics are the Bernstein form of 1 + t - 1.5 t^2 and of its mirror image: every term is positive).  A weight therefore
// carries at most 8 roundings relative to ITSELF, and the field, summed row by row, at most 24 relative to sum |w_r w_s c_rs|
// (tests/test_hip_elastic.py counts them).
#include "sgan_common.h"

#define SG_EL_MAX_G 13
#define SG_EL_MAX_DIM (1 << 22)      // H0, W0: (x0 + u) * 256 + q and u * G stay far inside int32, (float)n is exact
#define SG_EL_CLAMP 127.f

// i folded into [0, N) by reflection about the first and the last pixel, neither repeated: period P = 2 (N - 1), any number of folds
__device__ __forceinline__ int sg_el_mirror(int i, int N, int P) {
    if (N == 1) return 0;
    int m = i % P;
    if (m < 0) m += P;
    return m < N ? m : P - m;
}

// Catmull-Rom (a = -0.5) weights of the four control points around a cell at the fractional position rem / n, 0 <= rem < n
__device__ __forceinline__ void sg_el_weights(int rem, int n, float w[4]) {
    const float t = (float)rem / (float)n, s = (float)(n - rem) / (float)n;
    const float ss = s * s, st = s * t, tt = t * t;
    w[0] = (-0.5f * t) * ss;
    w[1] = s * ((ss + 3.f * st) + 0.5f * tt);
    w[2] = t * ((tt + 3.f * st) + 0.5f * ss);
    w[3] = (-0.5f * tt) * s;
}

__device__ __forceinline__ float sg_el_normalize(unsigned p) {
    float v = (float)p / 255.f;      // ToTensor
    return (v - 0.5f) / 0.5f;        // Normalize((.5,.5,.5), (.5,.5,.5)): the expressions of sg_image_prep_kernel
}

template <bool VEC4>
__global__ __launch_bounds__(256) void sg_image_prep_elastic_kernel(const unsigned char* __restrict__ img, int H0, int W0, int x0, int y0, int n,
                                                                    int flip, int rot, const float* __restrict__ ctrl, int G, int nearest_mask,
                                                                    float* __restrict__ dst, int dst_ld, int Cstore, float* __restrict__ field_out) {
    __shared__ f32x2 cp[(SG_EL_MAX_G + 3) * (SG_EL_MAX_G + 3)];      // (dx, dy) of control point (r, s) at r * GP + s
    const int GP = G + 3;
    for (int p = threadIdx.x; p < GP * GP; p += 256) cp[p] = f32x2{ctrl[2 * p], ctrl[2 * p + 1]};
    SG_SYNC();      // nothing writes cp after this

    const int PW = 2 * (W0 - 1), PH = 2 * (H0 - 1);
    const int64_t total = (int64_t)n * n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % n), i = (int)(e / n);
        int a = i, b = j;      // output (i, j) shows crop pixel (a, b): the mapping of sg_image_prep_kernel
        if (rot == 1) { a = j; b = n - 1 - i; }
        else if (rot == 2) { a = n - 1 - i; b = n - 1 - j; }
        else if (rot == 3) { a = n - 1 - j; b = i; }
        if (flip) b = n - 1 - b;

        // the field at crop coordinate (u, v) = (b, a): cell and fractional position in integers
        const int au = b * G, av = a * G;
        const int cu = au / n, cv = av / n;
        float wx[4], wy[4];
        sg_el_weights(au - cu * n, n, wx);
        sg_el_weights(av - cv * n, n, wy);
        float dx = 0.f, dy = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2* row = cp + (cv + k) * GP + cu;
            float rx = wx[0] * row[0].x, ry = wx[0] * row[0].y;
#pragma unroll
            for (int m = 1; m < 4; ++m) {
                rx += wx[m] * row[m].x;
                ry += wx[m] * row[m].y;
            }
            dx = k ? dx + wy[k] * rx : wy[0] * rx;
            dy = k ? dy + wy[k] * ry : wy[0] * ry;
        }
        dx = fminf(fmaxf(dx, -SG_EL_CLAMP), SG_EL_CLAMP);      // also what a NaN control value ends as: the addresses stay bounded
        dy = fminf(fmaxf(dy, -SG_EL_CLAMP), SG_EL_CLAMP);
        if (field_out) {
            float* f = field_out + ((int64_t)a * n + b) * 2;
            f[0] = dx;
            f[1] = dy;
        }

        // 8.8 fixed-point source position; integers from here on
        const int X = (x0 + b) * 256 + (int)rintf(dx * 256.f), Y = (y0 + a) * 256 + (int)rintf(dy * 256.f);
        unsigned pv[3] = {0u, 0u, 0u};
        if ((nearest_mask & 7) != 7) {
            const int ix = X >> 8, iy = Y >> 8, fx = X & 255, fy = Y & 255;
            const int64_t ra = (int64_t)sg_el_mirror(iy, H0, PH) * W0, rb = (int64_t)sg_el_mirror(iy + 1, H0, PH) * W0;
            const int xa = sg_el_mirror(ix, W0, PW), xb = sg_el_mirror(ix + 1, W0, PW);
            const unsigned char *p00 = img + (ra + xa) * 3, *p01 = img + (ra + xb) * 3, *p10 = img + (rb + xa) * 3, *p11 = img + (rb + xb) * 3;
            const int w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (!((nearest_mask >> c) & 1)) pv[c] = (unsigned)(w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 32768) >> 16;
        }
        if (nearest_mask & 7) {
            const unsigned char* pn = img + ((int64_t)sg_el_mirror((Y + 128) >> 8, H0, PH) * W0 + sg_el_mirror((X + 128) >> 8, W0, PW)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if ((nearest_mask >> c) & 1) pv[c] = pn[c];
        }

        float* o = dst + e * dst_ld;
        if (VEC4) {
            *(f32x4*)o = f32x4{sg_el_normalize(pv[0]), sg_el_normalize(pv[1]), sg_el_normalize(pv[2]), 0.f};
        } else {
            for (int c = 0; c < Cstore; ++c) o[c] = c < 3 ? sg_el_normalize(pv[c]) : 0.f;
        }
    }
}

extern "C" int sgan_image_prep_elastic(const unsigned char* img, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t n, int32_t flip,
                                       int32_t rot, const float* ctrl, int32_t G, int32_t nearest_mask, float* dst, int32_t dst_ld,
                                       int32_t Cstore, float* field_out, void* stream) {
    SGAN_CHECK(img && dst && H0 > 0 && W0 > 0 && n > 0, "bad argument");
    SGAN_CHECK(H0 <= SG_EL_MAX_DIM && W0 <= SG_EL_MAX_DIM, "image %d x %d: at most %d pixels a side", W0, H0, SG_EL_MAX_DIM);
    SGAN_CHECK(x0 >= 0 && y0 >= 0 && x0 + n <= W0 && y0 + n <= H0, "crop window %d+%d x %d+%d outside the %d x %d image", x0, n, y0, n, W0, H0);
    SGAN_CHECK(rot >= 0 && rot <= 3 && Cstore >= 3 && dst_ld >= Cstore, "bad rot / channel count");
    SGAN_CHECK(ctrl && G >= 1 && G <= SG_EL_MAX_G, "elastic grid: G = %d (1..%d) cells a side and a control array", G, SG_EL_MAX_G);
    const int64_t want = ((int64_t)n * n + 255) / 256;
    const int blocks = want > 4096 ? 4096 : (int)want;
    const bool vec4 = Cstore == 4 && dst_ld % 4 == 0 && ((uintptr_t)dst & 15) == 0;      // one 16-byte store per pixel
    if (vec4)
        hipLaunchKernelGGL(sg_image_prep_elastic_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, H0, W0, x0, y0, n,
                           flip != 0, rot, ctrl, G, nearest_mask, dst, dst_ld, Cstore, field_out);
    else
        hipLaunchKernelGGL(sg_image_prep_elastic_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, H0, W0, x0, y0, n,
                           flip != 0, rot, ctrl, G, nearest_mask, dst, dst_ld, Cstore, field_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_image_prep_elastic_kernel";
    return SGAN_OK;
}
