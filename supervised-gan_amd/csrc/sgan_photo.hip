// Photometric augmentation of a prepared training crop (include/sgan_hip.h, "photometric augmentation of a prepared crop"): blur,
// gamma, contrast / brightness, additive noise, clamp and occlusion boxes on the image channels of a padded NHWC fp32 crop, out of
// place; every other channel is copied bit for bit.  The host draws the parameters (util.photo_draw) and the noise comes in as a buffer
// (sgan_normal_fill): the kernel holds no random number generator.  util.photo_ref / util.photo_bounds are the NumPy restatement this is
// tested against (DESIGN.md R38 counts the roundings).
//
// One workgroup of 256 threads per 32 x 32 output tile (a grid-stride walk over the tiles when there are more than the grid holds).
// With R > 0 the tile and its R-pixel halo of up to SG_PH_PLANES masked channels are staged in LDS once, every index mirrored into the
// crop; the row pass runs over the (32 + 2 R) staged rows into a second LDS buffer, the column pass and the point stages run from there.
// A thread owns the four pixels (ly + 8 k, lx) of the tile: in both passes the 32 lanes of a half-wave read 32 consecutive floats of
// one LDS row, so neither pass has a bank conflict whatever the row pitch (ds_read_b32 is served per 32-lane half).  The taps are
// wave-uniform kernel arguments read with constant indices (the tap loop is unrolled to SGAN_PHOTO_MAX_R and left early), so they
// stay in scalar registers.  With R == 0 no LDS is used and no barrier is met.
//
// VEC4 (Cstore == 4, strides multiples of 4, 16-byte aligned pointers, at most SG_PH_PLANES masked channels): a pixel is one 16-byte
// load -- the tile's own pixels by their owner, who keeps them for the channels that are only copied -- and one 16-byte store.  The
// scalar path reads a masked channel when it stages it (or, with R == 0, where it is used) and an unmasked one where it is copied, in
// groups of SG_PH_PLANES masked channels.  So a source element is read once per tile that needs it; a pixel that the mirror brings in
// a second time at the crop's border is read again.
#include "sgan_common.h"

#define SG_PH_T 32               // tile side
#define SG_PH_PLANES 3           // masked channels staged together: 3 (32 + 24) (32 + 24 + 32) floats = 59136 bytes at R = 12
#define SG_PH_MAX_DIM (1 << 22)  // H, W: y * W + x and the mirror's 2 (N - 1) stay far inside int64 / int32

// i folded into [0, N) by reflection about the first and the last pixel, neither repeated (the rule of sgan_elastic.hip / sgan_tile.hip)
__device__ __forceinline__ int sg_ph_mirror(int i, int N) {
    if (N == 1) return 0;
    const int P = 2 * (N - 1);
    int m = i % P;
    if (m < 0) m += P;
    return m < N ? m : P - m;
}

// one pass of the separable blur at LDS address a, neighbours `pitch` floats apart: the expression of the header, tap by tap
__device__ __forceinline__ float sg_ph_pass(const float* a, int pitch, int R, const float (&w)[SGAN_PHOTO_MAX_R + 1]) {
    float acc = w[0] * a[0];
#pragma unroll
    for (int k = 1; k <= SGAN_PHOTO_MAX_R; ++k) {
        if (k > R) break;
        acc = fmaf(w[k], a[-k * pitch] + a[k * pitch], acc);
    }
    return acc;
}

struct SgPhPoint {      // which point stages run: wave-uniform
    bool gamma, cb, noise, clamp;
};

__device__ __forceinline__ float sg_ph_point(float s, const SgPhPoint& on, const sgan_photo_rec& rec, float nz) {
    if (on.gamma) {
        float u = fminf(fmaxf(fmaf(0.5f, s, 0.5f), 0.f), 1.f);
        u = powf(u, rec.gamma);
        s = fmaf(2.f, u, -1.f);
    }
    if (on.cb) s = fmaf(rec.contrast, s, 2.f * rec.brightness);
    if (on.noise) s = fmaf(rec.sigma_n, nz, s);
    if (on.clamp) s = fminf(fmaxf(s, -1.f), 1.f);
    return s;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void sg_image_photo_kernel(const float* __restrict__ src, int src_ld, float* __restrict__ dst, int dst_ld, int H,
                                                             int W, int Cstore, int mask, sgan_photo_rec rec, const float* __restrict__ noise,
                                                             int tiles_x, int64_t ntiles) {
    extern __shared__ __attribute__((aligned(16))) float sg_ph_lds[];
    const int R = rec.R, SW = SG_PH_T + 2 * R, SH = SG_PH_T + 2 * R;
    const int PL = __popc((unsigned)mask) < SG_PH_PLANES ? __popc((unsigned)mask) : SG_PH_PLANES;      // planes the launch allocated
    float* const S = sg_ph_lds;                                    // [plane][SH][SW]: the tile and its halo
    float* const Hb = S + PL * SH * SW;                            // [plane][SH][32]: after the row pass
    float w[SGAN_PHOTO_MAX_R + 1];
#pragma unroll
    for (int k = 0; k <= SGAN_PHOTO_MAX_R; ++k) w[k] = rec.w[k];
    SgPhPoint on;
    on.gamma = rec.gamma != 1.f;
    on.cb = rec.contrast != 1.f || rec.brightness != 0.f;
    on.noise = noise != nullptr && rec.sigma_n != 0.f;
    on.clamp = on.gamma || on.cb || on.noise;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;      // owns the pixels (ly + 8 k, lx), k < 4

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int ty0 = (int)(tile / tiles_x) * SG_PH_T, tx0 = (int)(tile % tiles_x) * SG_PH_T;
        const int x = tx0 + lx;
        bool occluded[4];
        float occ_value[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = ty0 + ly + 8 * k;
            occluded[k] = false;
            occ_value[k] = 0.f;
#pragma unroll
            for (int b = 0; b < SGAN_PHOTO_MAX_BOX; ++b)
                if (b < rec.nbox && y >= rec.box_y0[b] && y < rec.box_y1[b] && x >= rec.box_x0[b] && x < rec.box_x1[b]) {
                    occluded[k] = true;      // a later box wins
                    occ_value[k] = rec.box_value[b];
                }
        }

        f32x4 px[4];      // VEC4: the owned pixels, kept for the channels that are only copied
        if (VEC4) {
#pragma unroll
            for (int k = 0; k < 4; ++k)      // outside the crop (ragged tile): the mirrored pixel, needed in LDS only
                px[k] = *(const f32x4*)(src + ((int64_t)sg_ph_mirror(ty0 + ly + 8 * k, H) * W + sg_ph_mirror(x, W)) * src_ld);
        }

        int rem = mask, j0 = 0;      // masked channels not yet done; ordinal of the group's first one among the masked channels
        do {
            int ch[SG_PH_PLANES], np = 0;
#pragma unroll
            for (int p = 0; p < SG_PH_PLANES; ++p) {
                ch[p] = rem ? __ffs(rem) - 1 : -1;
                if (rem) ++np;
                rem &= rem - 1;
            }
            if (R > 0 && np > 0) {
                if (VEC4) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int p = 0; p < SG_PH_PLANES; ++p)
                            if (p < np) S[(p * SH + R + ly + 8 * k) * SW + R + lx] = px[k][ch[p]];
                }
                for (int i = threadIdx.x; i < SH * SW; i += 256) {
                    const int sy = i / SW, sx = i - sy * SW;
                    if (VEC4 && sy >= R && sy < R + SG_PH_T && sx >= R && sx < R + SG_PH_T) continue;      // the owner's
                    const float* q = src + ((int64_t)sg_ph_mirror(ty0 - R + sy, H) * W + sg_ph_mirror(tx0 - R + sx, W)) * src_ld;
                    if (VEC4) {
                        const f32x4 v = *(const f32x4*)q;
#pragma unroll
                        for (int p = 0; p < SG_PH_PLANES; ++p)
                            if (p < np) S[p * SH * SW + i] = v[ch[p]];
                    } else {
#pragma unroll
                        for (int p = 0; p < SG_PH_PLANES; ++p)
                            if (p < np) S[p * SH * SW + i] = q[ch[p]];
                    }
                }
                SG_SYNC();      // S is complete
                for (int i = threadIdx.x; i < np * SH * SG_PH_T; i += 256) {
                    const int row = i >> 5, c = i & 31;      // row = plane * SH + staged row
                    Hb[i] = sg_ph_pass(S + row * SW + R + c, 1, R, w);
                }
                SG_SYNC();      // Hb is complete; nothing reads S after this
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int y = ty0 + ly + 8 * k;
                if (y >= H || x >= W) continue;
                const int64_t pix = (int64_t)y * W + x;
#pragma unroll
                for (int p = 0; p < SG_PH_PLANES; ++p) {
                    if (p >= np) continue;
                    float s;
                    if (R > 0) s = sg_ph_pass(Hb + (p * SH + R + ly + 8 * k) * SG_PH_T + lx, SG_PH_T, R, w);
                    else s = VEC4 ? px[k][ch[p]] : src[pix * src_ld + ch[p]];
                    if (on.clamp) s = sg_ph_point(s, on, rec, on.noise ? noise[(int64_t)(j0 + p) * H * W + pix] : 0.f);
                    if (occluded[k]) s = occ_value[k];
                    if (VEC4) px[k][ch[p]] = s;
                    else dst[pix * dst_ld + ch[p]] = s;
                }
            }
            j0 += np;
            if (R > 0 && rem) SG_SYNC();      // the next group overwrites S and Hb
        } while (rem);

#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = ty0 + ly + 8 * k;
            if (y >= H || x >= W) continue;
            const int64_t pix = (int64_t)y * W + x;
            if (VEC4) {
                *(f32x4*)(dst + pix * dst_ld) = px[k];
            } else {
                const uint32_t* s = (const uint32_t*)(src + pix * src_ld);
                uint32_t* d = (uint32_t*)(dst + pix * dst_ld);
                for (int c = 0; c < Cstore; ++c)
                    if (c >= 31 || !((mask >> c) & 1)) d[c] = s[c];      // labels and padding: the bits
            }
        }
        if (R > 0 && tile + gridDim.x < ntiles) SG_SYNC();      // the next tile overwrites S and Hb
    }
}

// 1 with the reason set: refused, nothing launched
#define SG_PH_REFUSE(cond, ...)                         \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

extern "C" int sgan_image_photo(const float* src, int32_t src_ld, float* dst, int32_t dst_ld, int32_t H, int32_t W, int32_t Cstore,
                                int32_t channel_mask, const sgan_photo_rec* rec_host, const float* noise, void* stream) {
    SG_PH_REFUSE(src && dst && rec_host, "image_photo: null src, dst or record");
    SG_PH_REFUSE(H >= 1 && W >= 1 && H <= SG_PH_MAX_DIM && W <= SG_PH_MAX_DIM, "image_photo: crop %d x %d: sides of 1 .. %d pixels", W, H,
                 SG_PH_MAX_DIM);
    SG_PH_REFUSE(Cstore >= 1 && src_ld >= Cstore && dst_ld >= Cstore, "image_photo: %d stored channels at pixel strides %d and %d", Cstore,
                 src_ld, dst_ld);
    SG_PH_REFUSE(channel_mask >= 0 && (Cstore >= 31 || (channel_mask >> Cstore) == 0), "image_photo: channel mask 0x%x has a bit at or above "
                 "the %d stored channels", (unsigned)channel_mask, Cstore);
    const int64_t npix = (int64_t)H * W;
    const char *s0 = (const char*)src, *s1 = (const char*)(src + (npix - 1) * src_ld + Cstore);
    const char *d0 = (const char*)dst, *d1 = (const char*)(dst + (npix - 1) * dst_ld + Cstore);
    SG_PH_REFUSE(s1 <= d0 || d1 <= s0, "image_photo: src and dst overlap (the kernel is out of place)");
    const sgan_photo_rec rec = *rec_host;
    const int maxR = (H < W ? H : W) - 1 < SGAN_PHOTO_MAX_R ? (H < W ? H : W) - 1 : SGAN_PHOTO_MAX_R;
    SG_PH_REFUSE(rec.R >= 0 && rec.R <= maxR, "image_photo: blur radius %d outside 0 .. %d (at most %d, and min(H, W) - 1)", rec.R, maxR,
                 SGAN_PHOTO_MAX_R);
    for (int k = 0; k <= rec.R; ++k) SG_PH_REFUSE(__builtin_isfinite(rec.w[k]), "image_photo: tap %d is not finite", k);
    SG_PH_REFUSE(__builtin_isfinite(rec.gamma) && __builtin_isfinite(rec.contrast) && __builtin_isfinite(rec.brightness) && __builtin_isfinite(rec.sigma_n),
                 "image_photo: a parameter is not finite (gamma %g, contrast %g, brightness %g, sigma_n %g)", rec.gamma, rec.contrast,
                 rec.brightness, rec.sigma_n);
    SG_PH_REFUSE(rec.gamma >= 0.5f && rec.gamma <= 2.f, "image_photo: gamma %g outside [0.5, 2]", rec.gamma);
    SG_PH_REFUSE(rec.contrast > 0.f, "image_photo: contrast %g must be positive", rec.contrast);
    SG_PH_REFUSE(rec.sigma_n >= 0.f, "image_photo: sigma_n %g must not be negative", rec.sigma_n);
    SG_PH_REFUSE(rec.nbox >= 0 && rec.nbox <= SGAN_PHOTO_MAX_BOX, "image_photo: %d boxes (0 .. %d)", rec.nbox, SGAN_PHOTO_MAX_BOX);
    for (int b = 0; b < rec.nbox; ++b) SG_PH_REFUSE(__builtin_isfinite(rec.box_value[b]), "image_photo: the value of box %d is not finite", b);

    const int tiles_x = (W + SG_PH_T - 1) / SG_PH_T, tiles_y = (H + SG_PH_T - 1) / SG_PH_T;
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;
    const int blocks = ntiles > (1 << 20) ? (1 << 20) : (int)ntiles;
    const int side = SG_PH_T + 2 * rec.R;
    const int nmask = __builtin_popcount((unsigned)channel_mask), planes = nmask < SG_PH_PLANES ? nmask : SG_PH_PLANES;
    const size_t lds = rec.R > 0 ? (size_t)planes * side * (side + SG_PH_T) * sizeof(float) : 0;      // 19712 bytes a plane at R = 12
    const bool vec4 = Cstore == 4 && src_ld % 4 == 0 && dst_ld % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0 &&
                      nmask <= SG_PH_PLANES;      // one 16-byte load and store per pixel
    if (vec4)
        hipLaunchKernelGGL(sg_image_photo_kernel<true>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, src, src_ld, dst, dst_ld, H, W,
                           Cstore, channel_mask, rec, noise, tiles_x, ntiles);
    else
        hipLaunchKernelGGL(sg_image_photo_kernel<false>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, src, src_ld, dst, dst_ld, H, W,
                           Cstore, channel_mask, rec, noise, tiles_x, ntiles);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_image_photo_kernel";
    return SGAN_OK;
}
