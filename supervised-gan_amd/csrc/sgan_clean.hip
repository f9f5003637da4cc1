// Cleaning a predicted wall map before it is scored (include/sgan_hip.h, "cleaning the prediction"): a morphological
// closing with a Euclidean disk, wall components below an area dropped, cells below an area filled.  The expensive parts are the
// library's own exact kernels, called through their public entries: sgan_edt_sq twice for the closing (a threshold of the exact
// distance transform IS the dilation / erosion by a disk) and sgan_ccl_label once per area filter.  This file holds the streaming
// passes between them; every result is an integer or a 0 / 1 plane, so nothing depends on the order the atomics arrive in.
//
//   thresh: an int32 dsq plane (or, in copy mode, the input plane) to a 0 / 1 float plane and / or its complement.
//             copy    wall = x > 0.5                      the input, where no stage before the first labelling makes a dense plane
//             dilate  wall = 0 <= d <= rsq                D of the definition; only its complement is written, the second transform reads it
//             erode   wall = d < 0 || d > rsq             the closed wall; counts the pixels the input did not have
//   count:  count[label - 1] += pixels, label = 1 + the component's smallest raster index.  A wave holds 64 consecutive pixels and
//           merges them by label with ballots before it issues one atomic per distinct label (sgan_regions.hip's segmented reduction,
//           with the pixel count alone); a wave walks four such groups and carries a group that is one single label over to the next,
//           so a map that is one large component costs one atomic per 256 pixels, not one per pixel.
//   apply:  wall = label != 0 && count >= min  (specks: the labels are those of the wall components, i.e. of the complement plane)
//           wall = label == 0 || count < min   (small cells: the labels are those of the free components)
//           and the number of components / pixels that changed side; a component is counted at its root, label - 1 == raster index.
// The statistics go straight to the caller's accumulator: one 64-bit atomic per wave and nonzero counter.
// Workspace: [sgan_edt_sq's workspace][ip: H W int32, dsq during the closing, labels afterwards][count: H W int32][comp: H W float],
// each rounded up to 16 bytes.
#include "sgan_common.h"

#define SG_CLEAN_THREADS 256
#define SG_CLEAN_PER 4                                          // pixels per thread of the streaming passes, 256 apart
#define SG_CLEAN_BLOCK (SG_CLEAN_THREADS * SG_CLEAN_PER)
#define SG_CLEAN_MAX_RSQ 4096
#define SG_CLEAN_MAX_DIM 32768                                  // sgan_edt_sq's limit
#define SG_CLEAN_COPY 0
#define SG_CLEAN_DILATE 1
#define SG_CLEAN_ERODE 2
#define SG_CLEAN_ERR_LABELS 4                                   // a label outside 0 .. H W (the bit the Rand kernels raise for it)

// a refused call: the reason goes to sgan_last_error, the entry returns 1 and has launched nothing
#define SG_CLEAN_REFUSE(cond, ...)                      \
    do {                                                \
        if (!(cond)) {                                  \
            sgan_fail(SGAN_ERR_INVALID, __VA_ARGS__);   \
            return 1;                                   \
        }                                               \
    } while (0)

// acc[k] += the sum of v over the wave; every lane of the wave calls it
__device__ __forceinline__ void sg_clean_add(int64_t* acc, int k, int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)&acc[k], (unsigned long long)v);
}

__global__ __launch_bounds__(SG_CLEAN_THREADS) void sg_clean_zero_kernel(int4* __restrict__ p, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * SG_CLEAN_THREADS + threadIdx.x; i < n16; i += (int64_t)gridDim.x * SG_CLEAN_THREADS)
        p[i] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(SG_CLEAN_THREADS) void sg_clean_thresh_kernel(const int32_t* __restrict__ dsq, const float* __restrict__ plane,
                                                                           int64_t pix_stride, int n, int mode, int rsq, float* __restrict__ out,
                                                                           float* __restrict__ comp, int64_t* acc, int images) {
    const int base = blockIdx.x * SG_CLEAN_BLOCK + threadIdx.x;      // n < 2^30: no overflow
    int set = 0;
#pragma unroll
    for (int k = 0; k < SG_CLEAN_PER; ++k) {
        const int i = base + k * SG_CLEAN_THREADS;
        if (i >= n) continue;
        const bool was = mode != SG_CLEAN_DILATE && plane[(int64_t)i * pix_stride] > 0.5f;      // a NaN and an exact 0.5 are not wall
        bool wall = was;
        if (mode != SG_CLEAN_COPY) {
            const int d = dsq[i];
            wall = mode == SG_CLEAN_DILATE ? (d >= 0 && d <= rsq) : (d < 0 || d > rsq);
        }
        if (out) out[i] = wall ? 1.f : 0.f;
        if (comp) comp[i] = wall ? 0.f : 1.f;
        set += (wall && !was && mode == SG_CLEAN_ERODE) ? 1 : 0;
    }
    if (!acc) return;      // uniform
    sg_clean_add(acc, 0, set);
    if (images && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)&acc[5], 1ull);
}

__global__ __launch_bounds__(SG_CLEAN_THREADS) void sg_clean_count_kernel(const int32_t* __restrict__ L, int n, int32_t* count, int32_t* dev_err) {
    const int lane = threadIdx.x & 63;
    const int base = blockIdx.x * SG_CLEAN_BLOCK + (threadIdx.x >> 6) * (64 * SG_CLEAN_PER) + lane;      // a wave owns 256 consecutive pixels
    int carry_key = 0, carry_cnt = 0;      // pixels of whole groups of one label, not yet added: the same in every lane
    for (int k = 0; k < SG_CLEAN_PER; ++k) {
        const int i = base + k * 64;
        int t = i < n ? L[i] : 0;
        if (t < 0 || t > n) {
            __hip_atomic_fetch_or(dev_err, SG_CLEAN_ERR_LABELS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t = 0;
        }
        bool pending = t != 0;
        for (int it = 0; it < 64; ++it) {      // one round per distinct label of the group
            const unsigned long long waiting = __ballot(pending);
            if (waiting == 0) break;      // uniform
            const int leader = __builtin_ctzll(waiting);
            const int key = __shfl(t, leader, 64);
            const bool same = pending && t == key;
            const int cnt = __builtin_popcountll(__ballot(same));
            if (same) pending = false;
            if (cnt == 64) {      // uniform: the whole group is one label
                if (key != carry_key && carry_cnt) {
                    if (lane == 0) atomicAdd(&count[carry_key - 1], carry_cnt);
                    carry_cnt = 0;
                }
                carry_key = key;
                carry_cnt += 64;
            } else if (lane == leader) {
                atomicAdd(&count[key - 1], cnt);
            }
        }
    }
    if (carry_cnt && lane == 0) atomicAdd(&count[carry_key - 1], carry_cnt);
}

__global__ __launch_bounds__(SG_CLEAN_THREADS) void sg_clean_apply_kernel(const int32_t* __restrict__ L, const int32_t* __restrict__ count, int n,
                                                                          int min_area, int fill, float* __restrict__ out, int64_t* acc,
                                                                          int images) {
    const int base = blockIdx.x * SG_CLEAN_BLOCK + threadIdx.x;
    int comps = 0, pixels = 0;
#pragma unroll
    for (int k = 0; k < SG_CLEAN_PER; ++k) {
        const int i = base + k * SG_CLEAN_THREADS;
        if (i >= n) continue;
        int t = L[i];
        if (t < 0 || t > n) t = 0;      // reported by the count pass
        const bool small = t != 0 && count[t - 1] < min_area;
        const bool wall = fill ? (t == 0 || small) : (t != 0 && !small);
        out[i] = wall ? 1.f : 0.f;
        pixels += small ? 1 : 0;
        comps += (small && t - 1 == i) ? 1 : 0;
    }
    if (!acc) return;      // uniform
    sg_clean_add(acc, fill ? 3 : 1, comps);
    sg_clean_add(acc, fill ? 4 : 2, pixels);
    if (images && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)&acc[5], 1ull);
}

struct SgCleanLayout {
    int64_t off_ip, off_count, off_comp, bytes;
};

static bool sg_clean_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && H <= SG_CLEAN_MAX_DIM && W <= SG_CLEAN_MAX_DIM && (int64_t)H * W < (1ll << 30);
}

static SgCleanLayout sg_clean_layout(int32_t H, int32_t W) {
    const int64_t plane = (4ll * H * W + 15) & ~15ll;
    SgCleanLayout l;
    l.off_ip = (sgan_edt_workspace(H, W) + 15) & ~15ll;
    l.off_count = l.off_ip + plane;
    l.off_comp = l.off_count + plane;
    l.bytes = l.off_comp + plane;
    return l;
}

extern "C" int64_t sgan_clean_workspace(int32_t H, int32_t W) {
    if (!sg_clean_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_clean_layout(H, W).bytes;
}

extern "C" int sgan_clean_wall(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t close_rsq, int32_t min_wall, int32_t min_cell,
                               float* out, int64_t* acc, void* workspace, int64_t workspace_bytes, int32_t* dev_err, void* stream) {
    SG_CLEAN_REFUSE(plane && out && workspace && dev_err, "null pointer");
    SG_CLEAN_REFUSE(sg_clean_shape_ok(H, W) && pix_stride >= 1, "bad shape %d x %d (H, W <= %d, H W < 2^30), pixel stride %lld", H, W,
                    SG_CLEAN_MAX_DIM, (long long)pix_stride);
    SG_CLEAN_REFUSE(close_rsq >= 0 && close_rsq <= SG_CLEAN_MAX_RSQ && min_wall >= 0 && min_cell >= 0,
                    "bad parameter: close_rsq %d (0 .. %d), min_wall %d, min_cell %d (>= 0)", close_rsq, SG_CLEAN_MAX_RSQ, min_wall, min_cell);
    SG_CLEAN_REFUSE((const float*)out != plane, "out aliases the plane");
    const SgCleanLayout l = sg_clean_layout(H, W);
    SG_CLEAN_REFUSE(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_clean_workspace); nothing was launched",
                    (long long)workspace_bytes, (long long)l.bytes, H, W);
    SG_CLEAN_REFUSE(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    int32_t* ip = (int32_t*)((char*)workspace + l.off_ip);
    int32_t* count = (int32_t*)((char*)workspace + l.off_count);
    float* comp = (float*)((char*)workspace + l.off_comp);
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W;
    const dim3 grid((n + SG_CLEAN_BLOCK - 1) / SG_CLEAN_BLOCK), block(SG_CLEAN_THREADS);
    const int64_t n16 = (4ll * n + 15) / 16;
    const dim3 zgrid((unsigned)((n16 + SG_CLEAN_THREADS - 1) / SG_CLEAN_THREADS < 1024 ? (n16 + SG_CLEAN_THREADS - 1) / SG_CLEAN_THREADS : 1024));
    int rc;

    // The wall so far is `out` once a stage has written it, the caller's plane before; the last launch counts the image.
    if (close_rsq > 0) {
        if ((rc = sgan_edt_sq(plane, pix_stride, H, W, ip, workspace, l.off_ip, dev_err, stream)) != SGAN_OK) return rc;
        hipLaunchKernelGGL(sg_clean_thresh_kernel, grid, block, 0, st, (const int32_t*)ip, plane, pix_stride, n, SG_CLEAN_DILATE, close_rsq,
                           (float*)nullptr, comp, (int64_t*)nullptr, 0);
        SGAN_LAUNCH_CHECK();
        if ((rc = sgan_edt_sq(comp, 1, H, W, ip, workspace, l.off_ip, dev_err, stream)) != SGAN_OK) return rc;
        hipLaunchKernelGGL(sg_clean_thresh_kernel, grid, block, 0, st, (const int32_t*)ip, plane, pix_stride, n, SG_CLEAN_ERODE, close_rsq, out,
                           min_wall > 0 ? comp : (float*)nullptr, acc, min_wall == 0 && min_cell == 0 ? 1 : 0);
        SGAN_LAUNCH_CHECK();
    } else if (min_wall > 0 || min_cell == 0) {
        hipLaunchKernelGGL(sg_clean_thresh_kernel, grid, block, 0, st, (const int32_t*)nullptr, plane, pix_stride, n, SG_CLEAN_COPY, 0, out,
                           min_wall > 0 ? comp : (float*)nullptr, acc, min_wall == 0 ? 1 : 0);
        SGAN_LAUNCH_CHECK();
    }
    for (int fill = 0; fill < 2; ++fill) {
        const int min_area = fill ? min_cell : min_wall;
        if (min_area == 0) continue;
        // the specks are the free components of the complement plane; the cells those of the wall as it stands
        const bool from_plane = fill && close_rsq == 0 && min_wall == 0;
        if ((rc = sgan_ccl_label(fill ? (from_plane ? plane : out) : comp, from_plane ? pix_stride : 1, H, W, ip, dev_err, stream)) != SGAN_OK)
            return rc;
        hipLaunchKernelGGL(sg_clean_zero_kernel, zgrid, block, 0, st, (int4*)count, n16);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_clean_count_kernel, grid, block, 0, st, (const int32_t*)ip, n, count, dev_err);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_clean_apply_kernel, grid, block, 0, st, (const int32_t*)ip, (const int32_t*)count, n, min_area, fill, out,
                           acc, fill || min_cell == 0 ? 1 : 0);
        SGAN_LAUNCH_CHECK();
    }
    g_sgan_last_kernel = "sg_clean_apply_kernel";
    return SGAN_OK;
}
