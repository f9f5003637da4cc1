// Segmentation metrics on the device (include/sgan_hip.h, "segmentation metrics"): connected-component labelling of a thresholded
// boundary map, the Rand F-score, the information score (VInfo) and the object-level match counts of two such labellings, and the
// confusion matrix of two class maps.  The trainers call these after
// every optimizer step; nothing is read back until the accuracies are asked for.
//
// These kernels are bound by latency and atomics, not by arithmetic.  Three rules hold throughout:
//   * every loop has a bound that does not depend on what other threads do: a union-find parent is always SMALLER than its child,
//     so a walk to the root takes at most (index) steps and is cut at the pixel count anyway; a union retries only when another
//     thread lowered the same parent in between, and is cut at SG_UNION_MAX_TRIES; a table probe is cut at SGAN_RAND_F_MAX_PROBE.
//     A cut sets *dev_err and drops the pixel: a wrong label that is reported, never a hang.
//   * what workgroups tell each other inside one launch goes through atomics at agent scope (the XCDs' L2s are not coherent for
//     plain accesses); plain loads and stores carry data across launch boundaries only, or data that is valid whether old or new.
//   * the results are integers, so they do not depend on the order the atomics arrive in.
#include "sgan_common.h"
#include "sgan_reduce.h"

#define SG_CCL_TW 64
#define SG_CCL_TH 16
#define SG_CCL_THREADS 256
#define SG_UNION_MAX_TRIES (1 << 20)

#define SG_LOAD_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SG_LOAD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ void sg_flag(int32_t* dev_err, int code) {
    __hip_atomic_fetch_or(dev_err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Connected components.  Every link between two 8-neighbours joins a pixel p to one of the four neighbours that precede it in raster
// order: W, NW, N, NE.  Two of them are often implied by the others (N free: NW - N and N - NE are N's and NE's own W links; W free:
// W - NW is W's own N link), so a pixel makes the links
//     W if free;  N if free;  NW if free and neither N nor W is;  NE if free and N is not.
// A link inside a tile is made by the tile kernel in LDS, a link across a tile border by the border kernel on the label array; the
// rule holds for both because the links it relies on are made by one of the two as well.
// Union-find with "the smaller index is the parent": the root of a component is its smallest raster index, which IS the canonical
// label, so the outcome does not depend on the order the links are made in.
// ------------------------------------------------------------------------------------------------------------------------------

// LDS: P[i] = parent (tile-local index) of a free pixel, -1 for wall or outside the image
__device__ __forceinline__ int sg_lds_find(int* P, int i) {
    for (int it = 0; it < SG_CCL_TW * SG_CCL_TH; ++it) {
        const int p = SG_LOAD_WG(&P[i]);
        if (p == i) break;
        i = p;
    }
    return i;
}

__device__ __forceinline__ void sg_lds_union(int* P, int a, int b, int32_t* dev_err) {
    for (int it = 0; it < SG_UNION_MAX_TRIES; ++it) {
        a = sg_lds_find(P, a);
        b = sg_lds_find(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&P[a], b);      // a > b: hang the larger root under the smaller
        if (old == a) return;
        a = old;                                  // someone re-parented a meanwhile: its former parent still has to meet b
    }
    sg_flag(dev_err, 1);
}

// label array: L[i] = 0 for wall, else 1 + parent index
__device__ __forceinline__ int sg_glb_find(int32_t* L, int i, int n) {
    for (int it = 0; it < n; ++it) {
        const int p = SG_LOAD_AGENT(&L[i]) - 1;
        if (p == i || p < 0) break;
        i = p;
    }
    return i;
}

__device__ __forceinline__ void sg_glb_union(int32_t* L, int a, int b, int n, int32_t* dev_err) {
    for (int it = 0; it < SG_UNION_MAX_TRIES; ++it) {
        a = sg_glb_find(L, a, n);
        b = sg_glb_find(L, b, n);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b + 1) - 1;
        if (old == a) return;
        a = old;
    }
    sg_flag(dev_err, 1);
}

__global__ __launch_bounds__(SG_CCL_THREADS) void sg_ccl_tile_kernel(const float* __restrict__ plane, int64_t pix_stride, int H, int W,
                                                                     int32_t* __restrict__ L, int32_t* dev_err) {
    __shared__ int P[SG_CCL_TW * SG_CCL_TH];
    const int x0 = blockIdx.x * SG_CCL_TW, y0 = blockIdx.y * SG_CCL_TH;
    for (int p = threadIdx.x; p < SG_CCL_TW * SG_CCL_TH; p += SG_CCL_THREADS) {
        const int y = y0 + p / SG_CCL_TW, x = x0 + p % SG_CCL_TW;
        bool is_free = false;
        if (y < H && x < W) is_free = !(plane[((int64_t)y * W + x) * pix_stride] > 0.5f);
        P[p] = is_free ? p : -1;
    }
    SG_SYNC();      // P[] initialised
    for (int p = threadIdx.x; p < SG_CCL_TW * SG_CCL_TH; p += SG_CCL_THREADS) {
        if (SG_LOAD_WG(&P[p]) < 0) continue;      // a free pixel's entry stays >= 0 whatever the other threads do to it
        const int ly = p / SG_CCL_TW, lx = p % SG_CCL_TW;
        const bool fw = lx > 0 && SG_LOAD_WG(&P[p - 1]) >= 0;
        const bool fn = ly > 0 && SG_LOAD_WG(&P[p - SG_CCL_TW]) >= 0;
        const bool fnw = ly > 0 && lx > 0 && SG_LOAD_WG(&P[p - SG_CCL_TW - 1]) >= 0;
        const bool fne = ly > 0 && lx < SG_CCL_TW - 1 && SG_LOAD_WG(&P[p - SG_CCL_TW + 1]) >= 0;
        if (fw) sg_lds_union(P, p, p - 1, dev_err);
        if (fn) sg_lds_union(P, p, p - SG_CCL_TW, dev_err);
        if (fnw && !fn && !fw) sg_lds_union(P, p, p - SG_CCL_TW - 1, dev_err);
        if (fne && !fn) sg_lds_union(P, p, p - SG_CCL_TW + 1, dev_err);
    }
    SG_SYNC();      // every in-tile link made
    for (int p = threadIdx.x; p < SG_CCL_TW * SG_CCL_TH; p += SG_CCL_THREADS) {
        const int y = y0 + p / SG_CCL_TW, x = x0 + p % SG_CCL_TW;
        if (y >= H || x >= W) continue;
        int lab = 0;
        if (P[p] >= 0) {
            const int r = sg_lds_find(P, p);      // the tile-local order is the raster order, so r is the smallest raster index too
            lab = 1 + (y0 + r / SG_CCL_TW) * W + x0 + r % SG_CCL_TW;
        }
        L[y * W + x] = lab;
    }
}

__global__ __launch_bounds__(256) void sg_ccl_border_kernel(int32_t* L, int H, int W, int32_t* dev_err) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = H * W;
    if (i >= n) return;
    const int y = i / W, x = i % W, ly = y % SG_CCL_TH, lx = x % SG_CCL_TW;
    if (ly != 0 && lx != 0 && lx != SG_CCL_TW - 1) return;      // no preceding neighbour in another tile
    // wall or not never changes in this launch (a free entry stays >= 1), so plain loads may test it
    if (L[i] == 0) return;
    const bool fw = x > 0 && L[i - 1] != 0;
    const bool fn = y > 0 && L[i - W] != 0;
    const bool fnw = y > 0 && x > 0 && L[i - W - 1] != 0;
    const bool fne = y > 0 && x < W - 1 && L[i - W + 1] != 0;
    const bool cw = lx == 0, cn = ly == 0, cne = ly == 0 || lx == SG_CCL_TW - 1;      // which neighbours lie in another tile
    if (fw && cw) sg_glb_union(L, i, i - 1, n, dev_err);
    if (fn && cn) sg_glb_union(L, i, i - W, n, dev_err);
    if (fnw && !fn && !fw && (cw || cn)) sg_glb_union(L, i, i - W - 1, n, dev_err);
    if (fne && !fn && cne) sg_glb_union(L, i, i - W + 1, n, dev_err);
}

// Replaces every parent by the root.  In place: an entry another thread has already rewritten holds that pixel's root, which is as
// good a parent as the one it held before, and an aligned 4-byte access is never torn.
__global__ __launch_bounds__(256) void sg_ccl_flatten_kernel(int32_t* L, int n, int32_t* dev_err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int p = L[i] - 1;
    if (p < 0 || p == i) return;
    int it = 0;
    for (; it < n; ++it) {
        const int q = L[p] - 1;
        if (q == p || q < 0) break;
        p = q;
    }
    if (it == n) sg_flag(dev_err, 1);
    L[i] = p + 1;
}

extern "C" int sgan_ccl_label(const float* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t* labels, int32_t* dev_err, void* stream) {
    SGAN_CHECK(plane && labels && dev_err, "null pointer");
    SGAN_CHECK(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30) && pix_stride >= 1, "bad shape %d x %d, pixel stride %lld", H, W,
               (long long)pix_stride);
    const dim3 tiles((W + SG_CCL_TW - 1) / SG_CCL_TW, (H + SG_CCL_TH - 1) / SG_CCL_TH);
    SGAN_CHECK(tiles.y <= 65535, "more than 65535 tile rows");
    const int n = H * W, nb = (n + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_ccl_tile_kernel, tiles, dim3(SG_CCL_THREADS), 0, st, plane, pix_stride, H, W, labels, dev_err);
    SGAN_LAUNCH_CHECK();
    if (tiles.x > 1 || tiles.y > 1) {
        hipLaunchKernelGGL(sg_ccl_border_kernel, dim3(nb), dim3(256), 0, st, labels, H, W, dev_err);
        SGAN_LAUNCH_CHECK();
        hipLaunchKernelGGL(sg_ccl_flatten_kernel, dim3(nb), dim3(256), 0, st, labels, n, dev_err);
        SGAN_LAUNCH_CHECK();
    }
    g_sgan_last_kernel = "sg_ccl_tile_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Rand F-score.  Workspace: [A2, B2, AB2, aux: 4 uint64][keys: slots uint64][cnt_a: np int32][cnt_b: np int32][cnt_ab: slots int32],
// np = n + 1 rounded up to even, slots = the power of two >= max(2 n, 64).
// ------------------------------------------------------------------------------------------------------------------------------
struct SgRandLayout {
    int64_t slots, np, bytes;
    int log2_slots;
};

static SgRandLayout sg_rand_layout(int32_t H, int32_t W) {
    SgRandLayout l;
    const int64_t n = (int64_t)H * W;
    l.log2_slots = 6;
    while ((1ll << l.log2_slots) < 2 * n) ++l.log2_slots;
    l.slots = 1ll << l.log2_slots;
    l.np = (n + 2) & ~1ll;
    l.bytes = 32 + 8 * l.slots + 4 * (2 * l.np + l.slots);      // a multiple of 16
    return l;
}

__global__ __launch_bounds__(256) void sg_zero16_kernel(uint4* p, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ long long sg_wave_sum_i64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// n more pixels on a counter that held c:  (c + n)^2 - c^2
__device__ __forceinline__ long long sg_square_growth(int c, int n) { return (2ll * c + n) * n; }

// Lanes of one wave hold 64 consecutive pixels of a row.  `change`: this lane's value differs from its left neighbour's (lane 0: always;
// the lanes past the row's end hold 0, so they end the row's last run).  Returns the length inside the wave of the run that starts
// at this lane, or 0 when none starts here or `counted` is false.
__device__ __forceinline__ int sg_run_length(bool change, bool counted, int lane) {
    const unsigned long long changes = __ballot(change);
    if (!change || !counted) return 0;
    const unsigned long long later = lane == 63 ? 0ull : changes >> (lane + 1);
    return later ? __builtin_ctzll(later) + 1 : 64 - lane;
}

// Lanes with len > 0 hold (key, len).  The lanes of one key elect their first lane, which gets the key's summed length; every other
// lane gets 0.  A region that crosses the wave's 64 pixels several times (the one giant region of a percolating map crosses every
// wave of the image) then costs one atomic per wave instead of one per run: on per-pixel noise the same-address atomics of that
// region's counter were 94 % of the metric's time (kernel trace).  At most 64 rounds, one per distinct key.
__device__ __forceinline__ int sg_wave_merge(unsigned long long key, int len, int lane) {
    int total = 0;
    bool pending = len > 0;
    for (int it = 0; it < 64; ++it) {
        const unsigned long long waiting = __ballot(pending);
        if (waiting == 0) break;      // uniform
        const int leader = __builtin_ctzll(waiting);
        const unsigned lo = __shfl((unsigned)key, leader, 64), hi = __shfl((unsigned)(key >> 32), leader, 64);
        const bool same = pending && key == (((unsigned long long)hi << 32) | lo);
        int sum = same ? len : 0;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (same) {
            pending = false;
            if (lane == leader) total = sum;
        }
    }
    return total;
}

// What the two counting passes (Rand / VInfo and the object matches) share.  A workgroup's four waves each take one 64-pixel segment of a
// row; false, for the whole wave, when the segment lies past the image.  A lane past the row's end looks like wall in both maps and
// adds nothing; a label outside 0 .. H W sets bit 4 and its pixel is left out.
__device__ __forceinline__ bool sg_load_label_pair(const int32_t* __restrict__ T, const int32_t* __restrict__ S, int H, int W, int lane,
                                                   int32_t* dev_err, int& t, int& s) {
    const int segs = (W + 63) / 64;
    const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    t = s = 0;
    if (seg >= (int64_t)H * segs) return false;
    const int y = (int)(seg / segs), x = (int)(seg % segs) * 64 + lane;
    const int n = H * W;
    if (x < W) {
        t = T[y * W + x];
        s = S[y * W + x];
        if (t < 0 || t > n || s < 0 || s > n) {
            sg_flag(dev_err, 4);
            t = s = 0;
        }
    }
    return true;
}

// The slot of `key` in the open-addressing pair table, claimed if the key is new; -1, with bit 2 set, when the bounded probe ran out.
__device__ __forceinline__ long long sg_pair_slot(unsigned long long* keys, unsigned long long key, int log2_slots, int32_t* dev_err) {
    const unsigned long long mask = (1ull << log2_slots) - 1;
    unsigned long long slot = (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots);
    for (int probe = 0; probe < SGAN_RAND_F_MAX_PROBE; ++probe) {
        const unsigned long long seen = atomicCAS(&keys[slot], 0ull, key);      // t >= 1: a key is never 0
        if (seen == 0ull || seen == key) return (long long)slot;
        slot = (slot + 1) & mask;
    }
    sg_flag(dev_err, 2);
    return -1;
}

__global__ __launch_bounds__(256) void sg_rand_count_kernel(const int32_t* __restrict__ T, const int32_t* __restrict__ S, int H, int W,
                                                            unsigned long long* sums, unsigned long long* keys, int* cnt_a, int* cnt_b,
                                                            int* cnt_ab, int log2_slots, int32_t* dev_err) {
    const int lane = threadIdx.x & 63;
    int t, s;
    if (!sg_load_label_pair(T, S, H, W, lane, dev_err, t, s)) return;      // uniform over the wave
    const int tl = __shfl_up(t, 1, 64), sl = __shfl_up(s, 1, 64);
    const bool first = lane == 0;
    long long dA = 0, dB = 0, dAB = 0, aux = (t != 0 && s == 0) ? 1 : 0;
    // a_i: runs of one truth label
    int len = sg_wave_merge((unsigned)t, sg_run_length(first || tl != t, t != 0, lane), lane);
    if (len) dA = sg_square_growth(atomicAdd(&cnt_a[t], len), len);
    // b_j and c_ij: runs of one (truth, prediction) pair with both set.  Two neighbours that are both set in one map belong to one
    // component there, so such a run ends only where one of the maps has wall: a run of the pair is a run of the prediction label too.
    const bool both = t != 0 && s != 0;
    const int run = sg_run_length(first || tl != t || sl != s, both, lane);
    const unsigned long long key = ((unsigned long long)(unsigned)t << 32) | (unsigned)s;
    len = sg_wave_merge((unsigned)s, run, lane);
    if (len) dB = sg_square_growth(atomicAdd(&cnt_b[s], len), len);
    len = sg_wave_merge(key, run, lane);
    if (len) {
        const long long slot = sg_pair_slot(keys, key, log2_slots, dev_err);
        if (slot >= 0) dAB = sg_square_growth(atomicAdd(&cnt_ab[slot], len), len);
    }
    dA = sg_wave_sum_i64(dA);
    dB = sg_wave_sum_i64(dB);
    dAB = sg_wave_sum_i64(dAB);
    aux = sg_wave_sum_i64(aux);
    if (lane == 0) {
        if (dA) atomicAdd(&sums[0], (unsigned long long)dA);
        if (dB) atomicAdd(&sums[1], (unsigned long long)dB);
        if (dAB) atomicAdd(&sums[2], (unsigned long long)dAB);
        if (aux) atomicAdd(&sums[3], (unsigned long long)aux);
    }
}

// The F-score from the four integers; one expression for every kernel that reports it, so the same integers give the same bits.
__device__ __forceinline__ double sg_rand_f_from_sums(unsigned long long A2, unsigned long long B2, unsigned long long AB2,
                                                      unsigned long long aux) {
    double f = __builtin_nan("");
    if (A2 != 0 && B2 + aux != 0) {
        const double num = (double)(AB2 + aux);
        const double prec = num / (double)(B2 + aux), rec = num / (double)A2;
        f = 2.0 / (1.0 / prec + 1.0 / rec);
    }
    return f;
}

__global__ void sg_rand_final_kernel(const unsigned long long* sums, double* acc, int64_t* sums_out, double* f_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long A2 = sums[0], B2 = sums[1], AB2 = sums[2], aux = sums[3];
    const double f = sg_rand_f_from_sums(A2, B2, AB2, aux);
    acc[0] += f;
    acc[1] += 1.0;
    if (sums_out) {
        sums_out[0] = (int64_t)A2;
        sums_out[1] = (int64_t)B2;
        sums_out[2] = (int64_t)AB2;
        sums_out[3] = (int64_t)aux;
    }
    if (f_out) *f_out = f;
}

extern "C" int64_t sgan_rand_f_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_rand_layout(H, W).bytes;
}

// The launches both scores share: zero `zero_bytes` of the workspace (the Rand layout, and whatever the caller keeps behind it), then
// count.  Afterwards the workspace holds A2, B2, AB2, aux and every a_i, b_j, c_ij.
static int sg_rand_count_launch(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, void* workspace,
                                const SgRandLayout& l, int64_t zero_bytes, int32_t* dev_err, hipStream_t st) {
    unsigned long long* sums = (unsigned long long*)workspace;
    unsigned long long* keys = sums + 4;
    int* cnt_a = (int*)(keys + l.slots);
    int* cnt_b = cnt_a + l.np;
    int* cnt_ab = cnt_b + l.np;
    const int64_t n16 = zero_bytes / 16;
    hipLaunchKernelGGL(sg_zero16_kernel, dim3((unsigned)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048)), dim3(256), 0, st,
                       (uint4*)workspace, n16);
    SGAN_LAUNCH_CHECK();
    const int64_t waves = (int64_t)H * ((W + 63) / 64);
    SGAN_CHECK((waves + 3) / 4 < (1ll << 31), "too many rows");
    hipLaunchKernelGGL(sg_rand_count_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, t_labels, s_labels, H, W, sums, keys,
                       cnt_a, cnt_b, cnt_ab, l.log2_slots, dev_err);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}

extern "C" int sgan_rand_f_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, void* workspace,
                                      int64_t workspace_bytes, double* acc, int64_t* sums_out, double* f_out, int32_t* dev_err,
                                      void* stream) {
    SGAN_CHECK(t_labels && s_labels && workspace && acc && dev_err, "null pointer");
    SGAN_CHECK(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "bad shape %d x %d", H, W);
    const SgRandLayout l = sg_rand_layout(H, W);
    SGAN_CHECK(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_rand_f_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)l.bytes, H, W);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int rc = sg_rand_count_launch(t_labels, s_labels, H, W, workspace, l, l.bytes, dev_err, st);
    if (rc != SGAN_OK) return rc;
    hipLaunchKernelGGL(sg_rand_final_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)workspace, acc, sums_out, f_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_rand_count_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Information score (VInfo) from the counters the Rand count leaves behind.  Workspace: the Rand layout, then
// [SA, SB, SAB: 3 double][m: 1 uint64] (SG_VINFO_TAIL bytes), zeroed with it.
//   SA = sum_i a_i ln a_i,  SB = sum_j b_j ln b_j,  SAB = sum_ij c_ij ln c_ij,  m = sum_i a_i  (natural log, counts > 0)
// cnt_a, cnt_b and cnt_ab follow each other in the workspace (np, np and slots int32; np is even and slots a multiple of 64, so the
// three together are a whole number of 16-byte words starting on one): the reduce kernel reads them as ONE array of uint4 and tells
// by its index which sum a counter belongs to.  cnt_a[0] and cnt_b[0] (wall) are never written and stay 0.
// ------------------------------------------------------------------------------------------------------------------------------
#define SG_VINFO_TAIL 32
#define SG_VINFO_PARTS 11

__device__ __forceinline__ void sg_vinfo_term(unsigned c, int64_t e, int64_t np, double& sa, double& sb, double& sab, long long& m) {
    if (c == 0) return;
    const double term = c > 1 ? (double)c * log((double)c) : 0.0;
    if (e < np) {
        sa += term;
        m += c;
    } else if (e < 2 * np) {
        sb += term;
    } else {
        sab += term;
    }
}

__device__ __forceinline__ double sg_wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Latency-bound: ~4 H W counters, most of them 0, one 16-byte load per lane and trip; a word of four zeros costs nothing more.
// The fp64 sums arrive in an order that depends on scheduling: SA, SB, SAB are reproducible to rounding (~H W 2^-53 relative), m exactly.
__global__ __launch_bounds__(256) void sg_vinfo_reduce_kernel(const uint4* __restrict__ cnt, int64_t n16, int64_t np, double* vsum,
                                                              unsigned long long* m_out) {
    __shared__ double part[4][3];
    __shared__ long long part_m[4];
    double sa = 0.0, sb = 0.0, sab = 0.0;
    long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const uint4 v = cnt[i];
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        sg_vinfo_term(v.x, 4 * i, np, sa, sb, sab, m);
        sg_vinfo_term(v.y, 4 * i + 1, np, sa, sb, sab, m);
        sg_vinfo_term(v.z, 4 * i + 2, np, sa, sb, sab, m);
        sg_vinfo_term(v.w, 4 * i + 3, np, sa, sb, sab, m);
    }
    sa = sg_wave_sum_f64(sa);
    sb = sg_wave_sum_f64(sb);
    sab = sg_wave_sum_f64(sab);
    m = sg_wave_sum_i64(m);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = sa;
        part[wave][1] = sb;
        part[wave][2] = sab;
        part_m[wave] = m;
    }
    SG_SYNC();      // the four waves' partial sums
    if (threadIdx.x == 0) {
        sa = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
        sb = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
        sab = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
        m = part_m[0] + part_m[1] + part_m[2] + part_m[3];
        if (sa != 0.0) atomicAdd(&vsum[0], sa);
        if (sb != 0.0) atomicAdd(&vsum[1], sb);
        if (sab != 0.0) atomicAdd(&vsum[2], sab);
        if (m) atomicAdd(m_out, (unsigned long long)m);
    }
}

// Which entropies are zero is decided from the integers: H_T = 0 iff truth is one region (A2 == m^2); H_S = 0 iff the prediction is
// one region over all of it (no pixel on prediction wall and B2 == m^2) or there is one pixel.  m < 2^30, so m^2 is exact.
__global__ void sg_vinfo_final_kernel(const unsigned long long* sums, const double* vsum, const unsigned long long* m_in, double* acc,
                                      double* acc_rand, double* parts_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long A2 = sums[0], B2 = sums[1], AB2 = sums[2], aux = sums[3], m = *m_in;
    const double SA = vsum[0], SB = vsum[1], SAB = vsum[2], nan = __builtin_nan("");
    double hs = nan, ht = nan, mi = nan, v = nan, split = nan, merge = nan;
    if (m != 0) {
        const double dm = (double)m, lnm = log(dm);
        const bool ht_zero = A2 == m * m, hs_zero = (aux == 0 && B2 == m * m) || m == 1;
        ht = ht_zero ? 0.0 : lnm - SA / dm;
        hs = hs_zero ? 0.0 : lnm - SB / dm;
        const double hst = lnm - SAB / dm, lim = hs < ht ? hs : ht;
        mi = hs + ht - hst;
        mi = mi < 0.0 ? 0.0 : mi;
        mi = mi > lim ? lim : mi;
        if (ht_zero && hs_zero) v = 1.0;
        else if (ht_zero || hs_zero) v = 0.0;
        else v = 2.0 * mi / (hs + ht);
        if (!hs_zero) split = mi / hs;
        if (!ht_zero) merge = mi / ht;
    }
    acc[0] += v;
    acc[1] += 1.0;
    if (acc_rand) {
        acc_rand[0] += sg_rand_f_from_sums(A2, B2, AB2, aux);
        acc_rand[1] += 1.0;
    }
    if (parts_out) {
        parts_out[0] = SA;
        parts_out[1] = SB;
        parts_out[2] = SAB;
        parts_out[3] = (double)aux;
        parts_out[4] = (double)m;
        parts_out[5] = hs;
        parts_out[6] = ht;
        parts_out[7] = mi;
        parts_out[8] = v;
        parts_out[9] = split;
        parts_out[10] = merge;
    }
}

extern "C" int64_t sgan_vinfo_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_rand_layout(H, W).bytes + SG_VINFO_TAIL;
}

// workgroups of the reduce kernel: enough to fill the device's CUs four deep, never more than the data has 16-byte words for
static int64_t sg_vinfo_grid(int64_t n16) {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        cus = n;
    }
    const int64_t want = (n16 + 255) / 256, cap = 4ll * cus;
    return want < cap ? want : cap;
}

extern "C" int sgan_vinfo_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, void* workspace,
                                     int64_t workspace_bytes, double* acc, double* acc_rand, double* parts_out, int32_t* dev_err,
                                     void* stream) {
    SGAN_CHECK(t_labels && s_labels && workspace && acc && dev_err, "null pointer");
    SGAN_CHECK(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "bad shape %d x %d", H, W);
    const SgRandLayout l = sg_rand_layout(H, W);
    const int64_t need = l.bytes + SG_VINFO_TAIL;
    SGAN_CHECK(workspace_bytes >= need, "workspace of %lld bytes, %lld needed for %d x %d (sgan_vinfo_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)need, H, W);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int rc = sg_rand_count_launch(t_labels, s_labels, H, W, workspace, l, need, dev_err, st);
    if (rc != SGAN_OK) return rc;
    const unsigned long long* sums = (const unsigned long long*)workspace;
    const uint4* cnt = (const uint4*)((const char*)workspace + 32 + 8 * l.slots);
    double* vsum = (double*)((char*)workspace + l.bytes);
    unsigned long long* m_sum = (unsigned long long*)(vsum + 3);
    const int64_t n16 = (2 * l.np + l.slots) / 4;
    hipLaunchKernelGGL(sg_vinfo_reduce_kernel, dim3((unsigned)sg_vinfo_grid(n16)), dim3(256), 0, st, cnt, n16, l.np, vsum, m_sum);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_vinfo_final_kernel, dim3(1), dim3(64), 0, st, sums, (const double*)vsum, (const unsigned long long*)m_sum, acc,
                       acc_rand, parts_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_vinfo_reduce_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Object matching (include/sgan_hip.h, "object-level scores"): which truth region is found by which predicted region, at the ten
// IoU thresholds 0.5 .. 0.95.  Workspace: [stage: 16 x 8 bytes][keys: slots uint64][cnt_a: np int32][cnt_b: np int32][cnt_ab: slots
// int32] -- the Rand layout behind a staging block that is laid out as the accumulators are: stage[k] (uint64) is the pair's
// contribution to acc_i[k] (slot SGAN_OBJ_IMAGES stays 0), stage[14] and stage[15] (double) are SIoU and SSEG.
// Here a_i and b_j are WHOLE areas, so the count pass adds every run of a prediction label to cnt_b, not only those inside a truth
// region, and keeps no square sums.
// ------------------------------------------------------------------------------------------------------------------------------
#define SG_OBJ_STAGE 128
#define SG_OBJ_INTS 14      // the integer slots the evaluation reduces: acc_i[0 .. 13] (slot 12 is carried as 0)

static int64_t sg_obj_bytes(const SgRandLayout& l) { return l.bytes - 32 + SG_OBJ_STAGE; }

__global__ __launch_bounds__(256) void sg_obj_count_kernel(const int32_t* __restrict__ T, const int32_t* __restrict__ S, int H, int W,
                                                           unsigned long long* keys, int* cnt_a, int* cnt_b, int* cnt_ab, int log2_slots,
                                                           int32_t* dev_err) {
    const int lane = threadIdx.x & 63;
    int t, s;
    if (!sg_load_label_pair(T, S, H, W, lane, dev_err, t, s)) return;      // uniform over the wave
    const int tl = __shfl_up(t, 1, 64), sl = __shfl_up(s, 1, 64);
    const bool first = lane == 0;
    int len = sg_wave_merge((unsigned)t, sg_run_length(first || tl != t, t != 0, lane), lane);
    if (len) atomicAdd(&cnt_a[t], len);
    len = sg_wave_merge((unsigned)s, sg_run_length(first || sl != s, s != 0, lane), lane);
    if (len) atomicAdd(&cnt_b[s], len);
    const unsigned long long key = ((unsigned long long)(unsigned)t << 32) | (unsigned)s;
    len = sg_wave_merge(key, sg_run_length(first || tl != t || sl != s, t != 0 && s != 0, lane), lane);
    if (len) {
        const long long slot = sg_pair_slot(keys, key, log2_slots, dev_err);
        if (slot >= 0) atomicAdd(&cnt_ab[slot], len);
    }
}

struct SgObjPart {
    int n[SG_OBJ_INTS];      // a thread's and a wave's counts stay far below 2^31: there are fewer than 2^30 regions and pairs
    double siou, sseg;
};

// One nonzero counter of the array [cnt_a | cnt_b | cnt_ab]: a region that counts, or a pair whose two areas are looked up through
// the pair's key.  Every match is decided in 64-bit integers; the quotient is taken only for a pair that adds it to a sum.
__device__ __forceinline__ void sg_obj_term(unsigned c, int64_t e, int64_t np, const unsigned long long* __restrict__ keys,
                                            const int* __restrict__ cnt_a, const int* __restrict__ cnt_b, int min_area, SgObjPart& p) {
    if (c == 0) return;
    if (e < 2 * np) {
        if ((int)c < min_area) return;
        if (e < np) ++p.n[SGAN_OBJ_NT];
        else ++p.n[SGAN_OBJ_NS];
        return;
    }
    const unsigned long long key = keys[e - 2 * np];
    const int a = cnt_a[(unsigned)(key >> 32)], b = cnt_b[(unsigned)key];      // both labels were range-checked by the count pass
    if (a < min_area || b < min_area) return;
    const long long u = (long long)a + b - c, c20 = 20ll * c;
    const bool found = c20 > 10 * u, seg = 2ll * c > a;
    if (!found && !seg) return;
    const double iou = (double)c / (double)u;
    if (found) {
        p.siou += iou;
#pragma unroll
        for (int k = 0; k < 10; ++k) p.n[SGAN_OBJ_TP0 + k] += c20 > (10 + k) * u ? 1 : 0;
    }
    if (seg) {
        ++p.n[SGAN_OBJ_SEGN];
        p.sseg += iou;
    }
}

// As sg_vinfo_reduce_kernel: one 16-byte load per lane and trip over ~4 H W counters, most of them 0.  A workgroup adds what it found
// to the staging block once.
__global__ __launch_bounds__(256) void sg_obj_eval_kernel(const uint4* __restrict__ cnt, int64_t n16, int64_t np,
                                                          const unsigned long long* __restrict__ keys, int min_area,
                                                          unsigned long long* stage) {
    __shared__ int part_n[4][SG_OBJ_INTS];
    __shared__ double red[2][4];
    const int* cnt_a = (const int*)cnt;
    const int* cnt_b = cnt_a + np;
    SgObjPart p;
#pragma unroll
    for (int k = 0; k < SG_OBJ_INTS; ++k) p.n[k] = 0;
    p.siou = p.sseg = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const uint4 v = cnt[i];
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        sg_obj_term(v.x, 4 * i, np, keys, cnt_a, cnt_b, min_area, p);
        sg_obj_term(v.y, 4 * i + 1, np, keys, cnt_a, cnt_b, min_area, p);
        sg_obj_term(v.z, 4 * i + 2, np, keys, cnt_a, cnt_b, min_area, p);
        sg_obj_term(v.w, 4 * i + 3, np, keys, cnt_a, cnt_b, min_area, p);
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SG_OBJ_INTS; ++k) {
        int v = p.n[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) part_n[wave][k] = v;
    }
    const double siou = sg_block_sum<4>(p.siou, red[0]);      // its barrier covers part_n[] as well
    const double sseg = sg_block_sum<4>(p.sseg, red[1]);
    if (threadIdx.x < SG_OBJ_INTS) {
        const int v = part_n[0][threadIdx.x] + part_n[1][threadIdx.x] + part_n[2][threadIdx.x] + part_n[3][threadIdx.x];
        if (v) atomicAdd(&stage[threadIdx.x], (unsigned long long)v);
    }
    if (threadIdx.x == 0) {
        if (siou != 0.0) atomicAdd((double*)&stage[14], siou);
        if (sseg != 0.0) atomicAdd((double*)&stage[15], sseg);
    }
}

__global__ void sg_obj_final_kernel(const unsigned long long* stage, int64_t* acc_i, double* acc_f, int64_t* counts_out, double* sums_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double siou = ((const double*)stage)[14], sseg = ((const double*)stage)[15];
    for (int k = 0; k < 16; ++k) {
        const int64_t v = k == SGAN_OBJ_IMAGES ? 1 : k < SG_OBJ_INTS ? (int64_t)stage[k] : 0;
        if (k < SG_OBJ_INTS) acc_i[k] += v;
        else acc_i[k] = 0;
        if (counts_out) counts_out[k] = v;
    }
    acc_f[SGAN_OBJ_SIOU] += siou;
    acc_f[SGAN_OBJ_SSEG] += sseg;
    if (sums_out) {
        sums_out[SGAN_OBJ_SIOU] = siou;
        sums_out[SGAN_OBJ_SSEG] = sseg;
    }
}

extern "C" int64_t sgan_object_match_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_obj_bytes(sg_rand_layout(H, W));
}

extern "C" int sgan_object_match_accumulate(const int32_t* t_labels, const int32_t* s_labels, int32_t H, int32_t W, int32_t min_area,
                                            void* workspace, int64_t workspace_bytes, int64_t* acc_i, double* acc_f, int64_t* counts_out,
                                            double* sums_out, int32_t* dev_err, void* stream) {
    SGAN_CHECK(t_labels && s_labels && workspace && acc_i && acc_f && dev_err, "null pointer");
    SGAN_CHECK(H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30), "bad shape %d x %d", H, W);
    SGAN_CHECK(min_area >= 1, "min_area = %d (>= 1)", min_area);
    const SgRandLayout l = sg_rand_layout(H, W);
    const int64_t need = sg_obj_bytes(l);
    SGAN_CHECK(workspace_bytes >= need, "workspace of %lld bytes, %lld needed for %d x %d (sgan_object_match_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)need, H, W);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    const int64_t waves = (int64_t)H * ((W + 63) / 64);
    SGAN_CHECK((waves + 3) / 4 < (1ll << 31), "too many rows");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* stage = (unsigned long long*)workspace;
    unsigned long long* keys = stage + SG_OBJ_STAGE / 8;
    int* cnt_a = (int*)(keys + l.slots);
    int* cnt_b = cnt_a + l.np;
    int* cnt_ab = cnt_b + l.np;
    const int64_t z16 = need / 16, n16 = (2 * l.np + l.slots) / 4;
    hipLaunchKernelGGL(sg_zero16_kernel, dim3((unsigned)((z16 + 255) / 256 < 2048 ? (z16 + 255) / 256 : 2048)), dim3(256), 0, st,
                       (uint4*)workspace, z16);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_obj_count_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, t_labels, s_labels, H, W, keys, cnt_a, cnt_b,
                       cnt_ab, l.log2_slots, dev_err);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_obj_eval_kernel, dim3((unsigned)sg_vinfo_grid(n16)), dim3(256), 0, st, (const uint4*)cnt_a, n16, l.np,
                       (const unsigned long long*)keys, min_area, stage);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_obj_final_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)stage, acc_i, acc_f, counts_out, sums_out);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_obj_eval_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Confusion matrix: a histogram of (truth, prediction) pairs, k <= 17 classes.  Per workgroup in LDS, then one 64-bit atomic add per
// non-empty bin.
// ------------------------------------------------------------------------------------------------------------------------------
#define SG_CONF_MAX_K 17

// argmax as torch.argmax: the first maximum, a NaN beats every number
__device__ __forceinline__ void sg_argmax_step(float v, int c, float& best, int& arg) {
    if (v > best || (v != v && best == best)) {
        best = v;
        arg = c;
    }
}

__device__ __forceinline__ int sg_argmax_channels(const float* __restrict__ v, int C, bool add_background) {
    float best = v[0], sum = v[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        sg_argmax_step(v[c], c, best, arg);
        sum += v[c];
    }
    if (add_background) sg_argmax_step(1.0f - (sum > 1.0f ? 1.0f : sum), C, best, arg);      // a NaN sum stays NaN, as torch.clamp
    return arg;
}

__global__ __launch_bounds__(256) void sg_confusion_kernel(const float* __restrict__ x, int x_ld, int C, const int64_t* __restrict__ label,
                                                           const float* __restrict__ y, int y_ld, int add_background, int64_t npix,
                                                           unsigned long long* conf, int32_t* dev_err) {
    __shared__ int hist[SG_CONF_MAX_K * SG_CONF_MAX_K];
    const int k = C + (add_background ? 1 : 0);
    for (int b = threadIdx.x; b < k * k; b += 256) hist[b] = 0;
    SG_SYNC();      // hist[] zero
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
        const int pred = sg_argmax_channels(x + p * x_ld, C, add_background != 0);
        int64_t truth = label ? label[p] : (int64_t)sg_argmax_channels(y + p * y_ld, C, add_background != 0);
        if (truth < 0 || truth >= k) {
            sg_flag(dev_err, 8);
            continue;
        }
        atomicAdd(&hist[(int)truth * k + pred], 1);
    }
    SG_SYNC();      // hist[] complete
    for (int b = threadIdx.x; b < k * k; b += 256)
        if (hist[b]) atomicAdd(&conf[b], (unsigned long long)hist[b]);
}

extern "C" int sgan_confusion_accumulate(const float* x, int32_t x_ld, int32_t C, const int64_t* label, const float* y, int32_t y_ld,
                                         int32_t add_background, int64_t npix, int64_t* conf, int32_t* dev_err, void* stream) {
    SGAN_CHECK(x && conf && dev_err, "null pointer");
    SGAN_CHECK((label != nullptr) != (y != nullptr), "exactly one of label and y");
    SGAN_CHECK(C >= 1 && C <= 16 && x_ld >= C && (label || y_ld >= C), "C = %d (1..16), x_ld = %d, y_ld = %d", C, x_ld, y_ld);
    SGAN_CHECK(npix >= 1 && npix < (1ll << 31), "npix = %lld", (long long)npix);      // a workgroup's int bins cannot overflow
    const int64_t want = (npix + 255) / 256;
    hipLaunchKernelGGL(sg_confusion_kernel, dim3((unsigned)(want < 512 ? want : 512)), dim3(256), 0, (hipStream_t)stream, x, x_ld, C, label,
                       y, y_ld, add_background, npix, (unsigned long long*)conf, dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_confusion_kernel";
    return SGAN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Guo-Hall thinning of the wall pixels (skimage.morphology.thin; util.thin is the host restatement).  An iteration is two
// sub-iterations; each decides every wall pixel from ONE snapshot of its eight neighbours and then deletes, so a pixel after s
// sub-iterations depends on the pixels at most s away.  A workgroup holds a tile with a halo of SG_THIN_K pixels in LDS and runs up
// to SG_THIN_K sub-iterations on it: after sub-iteration s the outermost s rings of the region may be wrong (their neighbours outside
// the region were not known), the rest is exact, and the core is what it writes back.  Sub-iteration s therefore touches only the
// rings >= s + 1, which are all the later ones read.  Two byte masks in the workspace are ping-ponged between launches, because a
// tile's halo is its neighbours' state BEFORE the launch.
// Nothing is decided on the host: a call enqueues init, a fixed number of step launches and emit.  Convergence is carried by
// cnt[i] = pixels deleted in iteration i (core pixels only, so the tiles' counts add up to the image's), zeroed by init; a step
// launch whose predecessor's last iteration deleted nothing returns at once and leaves its destination mask untouched, and emit
// derives from the counters how many launches ran, which tells it the mask that is live.  The counters cross launch boundaries only,
// so plain loads read them.
// Workspace: [cnt: budget int32, rounded up to 16 bytes][mask 0: H W bytes, rounded up to 16][mask 1: likewise].
// ------------------------------------------------------------------------------------------------------------------------------
#define SG_THIN_K 16                                  // halo = sub-iterations per launch (even); 16 against 8 measured in DESIGN.md R11
#define SG_THIN_TH 32                                 // core rows of a tile
#define SG_THIN_RW 64                                 // region width: one wave holds one row of the region
#define SG_THIN_TW (SG_THIN_RW - 2 * SG_THIN_K)       // core columns of a tile
#define SG_THIN_RH (SG_THIN_TH + 2 * SG_THIN_K)
#define SG_THIN_IPL (SG_THIN_K / 2)                   // iterations per launch
#define SG_THIN_THREADS 256
static_assert(SG_THIN_K >= 2 && SG_THIN_K % 2 == 0 && SG_THIN_TW >= 8, "SG_THIN_K: even, and a core of at least 8 columns");

static int sg_thin_budget(int32_t H, int32_t W) { return (H < W ? H : W) / 2 + 2; }

// c: the neighbour code, bit k = b[k], b0..b7 = E, NE, N, NW, W, SW, S, SE (counter-clockwise from E).  The conditions as util.thin_tables
// states them, on the code rotated by one and two places: bit i of r1 is b[(i+1)%8], of r2 b[(i+2)%8], of l1 b[(i+7)%8].
__device__ __forceinline__ bool sg_thin_deletable(unsigned c, int second) {
    const unsigned r1 = ((c >> 1) | (c << 7)) & 255u, r2 = ((c >> 2) | (c << 6)) & 255u, l1 = ((c << 1) | (c >> 7)) & 255u;
    if (__builtin_popcount(~c & (r1 | r2) & 0x55u) != 1) return false;                                    // G1
    const int n1 = __builtin_popcount((c | l1) & 0xAAu), n2 = __builtin_popcount((c | r1) & 0xAAu);      // k odd: b[k] | b[k-1], b[k] | b[k+1]
    const int m = n1 < n2 ? n1 : n2;
    if (m != 2 && m != 3) return false;                                                                   // G2
    if (second) return !(((c & 0x60u) || !(c & 0x08u)) && (c & 0x10u));                                   // G3': not ((b5 | b6 | !b3) & b4)
    return !(((c & 0x06u) || !(c & 0x80u)) && (c & 0x01u));                                               // G3:  not ((b1 | b2 | !b7) & b0)
}

__global__ __launch_bounds__(256) void sg_thin_init_kernel(const float* __restrict__ plane, int64_t pix_stride, int n, uint8_t* __restrict__ mask,
                                                           int32_t* __restrict__ cnt, int iters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    for (int j = i; j < iters; j += gridDim.x * 256) cnt[j] = 0;
    if (i < n) mask[i] = plane[(int64_t)i * pix_stride] > 0.5f ? 1 : 0;
}

// Iterations it0 .. it0 + nit - 1 (nit <= SG_THIN_IPL) of the tile at (blockIdx.x, blockIdx.y): src -> dst.
__global__ __launch_bounds__(SG_THIN_THREADS) void sg_thin_step_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                                       int32_t* cnt, int it0, int nit) {
    if (it0 > 0 && cnt[it0 - 1] == 0) return;      // converged before this launch (uniform over the grid): dst stays as it is
    __shared__ uint8_t M[2][SG_THIN_RH * SG_THIN_RW];
    __shared__ int deleted[SG_THIN_IPL];
    const int tid = threadIdx.x;
    const int cx0 = blockIdx.x * SG_THIN_TW, cy0 = blockIdx.y * SG_THIN_TH;
    for (int p = tid; p < SG_THIN_RH * SG_THIN_RW; p += SG_THIN_THREADS) {
        const int y = cy0 - SG_THIN_K + p / SG_THIN_RW, x = cx0 - SG_THIN_K + p % SG_THIN_RW;
        M[0][p] = (y >= 0 && y < H && x >= 0 && x < W) ? src[y * W + x] : (uint8_t)0;      // outside the image: 0
    }
    if (tid < SG_THIN_IPL) deleted[tid] = 0;
    SG_SYNC();      // the region and deleted[] are in place
    const int rx = tid % SG_THIN_RW;
    for (int s = 0; s < 2 * nit; ++s) {
        const uint8_t* a = M[s & 1];
        uint8_t* b = M[(s & 1) ^ 1];
        const int lo = s + 1;      // rings 0 .. s are not needed any more
        int del = 0;
        if (rx >= lo && rx < SG_THIN_RW - lo) {
            for (int ry = lo + tid / SG_THIN_RW; ry < SG_THIN_RH - lo; ry += SG_THIN_THREADS / SG_THIN_RW) {      // uniform over a wave
                const int p = ry * SG_THIN_RW + rx;
                uint8_t v = a[p];
                if (v) {
                    const unsigned c = (unsigned)a[p + 1] | (unsigned)a[p - SG_THIN_RW + 1] << 1 | (unsigned)a[p - SG_THIN_RW] << 2 |
                                       (unsigned)a[p - SG_THIN_RW - 1] << 3 | (unsigned)a[p - 1] << 4 | (unsigned)a[p + SG_THIN_RW - 1] << 5 |
                                       (unsigned)a[p + SG_THIN_RW] << 6 | (unsigned)a[p + SG_THIN_RW + 1] << 7;
                    if (sg_thin_deletable(c, s & 1)) {
                        v = 0;
                        if (rx >= SG_THIN_K && rx < SG_THIN_RW - SG_THIN_K && ry >= SG_THIN_K && ry < SG_THIN_RH - SG_THIN_K) ++del;
                    }
                }
                b[p] = v;
            }
        }
        if (del) atomicAdd(&deleted[s >> 1], del);
        SG_SYNC();      // sub-iteration s is complete in b, and nobody reads a any more: the next one overwrites it
    }
    const uint8_t* f = M[(2 * nit) & 1];
    for (int p = tid; p < SG_THIN_TH * SG_THIN_TW; p += SG_THIN_THREADS) {
        const int cy = p / SG_THIN_TW, cx = p % SG_THIN_TW, y = cy0 + cy, x = cx0 + cx;
        if (y < H && x < W) dst[y * W + x] = f[(cy + SG_THIN_K) * SG_THIN_RW + cx + SG_THIN_K];
    }
    if (tid < nit && deleted[tid]) atomicAdd(&cnt[it0 + tid], deleted[tid]);
}

// Step launch j >= 1 ran iff cnt[j * SG_THIN_IPL - 1] > 0; with `ran` launches run in all the live mask is number ran & 1.
__global__ __launch_bounds__(256) void sg_thin_emit_kernel(const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1,
                                                           const int32_t* __restrict__ cnt, int iters, int n, float* __restrict__ out,
                                                           int32_t* iters_out, int flag_short, int32_t* dev_err) {
    __shared__ int ran, changing;
    if (threadIdx.x == 0) {
        ran = 1;
        changing = 0;
    }
    SG_SYNC();      // the two counts initialised
    for (int i = threadIdx.x; i < iters; i += 256) {
        if (cnt[i] > 0) {
            atomicAdd(&changing, 1);
            if ((i + 1) % SG_THIN_IPL == 0 && i + 1 < iters) atomicAdd(&ran, 1);
        }
    }
    SG_SYNC();      // the two counts complete
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (iters_out) *iters_out = changing;
        if (flag_short && cnt[iters - 1] > 0) sg_flag(dev_err, 16);      // the budget's last iteration still deleted something
    }
    const uint8_t* live = (ran & 1) ? m1 : m0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = live[i] ? 1.0f : 0.0f;
}

struct SgThinLayout {
    int budget;
    int64_t cnt_bytes, mask_bytes, bytes;
};

static SgThinLayout sg_thin_layout(int32_t H, int32_t W) {
    SgThinLayout l;
    l.budget = sg_thin_budget(H, W);
    l.cnt_bytes = (4ll * l.budget + 15) & ~15ll;
    l.mask_bytes = ((int64_t)H * W + 15) & ~15ll;
    l.bytes = l.cnt_bytes + 2 * l.mask_bytes;
    return l;
}

// the shapes both entries take: H W < 2^30, and no more tile rows than a grid has in y
static bool sg_thin_shape_ok(int32_t H, int32_t W) {
    return H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 30) && (H + SG_THIN_TH - 1) / SG_THIN_TH <= 65535;
}

extern "C" int64_t sgan_thin_workspace(int32_t H, int32_t W) {
    if (!sg_thin_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_thin_layout(H, W).bytes;
}

extern "C" int sgan_thin(const float* plane, int64_t pix_stride, int32_t H, int32_t W, float* out, int32_t max_num_iter, void* workspace,
                         int64_t workspace_bytes, int32_t* iters_out, int32_t* dev_err, void* stream) {
    SGAN_CHECK(plane && out && workspace && dev_err, "null pointer");
    SGAN_CHECK(sg_thin_shape_ok(H, W) && pix_stride >= 1, "bad shape %d x %d, pixel stride %lld", H, W, (long long)pix_stride);
    const SgThinLayout l = sg_thin_layout(H, W);
    SGAN_CHECK(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_thin_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)l.bytes, H, W);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0, "workspace not 16-byte aligned");
    const dim3 tiles((W + SG_THIN_TW - 1) / SG_THIN_TW, (H + SG_THIN_TH - 1) / SG_THIN_TH);
    // "until nothing changes" runs the budget; a max_num_iter beyond the budget is cut to it, and reported like the former if it was short
    const int iters = (max_num_iter > 0 && max_num_iter < l.budget) ? max_num_iter : l.budget;
    const int flag_short = (max_num_iter <= 0 || max_num_iter > l.budget) ? 1 : 0;
    int32_t* cnt = (int32_t*)workspace;
    uint8_t* mask[2] = {(uint8_t*)workspace + l.cnt_bytes, (uint8_t*)workspace + l.cnt_bytes + l.mask_bytes};
    const int n = H * W, nb = (n + 255) / 256;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_thin_init_kernel, dim3(nb), dim3(256), 0, st, plane, pix_stride, n, mask[0], cnt, iters);
    SGAN_LAUNCH_CHECK();
    int j = 0;
    for (int it0 = 0; it0 < iters; it0 += SG_THIN_IPL, ++j) {
        const int nit = iters - it0 < SG_THIN_IPL ? iters - it0 : SG_THIN_IPL;
        hipLaunchKernelGGL(sg_thin_step_kernel, tiles, dim3(SG_THIN_THREADS), 0, st, (const uint8_t*)mask[j & 1], mask[(j + 1) & 1], H, W, cnt,
                           it0, nit);
        SGAN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sg_thin_emit_kernel, dim3(nb), dim3(256), 0, st, (const uint8_t*)mask[0], (const uint8_t*)mask[1], (const int32_t*)cnt,
                       iters, n, out, iters_out, flag_short, dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_thin_step_kernel";
    return SGAN_OK;
}
