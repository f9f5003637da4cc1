// Region shape statistics on the device (include/sgan_hip.h, "region statistics"): one row of exact integers per connected region of
// a label map in sgan_ccl_label's form, appended to a caller-owned table in scipy.ndimage.label's order.  A driver measures any number
// of images into one table and reads it back once.
//
// Latency- and atomic-bound like the other metric kernels (sgan_metrics.hip), and under the same three rules: every loop has a bound
// that does not depend on other threads; what workgroups tell each other inside one launch goes through agent-scope atomics, and
// everything else crosses a launch boundary; the results are integers, so the order the atomics arrive in does not matter.
//
// Five launches, whose grids depend on (H, W) only:
//   flags    a root is a pixel with labels[p] == p + 1; every scan block of SG_RS_BLOCK pixels counts its roots
//   offsets  ONE workgroup: exclusive scan of the block counts in place, the region count R, and a copy of the caller's cursor
//   rank     every scan block again: the exclusive prefix sum over the flags (rank[p] = roots before p = the region's dense rank,
//            which is scipy's number - 1), and each root initialises its own staging row -- initialisation costs R rows, not capacity
//   count    a workgroup holds 64 x 4 pixels; a wave merges its 64 pixels by label, the four waves merge in an LDS table, and the
//            workgroup adds each region it met to that region's staging row ONCE
//   emit     staging rows -> table rows at the cursor; one thread advances the cursor
// Workspace: [R, cursor[0], cursor[1], 0: 4 int32][block counts: nb int32, padded to 16 bytes][rank: H W int32, padded][staging:
// ceil(H/2) ceil(W/2) rows of 16 int64 -- an 8-connected map has no more regions than that].
#include "sgan_common.h"

#define SG_RS_BLOCK 1024           // pixels per scan block: 256 threads x 4 consecutive pixels
#define SG_RS_COLS SGAN_REGION_COLS
#define SG_RS_SLOTS 512            // LDS table of a count workgroup: at most 256 distinct labels among its 256 pixels
#define SG_RS_FIELDS 12
#define SG_RS_ERR_LABELS 4         // a map that is not in sgan_ccl_label's form (the bit the Rand kernels raise for a label out of range)
#define SG_RS_ERR_FULL 32

__device__ __forceinline__ void sg_rs_flag(int32_t* dev_err, int code) {
    __hip_atomic_fetch_or(dev_err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SgRegionLayout {
    int64_t n, nb, max_regions;
    int64_t off_bsum, off_rank, off_stage, bytes;
};

// Beyond sgan_ccl_label's H W < 2^30: H, W <= 65536, so that sum x^2, sum y^2 and sum xy of a region stay below 2^62.
static bool sg_rs_shape_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && (int64_t)H * W < (1ll << 30); }

static SgRegionLayout sg_rs_layout(int32_t H, int32_t W) {
    SgRegionLayout l;
    l.n = (int64_t)H * W;
    l.nb = (l.n + SG_RS_BLOCK - 1) / SG_RS_BLOCK;
    l.max_regions = (int64_t)((H + 1) / 2) * ((W + 1) / 2);
    l.off_bsum = 16;
    l.off_rank = l.off_bsum + ((4 * l.nb + 15) & ~15ll);
    l.off_stage = l.off_rank + ((4 * l.n + 15) & ~15ll);
    l.bytes = l.off_stage + l.max_regions * SG_RS_COLS * 8;
    return l;
}

// Exclusive prefix sum of v over the 256 threads of a workgroup; `total` gets the sum.  part: 4 ints of LDS, free again on return.
__device__ __forceinline__ int sg_rs_block_scan(int v, int* part, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    SG_SYNC();      // the four waves' sums
    const int p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
    total = p0 + p1 + p2 + p3;
    const int before = (wave > 0 ? p0 : 0) + (wave > 1 ? p1 : 0) + (wave > 2 ? p2 : 0);
    SG_SYNC();      // part[] read by everyone: the caller may scan again
    return before + inc - v;
}

__global__ __launch_bounds__(256) void sg_rs_flags_kernel(const int32_t* __restrict__ L, int n, int32_t* __restrict__ bsum) {
    __shared__ int part[4];
    const int base = blockIdx.x * SG_RS_BLOCK + threadIdx.x * 4;
    int c = 0;
    for (int j = 0; j < 4; ++j)
        if (base + j < n && L[base + j] == base + j + 1) ++c;
    int total;
    sg_rs_block_scan(c, part, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void sg_rs_offsets_kernel(int32_t* __restrict__ bsum, int nb, int max_regions, const int32_t* __restrict__ cursor,
                                                            int32_t* __restrict__ hdr, int32_t* dev_err) {
    __shared__ int part[4];
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {      // nb <= 2^20: at most 4096 trips
        const int i = base + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int total;
        const int ex = sg_rs_block_scan(v, part, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (carry > max_regions) {      // more roots than an 8-connected map can have: not a labelling of sgan_ccl_label
            sg_rs_flag(dev_err, SG_RS_ERR_LABELS);
            carry = max_regions;
        }
        hdr[0] = carry;
        hdr[1] = cursor[0];
        hdr[2] = cursor[1];
        hdr[3] = 0;
    }
}

__global__ __launch_bounds__(256) void sg_rs_rank_kernel(const int32_t* __restrict__ L, int n, int W, const int32_t* __restrict__ bsum,
                                                         const int32_t* __restrict__ hdr, int32_t* __restrict__ rank, long long* __restrict__ stage) {
    __shared__ int part[4];
    const int base = blockIdx.x * SG_RS_BLOCK + threadIdx.x * 4;
    bool root[4];
    int c = 0;
    for (int j = 0; j < 4; ++j) {
        root[j] = base + j < n && L[base + j] == base + j + 1;
        c += root[j] ? 1 : 0;
    }
    int total;
    int r = bsum[blockIdx.x] + sg_rs_block_scan(c, part, total);
    const int R = hdr[0];
    const long long ordinal = hdr[2];
    for (int j = 0; j < 4; ++j) {
        const int p = base + j;
        if (p >= n) break;
        rank[p] = r;
        if (root[j]) {
            if (r < R) {      // R <= max_regions: inside the staging table
                const long long y = p / W;
                long long* row = stage + (int64_t)r * SG_RS_COLS;
                for (int k = 0; k < SG_RS_COLS; ++k) row[k] = 0;
                row[1] = W;           // xmin: lowered by the count pass
                row[2] = -1;          // xmax: raised
                row[3] = y;           // ymin: a root is its region's first pixel in raster order
                row[4] = y;           // ymax: raised
                row[11] = p;
                row[12] = ordinal;
            }
            ++r;
        }
    }
}

// One key of the workgroup's table.  f[]: pixels, sum dx, sum dy, sum dx^2, sum dy^2, sum dx dy, boundary pixels, exposed edges, then
// max(63 - dx), max(dx), max(3 - dy), max(dy) -- the minima as maxima of the mirrored coordinate, so that all twelve start at 0.
// dx < 64 and dy < 4 are relative to the workgroup's corner: 256 pixels keep every field in 32 bits, and LDS atomics are 32-bit.
struct SgRsSlot {
    int f[SG_RS_FIELDS];
};

__global__ __launch_bounds__(256) void sg_rs_count_kernel(const int32_t* __restrict__ L, int H, int W, const int32_t* __restrict__ rank,
                                                          const int32_t* __restrict__ hdr, long long* stage, int32_t* dev_err) {
    __shared__ int keys[SG_RS_SLOTS];
    __shared__ SgRsSlot slots[SG_RS_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, dy = tid >> 6;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4;
    const int x = x0 + lane, y = y0 + dy, n = H * W;
    for (int i = tid; i < SG_RS_SLOTS; i += 256) keys[i] = 0;
    for (int i = tid; i < SG_RS_SLOTS * SG_RS_FIELDS; i += 256) (&slots[0].f[0])[i] = 0;

    // a lane outside the image looks like wall; no wave leaves early, every one of them meets the barriers below
    int t = 0;
    const bool inside = x < W && y < H;
    if (inside) {
        t = L[y * W + x];
        if (t < 0 || t > n) {
            sg_rs_flag(dev_err, SG_RS_ERR_LABELS);
            t = 0;
        }
    }
    int tw = __shfl_up(t, 1, 64), te = __shfl_down(t, 1, 64);
    int edges = 0;
    if (t != 0) {
        if (lane == 0) tw = x > 0 ? L[y * W + x - 1] : 0;
        if (lane == 63 || x == W - 1) te = x < W - 1 ? L[y * W + x + 1] : 0;
        const int tn = y > 0 ? L[(y - 1) * W + x] : 0, ts = y < H - 1 ? L[(y + 1) * W + x] : 0;
        edges = (tw != t) + (te != t) + (tn != t) + (ts != t);
    }

    // Segmented reduction over the wave: the lanes of one label elect their first lane, which gets the label's sums; at most 64
    // rounds, one per distinct label.  The row is the same for the whole wave, so what has to be summed is the pixel count, the
    // lane numbers and their squares, the boundary flags and the edge counts: the counts come from ballots, sum dx and sum dx^2
    // (<= 2016 and <= 85344) travel packed in one word through one butterfly.
    int m_cnt = 0, m_sx = 0, m_sxx = 0, m_b = 0, m_e = 0, m_lo = 0, m_hi = 0;
    bool pending = t != 0;
    for (int it = 0; it < 64; ++it) {
        const unsigned long long waiting = __ballot(pending);
        if (waiting == 0) break;      // uniform
        const int leader = __builtin_ctzll(waiting);
        const int key = __shfl(t, leader, 64);
        const bool same = pending && t == key;
        const unsigned long long m = __ballot(same), mb = __ballot(same && edges != 0);
        const unsigned long long e0 = __ballot(same && (edges & 1)), e1 = __ballot(same && (edges & 2)), e2 = __ballot(same && (edges & 4));
        int packed = same ? ((lane * lane) << 11) | lane : 0;
        for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
        if (same) {
            pending = false;
            if (lane == leader) {
                m_cnt = __builtin_popcountll(m);
                m_sx = packed & 2047;
                m_sxx = packed >> 11;
                m_b = __builtin_popcountll(mb);
                m_e = __builtin_popcountll(e0) + 2 * __builtin_popcountll(e1) + 4 * __builtin_popcountll(e2);
                m_lo = __builtin_ctzll(m);
                m_hi = 63 - __builtin_clzll(m);
            }
        }
    }
    SG_SYNC();      // the table is zero

    // The four waves of the workgroup meet in the table: open addressing on the label, at most 256 labels in 512 slots, so a probe
    // finds its slot or a free one within SG_RS_SLOTS steps.
    if (m_cnt) {
        unsigned slot = ((unsigned)t * 2654435761u) >> 23;
        int probe = 0;
        for (; probe < SG_RS_SLOTS; ++probe) {
            const int seen = atomicCAS(&keys[slot], 0, t);
            if (seen == 0 || seen == t) break;
            slot = (slot + 1) & (SG_RS_SLOTS - 1);
        }
        if (probe < SG_RS_SLOTS) {
            int* f = slots[slot].f;
            atomicAdd(&f[0], m_cnt);
            atomicAdd(&f[1], m_sx);
            atomicAdd(&f[2], m_cnt * dy);
            atomicAdd(&f[3], m_sxx);
            atomicAdd(&f[4], m_cnt * dy * dy);
            atomicAdd(&f[5], m_sx * dy);
            atomicAdd(&f[6], m_b);
            atomicAdd(&f[7], m_e);
            atomicMax(&f[8], 63 - m_lo);
            atomicMax(&f[9], m_hi);
            atomicMax(&f[10], 3 - dy);
            atomicMax(&f[11], dy);
        } else {
            sg_rs_flag(dev_err, 1);      // cannot happen with 256 pixels; reported like every other bounded loop that ran out
        }
    }
    SG_SYNC();      // the table is complete

    const int R = hdr[0];
    for (int s = tid; s < SG_RS_SLOTS; s += 256) {
        const int key = keys[s];
        if (key == 0) continue;
        const int root = key - 1;                       // 0 <= root < n, checked at the load
        const int k = rank[root];
        if (L[root] != key || k < 0 || k >= R) {        // not a root, or beyond the rows the rank pass initialised: dropped and reported
            sg_rs_flag(dev_err, SG_RS_ERR_LABELS);
            continue;
        }
        const int* f = slots[s].f;
        const long long c = f[0], sdx = f[1], sdy = f[2], X0 = x0, Y0 = y0;
        long long* row = stage + (int64_t)k * SG_RS_COLS;
        const long long sx = c * X0 + sdx, sy = c * Y0 + sdy;
        __hip_atomic_fetch_add(&row[0], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(&row[1], X0 + 63 - f[8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&row[2], X0 + f[9], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(&row[3], Y0 + 3 - f[10], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&row[4], Y0 + f[11], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&row[5], sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&row[6], sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&row[7], c * X0 * X0 + 2 * X0 * sdx + f[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&row[8], c * Y0 * Y0 + 2 * Y0 * sdy + f[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&row[9], c * X0 * Y0 + X0 * sdy + Y0 * sdx + f[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f[6]) __hip_atomic_fetch_add(&row[10], (long long)f[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f[7]) __hip_atomic_fetch_add(&row[13], (long long)f[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One thread per value of the staging table's first R rows.  The cursor is read from the copy the offsets launch took, so the one
// thread that advances it races with nobody.
__global__ __launch_bounds__(256) void sg_rs_emit_kernel(const long long* __restrict__ stage, const int32_t* __restrict__ hdr,
                                                         long long* __restrict__ table, int capacity, int32_t* cursor, int32_t* dev_err) {
    const int R = hdr[0];
    int c0 = hdr[1];
    c0 = c0 < 0 ? 0 : (c0 > capacity ? capacity : c0);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, r = i / SG_RS_COLS;
    if (r < R && c0 + r < capacity) table[(c0 + r) * SG_RS_COLS + i % SG_RS_COLS] = stage[i];
    if (i == 0) {
        const int64_t end = (int64_t)c0 + R;
        if (end > capacity) sg_rs_flag(dev_err, SG_RS_ERR_FULL);
        cursor[0] = (int32_t)(end > capacity ? capacity : end);
        cursor[1] = hdr[2] + 1;
    }
}

extern "C" int64_t sgan_region_stats_workspace(int32_t H, int32_t W) {
    if (!sg_rs_shape_ok(H, W)) return sgan_fail(SGAN_ERR_INVALID, "bad shape %d x %d", H, W);
    return sg_rs_layout(H, W).bytes;
}

extern "C" int sgan_region_stats(const int32_t* labels, int32_t H, int32_t W, int64_t* table, int32_t capacity, int32_t* cursor,
                                 void* workspace, int64_t workspace_bytes, int32_t* dev_err, void* stream) {
    SGAN_CHECK(labels && table && cursor && workspace && dev_err, "null pointer");
    SGAN_CHECK(sg_rs_shape_ok(H, W), "bad shape %d x %d", H, W);
    SGAN_CHECK(capacity >= 1, "capacity %d", capacity);
    const SgRegionLayout l = sg_rs_layout(H, W);
    SGAN_CHECK(workspace_bytes >= l.bytes, "workspace of %lld bytes, %lld needed for %d x %d (sgan_region_stats_workspace); nothing was launched",
               (long long)workspace_bytes, (long long)l.bytes, H, W);
    SGAN_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)table & 7) == 0, "workspace not 16-byte aligned, or table not 8-byte aligned");
    int32_t* hdr = (int32_t*)workspace;
    int32_t* bsum = (int32_t*)((char*)workspace + l.off_bsum);
    int32_t* rank = (int32_t*)((char*)workspace + l.off_rank);
    long long* stage = (long long*)((char*)workspace + l.off_stage);
    const int n = (int)l.n, nb = (int)l.nb, max_regions = (int)l.max_regions;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_rs_flags_kernel, dim3(nb), dim3(256), 0, st, labels, n, bsum);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_rs_offsets_kernel, dim3(1), dim3(256), 0, st, bsum, nb, max_regions, (const int32_t*)cursor, hdr, dev_err);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_rs_rank_kernel, dim3(nb), dim3(256), 0, st, labels, n, W, (const int32_t*)bsum, (const int32_t*)hdr, rank, stage);
    SGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_rs_count_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, labels, H, W, (const int32_t*)rank,
                       (const int32_t*)hdr, stage, dev_err);
    SGAN_LAUNCH_CHECK();
    const int64_t values = l.max_regions * SG_RS_COLS;
    hipLaunchKernelGGL(sg_rs_emit_kernel, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, st, (const long long*)stage, (const int32_t*)hdr,
                       (long long*)table, capacity, cursor, dev_err);
    SGAN_LAUNCH_CHECK();
    g_sgan_last_kernel = "sg_rs_count_kernel";
    return SGAN_OK;
}
