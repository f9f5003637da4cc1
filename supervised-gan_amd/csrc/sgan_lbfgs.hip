// L-BFGS advance on the device (latent reconstruction, models/fcgan_model.py:278-302): torch.optim.LBFGS(line_search_fn=None).step
// as a state machine that consumes one closure evaluation per launch.  torch/optim/lbfgs.py reads ~2 m + 5 scalars back to the host
// per iteration (every alpha of the two-loop recursion, ys, gtd, the loss); here every decision is taken in the workgroup that owns
// the problem, so a closure plus this launch can be captured once and replayed.  The control flow is the Python reference's
// (supervised-gan_amd/lbfgs.py, _advance_one) line by line; the vectors are fp32 like torch's, the dot products accumulate in fp64.
//
// Layout: one workgroup per problem (J <= 8).  Thread i owns elements i, i + blockDim, ... of every vector of its problem, so the
// element-wise updates need no barrier; only the reductions (dots, |g|_1, max |g|) cross waves: a wave reduction by shuffles, one
// LDS slot per wave, ONE barrier, and every thread sums the slots.  The slot array is double-buffered: a reduction writes the half
// the previous one did not, and the barrier of that previous one separates the reads of the half from its next writes.
#include "sgan_common.h"

#define SG_LBFGS_MAX_WAVES 16

struct SgLbfgsRed {
    double (*slots)[SG_LBFGS_MAX_WAVES][2];
    int half;
};

__device__ __forceinline__ double sg_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double sg_wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// (a, b) summed (is_max: maximised) over the workgroup; every thread gets the result
__device__ __forceinline__ void sg_block_reduce2(SgLbfgsRed& r, double& a, double& b, bool is_max) {
    a = is_max ? sg_wave_max(a) : sg_wave_sum(a);
    b = is_max ? sg_wave_max(b) : sg_wave_sum(b);
    const int wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    double (*s)[2] = r.slots[r.half];
    if ((threadIdx.x & 63) == 0) {
        s[wid][0] = a;
        s[wid][1] = b;
    }
    SG_SYNC();
    double ra = s[0][0], rb = s[0][1];
    for (int w = 1; w < nw; ++w) {
        ra = is_max ? fmax(ra, s[w][0]) : ra + s[w][0];
        rb = is_max ? fmax(rb, s[w][1]) : rb + s[w][1];
    }
    a = ra;
    b = rb;
    r.half ^= 1;
}

__device__ __forceinline__ double sg_block_sum(SgLbfgsRed& r, double a) {
    double b = 0.0;
    sg_block_reduce2(r, a, b, false);
    return a;
}

__device__ __forceinline__ void sg_lbfgs_end_step(sgan_lbfgs_state& st, int code) {
    st.last_exit = code;
    st.steps += 1;
    st.phase = SGAN_LBFGS_PHASE_START;
    if (st.steps >= st.n_steps) st.done = 1;
}

__global__ __launch_bounds__(1024) void sg_lbfgs_advance_kernel(sgan_lbfgs_state* __restrict__ states, int64_t n, float* __restrict__ x,
                                                                int64_t x_ld, const float* __restrict__ grad, int64_t g_ld,
                                                                const float* __restrict__ loss_in, float* __restrict__ dvec,
                                                                float* __restrict__ prev_grad, float* __restrict__ hist_s,
                                                                float* __restrict__ hist_y, float* __restrict__ hist_rho, int32_t cap) {
    __shared__ double slots[2][SG_LBFGS_MAX_WAVES][2];
    __shared__ float al[SGAN_LBFGS_MAX_HISTORY];
    __shared__ float rho[SGAN_LBFGS_MAX_HISTORY];
    const int j = blockIdx.x;
    sgan_lbfgs_state st = states[j];
    // uniform over the workgroup (every thread read the same state); a history longer than the buffers is refused here as well
    if (st.done || st.history_size < 1 || st.history_size > cap) return;
    SgLbfgsRed red{slots, 0};
    const int tid = threadIdx.x, nt = blockDim.x;
    float* xj = x + (int64_t)j * x_ld;
    const float* gj = grad + (int64_t)j * g_ld;
    float* dj = dvec + (int64_t)j * n;
    float* pg = prev_grad + (int64_t)j * n;
    float* S = hist_s + (int64_t)j * cap * n;
    float* Y = hist_y + (int64_t)j * cap * n;
    float* R = hist_rho + (int64_t)j * cap;
    const int hs = st.history_size;
    const double loss = (double)loss_in[j];
    const float tol_change_f = (float)st.tolerance_change;

    double gmax = 0.0, gl1 = 0.0;
    for (int64_t i = tid; i < n; i += nt) gmax = fmax(gmax, (double)fabsf(gj[i]));
    {
        double dummy = 0.0;
        sg_block_reduce2(red, gmax, dummy, true);
    }
    const bool opt_cond = (float)gmax <= st.tolerance_grad;
    st.func_evals += 1;
    int code = 0;
    if (st.phase == SGAN_LBFGS_PHASE_START) {       // orig_loss = closure()
        st.evals_in_step = 1;
        if (opt_cond) code = SGAN_LBFGS_EXIT_OPT_START;
        else st.iter_in_step = 0;
    } else {                                        // loss = closure() after the move, then the checks that end the while body
        st.evals_in_step += 1;
        if (st.iter_in_step == st.max_iter) code = SGAN_LBFGS_EXIT_MAX_ITER;
        else if (st.evals_in_step >= st.max_eval) code = SGAN_LBFGS_EXIT_MAX_EVAL;
        else if (opt_cond) code = SGAN_LBFGS_EXIT_OPT_COND;
        else {
            double dtmax = 0.0, dummy = 0.0;
            for (int64_t i = tid; i < n; i += nt) dtmax = fmax(dtmax, (double)fabsf(dj[i] * st.t));
            sg_block_reduce2(red, dtmax, dummy, true);
            if ((float)dtmax <= tol_change_f) code = SGAN_LBFGS_EXIT_SMALL_STEP;
            else if (fabs(loss - st.prev_loss) < st.tolerance_change) code = SGAN_LBFGS_EXIT_NO_PROGRESS;
        }
    }
    if (code == 0) {
        st.iter_in_step += 1;
        st.n_iter += 1;
        double gtd = 0.0;
        if (st.n_iter == 1) {       // d = -g; empty history; H_diag = 1; prev_flat_grad = g; |g|_1 for the first step length
            st.hist_len = 0;
            st.hist_head = 0;
            st.h_diag = 1.f;
            for (int64_t i = tid; i < n; i += nt) {
                const float g = gj[i], d = -g;
                dj[i] = d;
                pg[i] = g;
                gtd += (double)(g * d);
                gl1 += (double)fabsf(g);
            }
            sg_block_reduce2(red, gtd, gl1, false);
        } else {
            // y = g - prev_g, s = d t: ys and yy first, the memory update only when ys > 1e-10
            double ys = 0.0, yy = 0.0;
            for (int64_t i = tid; i < n; i += nt) {
                const float y = gj[i] - pg[i], s = dj[i] * st.t;
                ys += (double)(y * s);
                yy += (double)(y * y);
            }
            sg_block_reduce2(red, ys, yy, false);
            const float ys_f = (float)ys;
            int len = st.hist_len, slot = -1;
            const float r_new = 1.f / ys_f;
            if (ys_f > 1e-10f) {
                if (len == hs) {            // pop the oldest: its slot takes the new pair
                    slot = st.hist_head;
                    st.hist_head = (st.hist_head + 1) % hs;
                } else {
                    slot = (st.hist_head + len) % hs;
                    len += 1;
                }
                st.hist_len = len;
                st.h_diag = ys_f / (float)yy;
                if (tid == 0) R[slot] = r_new;      // no thread reads R[slot] below: rho[len - 1] comes from r_new
            } else {
                st.n_skipped += 1;
            }
            for (int k = tid; k < len; k += nt) rho[k] = (slot >= 0 && k == len - 1) ? r_new : R[(st.hist_head + k) % hs];
            SG_SYNC();      // rho[] complete
            // q = -g (in d's storage); the new pair into its slot; first dot of the first loop
            const int newest = len - 1;
            float* Sk = newest >= 0 ? S + (int64_t)((st.hist_head + newest) % hs) * n : nullptr;
            double part = 0.0;
            for (int64_t i = tid; i < n; i += nt) {
                const float g = gj[i];
                if (slot >= 0) {
                    S[(int64_t)slot * n + i] = dj[i] * st.t;
                    Y[(int64_t)slot * n + i] = g - pg[i];
                }
                const float q = -g;
                dj[i] = q;
                if (Sk) part += (double)(Sk[i] * q);
            }
            // first loop, newest to oldest: al_k = (s_k . q) rho_k; q -= al_k y_k   (one pass per k: update, then the next dot)
            for (int k = newest; k >= 0; --k) {
                const float a = (float)sg_block_sum(red, part) * rho[k];
                if (tid == 0) al[k] = a;
                const float* Yk = Y + (int64_t)((st.hist_head + k) % hs) * n;
                const float* Sn = k > 0 ? S + (int64_t)((st.hist_head + k - 1) % hs) * n : nullptr;
                part = 0.0;
                for (int64_t i = tid; i < n; i += nt) {
                    const float q = dj[i] + (-a) * Yk[i];
                    dj[i] = q;
                    if (Sn) part += (double)(Sn[i] * q);
                }
            }
            // r = q H_diag; second loop, oldest to newest: be_k = (y_k . r) rho_k; r += (al_k - be_k) s_k
            const float hd = st.h_diag;
            const float* Y0 = len > 0 ? Y + (int64_t)(st.hist_head % hs) * n : nullptr;
            part = 0.0;
            for (int64_t i = tid; i < n; i += nt) {
                const float r = dj[i] * hd;
                dj[i] = r;
                if (Y0) part += (double)(Y0[i] * r);
            }
            SG_SYNC();      // al[] complete (written by thread 0 inside the first loop)
            for (int k = 0; k < len; ++k) {
                const float be = (float)sg_block_sum(red, part) * rho[k];
                const float c = al[k] - be;
                const float* Sk2 = S + (int64_t)((st.hist_head + k) % hs) * n;
                const float* Yn = k + 1 < len ? Y + (int64_t)((st.hist_head + k + 1) % hs) * n : nullptr;
                part = 0.0;
                for (int64_t i = tid; i < n; i += nt) {
                    const float r = dj[i] + c * Sk2[i];
                    dj[i] = r;
                    if (Yn) part += (double)(Yn[i] * r);
                }
            }
            // prev_flat_grad = g; gtd = g . d
            for (int64_t i = tid; i < n; i += nt) {
                const float g = gj[i];
                pg[i] = g;
                gtd += (double)(g * dj[i]);
            }
            gtd = sg_block_sum(red, gtd);
        }
        st.prev_loss = loss;
        if (st.n_iter == 1) {
            const float inv = 1.f / (float)gl1;
            st.t = (inv < 1.f ? inv : 1.f) * st.lr;
        } else {
            st.t = st.lr;
        }
        if ((float)gtd > -tol_change_f) {
            code = SGAN_LBFGS_EXIT_GTD;
        } else {
            const float t = st.t;
            for (int64_t i = tid; i < n; i += nt) xj[i] = xj[i] + t * dj[i];
            if (st.iter_in_step != st.max_iter) st.phase = SGAN_LBFGS_PHASE_AFTER_MOVE;
            else code = SGAN_LBFGS_EXIT_MAX_ITER;       // no re-evaluation after the max_iter-th move
        }
    }
    if (code) sg_lbfgs_end_step(st, code);
    SG_SYNC();      // every thread has read states[j] (and R[] / rho[]) before thread 0 writes
    if (tid == 0) states[j] = st;
}

extern "C" int sgan_lbfgs_advance(sgan_lbfgs_state* state, int32_t J, int64_t n, float* x, int64_t x_ld, const float* grad, int64_t g_ld,
                                  const float* loss, float* d, float* prev_grad, float* hist_s, float* hist_y, float* hist_rho,
                                  int32_t history_cap, void* stream) {
    SGAN_CHECK(state && x && grad && loss && d && prev_grad && hist_s && hist_y && hist_rho, "null pointer");
    SGAN_CHECK(J >= 1 && J <= SGAN_LBFGS_MAX_PROBLEMS && n >= 1 && x_ld >= n && g_ld >= n, "bad shape");
    SGAN_CHECK(history_cap >= 1 && history_cap <= SGAN_LBFGS_MAX_HISTORY, "history_cap out of range");
    const int threads = n <= 4096 ? 256 : 1024;
    static_assert(1024 / 64 <= SG_LBFGS_MAX_WAVES, "reduction slots");
    static_assert(sizeof(sgan_lbfgs_state) == 128, "state layout");
    hipLaunchKernelGGL(sg_lbfgs_advance_kernel, dim3(J), dim3(threads), 0, (hipStream_t)stream, state, n, x, x_ld, grad, g_ld, loss, d,
                       prev_grad, hist_s, hist_y, hist_rho, history_cap);
    SGAN_LAUNCH_CHECK();
    return SGAN_OK;
}
