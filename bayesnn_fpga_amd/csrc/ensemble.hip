// The exit ensemble as a predictor of its own (bmi_ensemble_moments, bmi_forward_mcd_ensemble, bmi_finalize_ensemble): the reference's
// cumulative mean of the exits' softmax outputs, formed PER STOCHASTIC PASS (SA/train/loss/base_classes.py:41,54,58: `ensemble +=
// softmax(logits)` inside one forward) and then treated like any other Monte-Carlo predictor.  On per-sample logits [t][E][B][C]
// (bmi_forward_mcd_samples' layout), all in float64 and without fused multiply-adds:
//     z_te = (double) fl32(l_te * inv_e)             inv_e = float32(1 / tau_e), the ONE rounded fp32 product of the tempered head (1: off)
//     p_te = softmax_c(z_te)                         max-subtracted
//     q_te = (p_t0 + ... + p_te) / (e + 1)           summed in exit order, divided once
//     Q1[e][b][c] += q      Q2[e][b][c] += q * q      QH[e][b] += -sum_c q log q   (0 log 0 = 0, class order)
// The exits of one pass share the trunk's dropout draw, so the second moment of q holds cross-exit terms that no per-exit sum contains:
// it has to be formed per sample (train/uncertainty.py: decompose_ensemble_logits is the host restatement).
//
//   workgroup = one image, 256 threads; the samples of the launch go through LDS in chunks of TS samples (what fits), in sample order.
//   phase A     a group of L = min(64, pow2 >= C) lanes per softmax row (sample, exit): running max in fp32 (the logits ARE fp32), the
//               float64 exponentials to LDS ([row][C | 1]: an odd stride, lanes of phase C walk different rows at one class), their sum
//               by shuffle butterfly inside the group — a fixed tree, the same for every row wherever the row sits in a launch.
//   phase B     a thread per (sample, class) walks the exits: p = exp / sum, running sum, q = sum / (e + 1) over the exponential in
//               place, q log q beside it.
//   phase C     a thread per row adds its q log q in class order; then a thread per (exit, class) LOADS the running Q1 / Q2, adds the
//               chunk's samples in sample order and stores them, a thread per exit does the same for QH.  No floating-point atomics, and
//               the sums are the same bits however the samples were split into launches: every launch continues the one running sum.
#include <algorithm>
#include <cmath>

#include "kernels.h"

#define ENS_THREADS 256
#define ENS_SLAB 3456            // float64 entries of each of the two staged arrays (27 KB each)
#define ENS_ROWS 512             // (sample, exit) rows per staged chunk, at most

struct EnsTau { float inv[BMI_ENS_MAX_EXITS]; };

// ROWS (bmi_forward_mcd_adaptive_ensemble, bmi_forward_mcd_exit_staged_ensemble): workgroup i works on image b = list[i] of the B-image
// batch (list null: b = i) and on its first n_e[b] exits only (n_e null: all E) — the running exit sum is cut there, so the rows
// e < n_e[b] are the full form's bits; `logits` and the sums keep the ORIGINAL image index, rows of other images and of later exits are
// neither read nor written.  Both lookups are the same for the whole workgroup.  Not ROWS: the code as it was.
// WEIGHTED (bmi_engine_set_ensemble_weights, bmi_ensemble_moments_weighted): q_te = ((W[e][0] p_t0 + W[e][1] p_t1) + ...) + W[e][e] p_te,
// W device float64 [E_all][E_all] row-major, used as given (no renormalisation): every product rounded, added in exit order from 0.0.
// Phase B first turns the rows of pq into p in place, then forms q_e for e DESCENDING: row e reads the rows i <= e, which are still p.
// e and i are the same for the whole wave, so a weight is one scalar load (the 63.6 KB of LDS leave no room for a [32][32] table); under
// ROWS only the rows e < n_e[b] of W are read.  Not WEIGHTED: the code as it was, W is never read.
// VEC (bmi_engine_set_vector_scaling, bmi_ensemble_moments_vector): z_te,c = (double) fl32(fl32(l * vs[e][c]) + vb[e][c]), the vector-scaled head's
// own number (two rounded fp32 operations: plain operators under this body's `fp contract(off)`), in place of fl32(l * inv_e); vs / vb are device fp32 [E_all][C], read where they are used (the static LDS is full: 3.2 KB at
// E = 4, C = 100 are cache hits after the first row).  Not VEC: the code as it was, vs / vb are never read.
// MAP == 2 (bmi_engine_set_matrix_scaling, bmi_ensemble_moments_matrix): z_te,c = (double) fl32((..(fl32(M[e][c][0] * l_0) + fl32(M[e][c][1] * l_1))
// + ..) + vb[e][c]), j ascending, every operation rounded — the matrix-scaled head's own number; vs = M, device fp32 [E_all][C][C].  Formed ONCE
// per row, by the lane that owns class c, and parked (exactly, as a float64) in the row's slot of ql, which phase B overwrites later; the
// row of M is read through L1, the logits straight from the caller's array (a row is C floats: cache hits after the first class).
// The body of the kernels below: the vector and the matrix forms are kernels of their own name and arguments, so that the four older ones keep theirs.
template <bool ROWS, bool WEIGHTED, int MAP>
__device__ __forceinline__ void ensemble_moments_body(const float* __restrict__ logits, int T, int E_all, int B, int C, int CS, int TS, int L,
                                                      const EnsTau& tau, double* __restrict__ Q1, double* __restrict__ Q2, double* __restrict__ QH,
                                                      const int* __restrict__ list, const int* __restrict__ n_e, const double* __restrict__ W,
                                                      const float* __restrict__ vs, const float* __restrict__ vb) {
#pragma clang fp contract(off)
    constexpr bool VEC = MAP == 1;
    __shared__ double pq[ENS_SLAB];                      // [row][CS], row = tl * E + e: exp(z - max), then q
    __shared__ double ql[ENS_SLAB];                      // q log q
    __shared__ double row_sum[ENS_ROWS], row_h[ENS_ROWS];
    __shared__ float inv_s[BMI_ENS_MAX_EXITS];
    const int tid = threadIdx.x;
    const int b = (ROWS && list) ? list[blockIdx.x] : (int)blockIdx.x;
    const int E = (ROWS && n_e) ? min(n_e[b], E_all) : E_all;       // the exits of THIS image (rows of the chunk: [tl][E])
    if (ROWS && (E < 1 || (unsigned)b >= (unsigned)B)) return;       // (the whole workgroup)
    const int lane = tid & (L - 1), grp = tid / L, ngrp = ENS_THREADS / L;
    if (MAP == 0 && tid < E) inv_s[tid] = tau.inv[tid];
    for (int t0 = 0; t0 < T; t0 += TS) {
        const int tn = min(TS, T - t0);
        const int rows = tn * E;                         // <= ENS_ROWS, rows * CS <= ENS_SLAB (the launcher's TS)
        __syncthreads();                                 // the previous chunk's readers are done (first chunk: inv_s is written)
        for (int r0 = 0; r0 < rows; r0 += ngrp) {        // (every lane walks every step: the shuffles below need whole groups)
            const int r = r0 + grp;
            const bool live = r < rows;
            const int tl = live ? r / E : 0, e = live ? r - tl * E : 0;
            const float* src = logits + (((size_t)(t0 + tl) * E_all + e) * B + b) * C;
            if constexpr (MAP == 2) {
                const float* const mat = vs + (size_t)e * C * C;
                const float* const bi = vb + (size_t)e * C;
                float mx = -INFINITY;
                if (live)
                    for (int c = lane; c < C; c += L) {
                        const float* const mrow = mat + (size_t)c * C;
                        float acc = mrow[0] * src[0];
                        for (int j = 1; j < C; ++j) {
                            const float prod = mrow[j] * src[j];
                            acc = acc + prod;
                        }
                        const float z = acc + bi[c];
                        ql[r * CS + c] = (double)z;
                        mx = fmaxf(mx, z);
                    }
                for (int m = L >> 1; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
                double s = 0.0;
                if (live)
                    for (int c = lane; c < C; c += L) {
                        const double ex = exp(ql[r * CS + c] - (double)mx);
                        pq[r * CS + c] = ex;
                        s += ex;
                    }
                for (int m = L >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m);
                if (live && lane == 0) row_sum[r] = s;
                continue;
            }
            const float inv = VEC ? 1.f : inv_s[e];
            const float* const sc = VEC ? vs + (size_t)e * C : nullptr;
            const float* const bi = VEC ? vb + (size_t)e * C : nullptr;
            float mx = -INFINITY;
            if (live)
                for (int c = lane; c < C; c += L) mx = fmaxf(mx, VEC ? (src[c] * sc[c] + bi[c]) : src[c] * inv);
            for (int m = L >> 1; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
            double s = 0.0;
            if (live)
                for (int c = lane; c < C; c += L) {
                    const double ex = exp((double)(VEC ? (src[c] * sc[c] + bi[c]) : src[c] * inv) - (double)mx);
                    pq[r * CS + c] = ex;
                    s += ex;
                }
            for (int m = L >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (live && lane == 0) row_sum[r] = s;
        }
        __syncthreads();
        for (int i = tid; i < tn * C; i += ENS_THREADS) {
            const int tl = i / C, c = i - tl * C;
            if (WEIGHTED) {
                double* col = pq + tl * E * CS + c;          // this thread's (sample, class) column: element e at col[e * CS]
                for (int e = 0; e < E; ++e) col[e * CS] = col[e * CS] / row_sum[tl * E + e];
                for (int e = E - 1; e >= 0; --e) {
                    const double* w = W + (size_t)e * E_all;
                    double q = 0.0;
                    for (int x = 0; x <= e; ++x) q = q + w[x] * col[x * CS];
                    col[e * CS] = q;
                    ql[(tl * E + e) * CS + c] = q > 0.0 ? q * log(q) : (q == q ? 0.0 : q);
                }
                continue;
            }
            double acc = 0.0;
            for (int e = 0; e < E; ++e) {
                const int r = tl * E + e;
                acc += pq[r * CS + c] / row_sum[r];
                const double q = acc / (double)(e + 1);
                pq[r * CS + c] = q;
                ql[r * CS + c] = q > 0.0 ? q * log(q) : (q == q ? 0.0 : q);      // (a NaN stays a NaN)
            }
        }
        __syncthreads();
        for (int r = tid; r < rows; r += ENS_THREADS) {
            const double* row = ql + r * CS;
            double h = 0.0;
            for (int c = 0; c < C; ++c) h += row[c];
            row_h[r] = -h;
        }
        __syncthreads();
        for (int i = tid; i < E * C + E; i += ENS_THREADS) {
            if (i < E * C) {
                const int e = i / C, c = i - e * C;
                const size_t o = ((size_t)e * B + b) * C + c;
                double s1 = Q1[o], s2 = Q2[o];
                for (int tl = 0; tl < tn; ++tl) {
                    const double q = pq[(tl * E + e) * CS + c];
                    s1 += q;
                    s2 += q * q;
                }
                Q1[o] = s1;
                Q2[o] = s2;
            } else {
                const int e = i - E * C;
                double sh = QH[(size_t)e * B + b];
                for (int tl = 0; tl < tn; ++tl) sh += row_h[tl * E + e];
                QH[(size_t)e * B + b] = sh;
            }
        }
    }
}

template <bool ROWS, bool WEIGHTED>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_moments_kernel(const float* __restrict__ logits, int T, int E_all, int B, int C, int CS,
                                                                       int TS, int L, EnsTau tau, double* __restrict__ Q1,
                                                                       double* __restrict__ Q2, double* __restrict__ QH,
                                                                       const int* __restrict__ list, const int* __restrict__ n_e,
                                                                       const double* __restrict__ W) {
    ensemble_moments_body<ROWS, WEIGHTED, 0>(logits, T, E_all, B, C, CS, TS, L, tau, Q1, Q2, QH, list, n_e, W, nullptr, nullptr);
}

template <bool ROWS, bool WEIGHTED>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_moments_vec_kernel(const float* __restrict__ logits, int T, int E_all, int B, int C, int CS,
                                                                           int TS, int L, const float* __restrict__ vs,
                                                                           const float* __restrict__ vb, double* __restrict__ Q1,
                                                                           double* __restrict__ Q2, double* __restrict__ QH,
                                                                           const int* __restrict__ list, const int* __restrict__ n_e,
                                                                           const double* __restrict__ W) {
    ensemble_moments_body<ROWS, WEIGHTED, 1>(logits, T, E_all, B, C, CS, TS, L, EnsTau{}, Q1, Q2, QH, list, n_e, W, vs, vb);
}

template <bool ROWS, bool WEIGHTED>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_moments_mat_kernel(const float* __restrict__ logits, int T, int E_all, int B, int C, int CS,
                                                                           int TS, int L, const float* __restrict__ mat,
                                                                           const float* __restrict__ mb, double* __restrict__ Q1,
                                                                           double* __restrict__ Q2, double* __restrict__ QH,
                                                                           const int* __restrict__ list, const int* __restrict__ n_e,
                                                                           const double* __restrict__ W) {
    ensemble_moments_body<ROWS, WEIGHTED, 2>(logits, T, E_all, B, C, CS, TS, L, EnsTau{}, Q1, Q2, QH, list, n_e, W, mat, mb);
}

bool ensemble_takes(int E, int C) {
    return E >= 1 && C >= 1 && E <= BMI_ENS_MAX_EXITS && C <= BMI_ENS_MAX_CLASSES && E * (C | 1) <= ENS_SLAB;
}

// One of the twelve kernels: the vector form (MAP 1) and the matrix form (MAP 2) take their two coefficient arrays where the tempered form
// (MAP 0) takes the table of inverses
template <int MAP, bool ROWS, bool WEIGHTED>
static void launch_ens(unsigned grid, hipStream_t s, const float* logits, int T, int E, int B, int C, int CS, int TS, int L, const Calibration& cal,
                       const EnsTau& tau, const EnsRows& rows, double* Q1, double* Q2, double* QH) {
    if constexpr (MAP == 2)
        hipLaunchKernelGGL((ensemble_moments_mat_kernel<ROWS, WEIGHTED>), dim3(grid), dim3(ENS_THREADS), 0, s, logits, T, E, B, C, CS, TS, L,
                           cal.mat, cal.mat_bias, Q1, Q2, QH, rows.list, rows.n_e, cal.ens_w);
    else if constexpr (MAP == 1)
        hipLaunchKernelGGL((ensemble_moments_vec_kernel<ROWS, WEIGHTED>), dim3(grid), dim3(ENS_THREADS), 0, s, logits, T, E, B, C, CS, TS, L,
                           cal.vec_scale, cal.vec_bias, Q1, Q2, QH, rows.list, rows.n_e, cal.ens_w);
    else
        hipLaunchKernelGGL((ensemble_moments_kernel<ROWS, WEIGHTED>), dim3(grid), dim3(ENS_THREADS), 0, s, logits, T, E, B, C, CS, TS, L, tau, Q1, Q2,
                           QH, rows.list, rows.n_e, cal.ens_w);
}

// The one dispatch over (ROWS, WEIGHTED), for either form
template <int MAP, class... Args>
static void dispatch_ens(bool by_rows, bool weighted, const Args&... args) {
    if (by_rows && weighted) launch_ens<MAP, true, true>(args...);
    else if (by_rows) launch_ens<MAP, true, false>(args...);
    else if (weighted) launch_ens<MAP, false, true>(args...);
    else launch_ens<MAP, false, false>(args...);
}

int launch_ensemble_moments(const float* logits, int T, int E, int B, int C, const Calibration& cal, const EnsRows& rows, double* Q1, double* Q2,
                            double* QH, hipStream_t s) {
    if (T < 1 || B < 1 || (rows.list && (rows.Bc < 1 || rows.Bc > B))) return BMI_ERR_INVALID;
    if (cal.check() != BMI_OK) return BMI_ERR_INVALID;
    if (!ensemble_takes(E, C)) return BMI_ERR_UNSUPPORTED;
    const int CS = C | 1;                                // odd row stride
    const int TS = std::min(ENS_SLAB / (E * CS), ENS_ROWS / E);      // >= 1 (ensemble_takes)
    int L = 1;
    while (L < C && L < 64) L <<= 1;
    EnsTau tau;
    for (int e = 0; e < BMI_ENS_MAX_EXITS; ++e) tau.inv[e] = e < E && e < (int)cal.inv_tau.size() ? cal.inv_tau[e] : 1.f;
    const bool by_rows = rows.list || rows.n_e, weighted = cal.ens_w != nullptr;
    const unsigned grid = (unsigned)(rows.list ? rows.Bc : B);
    if (cal.mat) dispatch_ens<2>(by_rows, weighted, grid, s, logits, T, E, B, C, CS, TS, L, cal, tau, rows, Q1, Q2, QH);
    else if (cal.vec_scale) dispatch_ens<1>(by_rows, weighted, grid, s, logits, T, E, B, C, CS, TS, L, cal, tau, rows, Q1, Q2, QH);
    else dispatch_ens<0>(by_rows, weighted, grid, s, logits, T, E, B, C, CS, TS, L, cal, tau, rows, Q1, Q2, QH);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// n_e[b] = exit_of[b] + 1: the exits image b ran under bmi_forward_mcd_exit_staged, the per-image exit count of the launch above
__global__ void exit_counts_kernel(const int* __restrict__ exit_of, int n, int* __restrict__ n_e) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b < n) n_e[b] = exit_of[b] + 1;
}

int launch_exit_counts(const int* exit_of, int n, int* n_e, hipStream_t s) {
    if (!exit_of || !n_e || n < 1) return BMI_ERR_INVALID;
    hipLaunchKernelGGL(exit_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, exit_of, n, n_e);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// One wave per (exit, image) row: mean = Q1 / T, var = max(Q2 / T - mean^2, 0) (ddof 0, a NaN stays a NaN), the entropy of the mean by
// float64 wavefront shuffle like finalize_uncertainty_kernel, expected entropy QH / T, mutual information clamped at 0.
// PER_IMAGE (bmi_finalize_ensemble_per_image): row (exit, image b) divides by t_used[b].
template <bool PER_IMAGE = false>
__global__ __launch_bounds__(256) void finalize_ensemble_kernel(int rows, int C, double t, const double* __restrict__ Q1,
                                                                const double* __restrict__ Q2, const double* __restrict__ QH,
                                                                double* __restrict__ mean, double* __restrict__ var, double* __restrict__ pred,
                                                                double* __restrict__ expd, double* __restrict__ mi, int* nonfinite,
                                                                const int* __restrict__ t_used, int batch) {
#pragma clang fp contract(off)
    const int row = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                       // (wave-uniform)
    if (PER_IMAGE) t = (double)t_used[row % batch];
    double h = 0.0;
    int bad = 0;
    for (int c = lane; c < C; c += 64) {
        const size_t o = (size_t)row * C + c;
        const double s1 = Q1[o], s2 = Q2[o];
        const double m = s1 / t;
        const double v = s2 / t - m * m;
        mean[o] = m;
        var[o] = v > 0 ? v : (v == v ? 0 : v);
        if (m > 0.0) h -= m * log(m);
        const bool nf = !(__builtin_isfinite(s1) && __builtin_isfinite(s2));
        bad += nf;
        if (!__builtin_isfinite(s1)) h = s1 - s1;   // NaN: the row's entropy is not a number either
    }
    const double sh = QH[row];
    if (lane == 0) bad += !__builtin_isfinite(sh);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        h += __shfl_xor(h, m);
        bad += __shfl_xor(bad, m);
    }
    if (lane == 0) {
        const double e = sh / t, d = h - e;
        pred[row] = h;
        expd[row] = e;
        mi[row] = d > 0 ? d : (d == d ? 0.0 : d);
        if (nonfinite && bad) atomicAdd(nonfinite, bad);
    }
}

int launch_finalize_ensemble(int n_rows, int C, int t_total, const double* Q1, const double* Q2, const double* QH, double* mean, double* var,
                             double* pred, double* expd, double* mi, int* nonfinite, hipStream_t s) {
    if (n_rows <= 0 || C <= 0 || t_total <= 0) return BMI_ERR_INVALID;
    hipLaunchKernelGGL((finalize_ensemble_kernel<false>), dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, n_rows, C, (double)t_total, Q1, Q2,
                       QH, mean, var, pred, expd, mi, nonfinite, (const int*)nullptr, 1);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_finalize_ensemble_per_image(int n_exits, int batch, int C, const int* t_used, const double* Q1, const double* Q2, const double* QH,
                                       double* mean, double* var, double* pred, double* expd, double* mi, int* nonfinite, hipStream_t s) {
    if (n_exits <= 0 || batch <= 0 || C <= 0 || !t_used) return BMI_ERR_INVALID;
    const int n_rows = n_exits * batch;
    hipLaunchKernelGGL((finalize_ensemble_kernel<true>), dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, n_rows, C, 1.0, Q1, Q2, QH, mean, var,
                       pred, expd, mi, nonfinite, t_used, batch);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
