// Per-pass multi-exit accuracy (bmi_pass_accuracy): every top-k hit count of every exit and of every exit ensemble of every stochastic pass,
// and every exit's summed max-probability, from per-sample logits [t][E][B][C] (bmi_forward_mcd_samples' layout) and the labels — the
// read-out of the reference's `_MultiExitAccuracy._metrics` (SA/train/loss/base_classes.py:39-66) without its row-0 overwrite.  For pass t
// and image b, y = labels[b], float64 and no fused multiply-add wherever a number is formed:
//     rank(score) = #{c : score_c > score_y} + #{c < y : score_c == score_y}       the label loses ties to lower class indices ("lowest
//                                                                                   index on ties" = a stable descending sort)
//     rank_clf[e] = rank(l_te)                          comparisons of the fp32 logits as given
//     p_te        = softmax_c((double) l_te)            max-subtracted, as ensemble.hip's phase A
//     s_te        = p_t0 + ... + p_te                   in exit order from exit 0: the reference's unnormalised `ensemble += softmax(logits)`
//     rank_ens[e] = rank(s_te)
//     m_te        = 1 / sum_c exp(z_c - max)            the row's max-probability: the max element's exponential is exactly 1
// A row (t, e, b) with a non-finite logit is a miss in clf[e] and in ens[e' >= e] of that (t, b), adds 0.0 to the max-probability sum and 1
// to *nonfinite; a label outside [0, C) makes the image a miss everywhere (nothing is read outside the row, the row is not counted as
// non-finite).  No NaN reaches an output.
//
//   pass_accuracy_rows_kernel    one wave per (t, b) walks the exits; lane i owns classes i and i + 64 (C <= 128).  The row max and the sum of
//                                the exponentials by __shfl_xor butterfly (a fixed tree, the same wherever the row sits in a launch), the two
//                                rank counts by ballot + popcount (integers: no order), l_y loaded directly, s_y broadcast from its owner
//                                lane.  The wave writes 2 E ranks (INT32_MAX: a miss for every k) and E max-probabilities to the scratch.
//   pass_accuracy_reduce_kernel  one wave per (t, e): hits[t][kind][e][i] = #{b : rank < tops[i]} by ballot + popcount over runs of 64
//                                images, maxprob[t][e] = the m_te added in image order b = 0, 1, ... from 0.0 (every lane adds the same
//                                broadcast values): the same bits on every run, whatever the launch geometry.
// No floating-point atomics; the outputs are overwritten, not added to.
#include <climits>
#include <cmath>
#include <cstdint>

#include "kernels.h"

#define PA_THREADS 256
#define PA_MISS INT_MAX

struct PaTops { int v[BMI_PASS_ACC_MAX_TOPS]; };

// scratch: mprob float64 [T][E][B] in front (8-byte aligned at the base), then ranks int32 [T][2][E][B]
__global__ __launch_bounds__(PA_THREADS) void pass_accuracy_rows_kernel(const float* __restrict__ logits, int T, int E, int B, int C,
                                                                        const int* __restrict__ labels, double* __restrict__ mprob,
                                                                        int* __restrict__ ranks, int* nonfinite) {
#pragma clang fp contract(off)
    const long long w = ((long long)blockIdx.x * PA_THREADS + threadIdx.x) >> 6;       // (t, b), wave-uniform
    if (w >= (long long)T * B) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(w / B), b = (int)(w - (long long)t * B);
    const int y = labels[b];
    const bool labelled = (unsigned)y < (unsigned)C;
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < C, in1 = c1 < C;
    // (c < y, per owned class: what a tie with the label's score counts as)
    const bool lo0 = c0 < y, lo1 = c1 < y;
    double s0 = 0.0, s1 = 0.0;          // the running exit sum of the two owned classes
    bool ens_ok = true;                 // no non-finite row among the exits so far
    int bad_rows = 0;
    for (int e = 0; e < E; ++e) {
        const size_t rw = ((size_t)t * E + e) * B + b;
        const float* row = logits + rw * C;
        const float l0 = in0 ? row[c0] : -INFINITY, l1 = in1 ? row[c1] : -INFINITY;
        const bool bad = __ballot((in0 && !__builtin_isfinite(l0)) || (in1 && !__builtin_isfinite(l1))) != 0ull;
        int r_clf = PA_MISS, r_ens = PA_MISS;
        double m = 0.0;
        if (bad) {                      // (wave-uniform)
            ++bad_rows;
            ens_ok = false;
        } else {
            float mx = fmaxf(l0, l1);
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) mx = fmaxf(mx, __shfl_xor(mx, k));
            const double e0 = in0 ? exp((double)l0 - (double)mx) : 0.0, e1 = in1 ? exp((double)l1 - (double)mx) : 0.0;
            double s = e0 + e1;
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k);
            m = 1.0 / s;
            s0 += e0 / s;
            s1 += e1 / s;
            if (labelled) {
                const float ly = row[y];
                r_clf = __popcll(__ballot(in0 && (l0 > ly || (l0 == ly && lo0)))) + __popcll(__ballot(in1 && (l1 > ly || (l1 == ly && lo1))));
                if (ens_ok) {
                    const double sy = __shfl(y < 64 ? s0 : s1, y & 63);
                    r_ens = __popcll(__ballot(in0 && (s0 > sy || (s0 == sy && lo0)))) + __popcll(__ballot(in1 && (s1 > sy || (s1 == sy && lo1))));
                }
            }
        }
        if (lane == 0) {
            mprob[rw] = m;
            ranks[(((size_t)t * 2 + 0) * E + e) * B + b] = r_clf;
            ranks[(((size_t)t * 2 + 1) * E + e) * B + b] = r_ens;
        }
    }
    if (lane == 0 && nonfinite && bad_rows) atomicAdd(nonfinite, bad_rows);
}

__global__ __launch_bounds__(64) void pass_accuracy_reduce_kernel(const double* __restrict__ mprob, const int* __restrict__ ranks, int E, int B,
                                                                  PaTops tops, int K, int* __restrict__ hits, double* __restrict__ maxprob) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int t = (int)(blockIdx.x / (unsigned)E), e = (int)(blockIdx.x - (unsigned)t * (unsigned)E);
    const double* mp = mprob + ((size_t)t * E + e) * B;
    const int* rc = ranks + (((size_t)t * 2 + 0) * E + e) * B;
    const int* re = ranks + (((size_t)t * 2 + 1) * E + e) * B;
    int n_clf[BMI_PASS_ACC_MAX_TOPS] = {}, n_ens[BMI_PASS_ACC_MAX_TOPS] = {};
    double s = 0.0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int n = min(64, B - b0);
        const bool live = lane < n;
        const int r0 = live ? rc[b0 + lane] : PA_MISS, r1 = live ? re[b0 + lane] : PA_MISS;
        const double m = live ? mp[b0 + lane] : 0.0;
#pragma unroll
        for (int i = 0; i < BMI_PASS_ACC_MAX_TOPS; ++i) {
            n_clf[i] += __popcll(__ballot(r0 < tops.v[i]));
            n_ens[i] += __popcll(__ballot(r1 < tops.v[i]));
        }
        for (int j = 0; j < n; ++j) s += __shfl(m, j);       // image order
    }
    if (lane < K) {
        int a = 0, c = 0;
#pragma unroll
        for (int i = 0; i < BMI_PASS_ACC_MAX_TOPS; ++i)
            if (i == lane) { a = n_clf[i]; c = n_ens[i]; }
        hits[(((size_t)t * 2 + 0) * E + e) * K + lane] = a;
        hits[(((size_t)t * 2 + 1) * E + e) * K + lane] = c;
    }
    if (lane == 0) maxprob[(size_t)t * E + e] = s;
}

bool pass_accuracy_takes(int T, int E, int B, int C, int K) {
    return T >= 1 && E >= 1 && B >= 1 && C >= 1 && K >= 1 && C <= BMI_ENS_MAX_CLASSES && E <= BMI_ENS_MAX_EXITS && K <= BMI_PASS_ACC_MAX_TOPS &&
           (int64_t)T * B <= INT32_MAX / 64 && (int64_t)T * E <= INT32_MAX;       // (the launch grids: 64 threads per (t, b), a block per (t, e))
}

int launch_pass_accuracy(const float* logits, int T, int E, int B, int C, const int* labels, const int* tops, int K, int* hits, double* maxprob,
                         int* nonfinite, void* scratch, hipStream_t s) {
    if (!pass_accuracy_takes(T, E, B, C, K)) return BMI_ERR_UNSUPPORTED;
    PaTops tp;
    for (int i = 0; i < BMI_PASS_ACC_MAX_TOPS; ++i) tp.v[i] = i < K ? tops[i] : 0;       // (0: never a hit)
    double* mprob = (double*)scratch;
    int* ranks = (int*)(mprob + (size_t)T * E * B);
    const unsigned grid = (unsigned)(((int64_t)T * B * 64 + PA_THREADS - 1) / PA_THREADS);
    hipLaunchKernelGGL(pass_accuracy_rows_kernel, dim3(grid), dim3(PA_THREADS), 0, s, logits, T, E, B, C, labels, mprob, ranks, nonfinite);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(pass_accuracy_reduce_kernel, dim3((unsigned)(T * E)), dim3(64), 0, s, (const double*)mprob, (const int*)ranks, E, B, tp, K,
                       hits, maxprob);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
