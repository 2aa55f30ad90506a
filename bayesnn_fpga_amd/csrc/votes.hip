// Vote counts (bmi_vote_counts, bmi_forward_mcd_votes, bmi_finalize_votes): how many of the stochastic passes vote for each class, per exit
// and per exit ensemble — the input of the variation ratio (1 - the modal class's share of the votes) and of the majority-vote prediction,
// the third MC-dropout uncertainty measure beside the predictive entropy and the mutual information.  A vote is the arg-max of ONE pass, so
// it has to be taken where the per-sample logits exist: [t][E][B][C] (bmi_forward_mcd_samples' layout; the chunk bmi_forward_mcd_ensemble
// leaves in its scratch).  For pass t, image b and exit e, no fused multiply-add wherever a number is formed:
//     z_te   = the calibrated fp32 logits (Calibration, kernels.h): l | fl32(l * inv_e) | fl32(fl32(l * a_c) + b_c) | the matrix map's
//              fl32((..(fl32(M[c][0] l_0) + fl32(M[c][1] l_1)) + ..) + b_c), j ascending — the head's and ensemble.hip's own numbers
//     bad    = some z_tec, c < C, is not finite: the row casts no vote, neither does an ensemble row e' >= e of that (t, b); *nonfinite += 1
//     V[0][e][b][k] += 1,  k = min{c : z_c == max_c z}                                  fp32 comparisons, the lowest index on ties
//     p_te   = softmax_c((double) z_te), max-subtracted (ensemble.hip's phase A: the same butterfly, the same bits)
//     q_te   = (p_t0 + ... + p_te) / (e + 1)   |   ((W[e][0] p_t0 + W[e][1] p_t1) + ...) + W[e][e] p_te from 0.0, every product rounded
//     V[1][e][b][k] += 1,  k = min{c : q_c == max_c q}
// V is int32 [2][E][B][C], ADDED to with integer atomics: exact, order-free, the same counts however the passes are split into chunks,
// launches, calls or ranks.  No floating-point atomics.
//
//   vote_counts_kernel     one wave per (t, b) walks the exits; lane i owns classes i and i + 64 (C <= 128).  The row max and the sum of the
//                          exponentials by __shfl_xor butterfly, the arg-max by butterfly max + ballot + find-first-set, classes < 64 before
//                          classes >= 64: the lowest index without comparing indices.  The lane that owns the winner adds 1.  The matrix map
//                          reads the raw row through wave-uniform loads (a j loop every lane walks); the weighted ensemble parks p_ti of the
//                          exits so far in LDS, every lane in words of its own (no barrier: nobody reads another lane's).  Templated on the
//                          map and on WEIGHTED: the plain instantiation carries none of the others' registers.
//   finalize_votes_kernel  one wave per (kind, exit, image) row of V: n = the votes cast, m = the modal count, vote_class = the lowest class
//                          that has it, variation_ratio = 1 - m / n, vote_entropy = -sum f log f in class order (f = V_c / n); n = 0:
//                          -1, 1.0, 0.0.  Outputs overwritten.
#include <climits>
#include <cmath>
#include <cstdint>

#include "kernels.h"
#include "vote_walk.h"      // the exit walk of one (pass, image), shared with votes_rows.hip

template <int MAP, bool WEIGHTED>
__global__ __launch_bounds__(VOTE_THREADS) void vote_counts_kernel(const float* __restrict__ logits, int T, int E, int B, int C, VoteTau tau,
                                                                   const float* __restrict__ ma, const float* __restrict__ mb,
                                                                   const double* __restrict__ W, int* __restrict__ V, int* nonfinite) {
#pragma clang fp contract(off)
    extern __shared__ double vote_p[];                    // WEIGHTED: [wave][exit][2][64] — p of this lane's two classes
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + wv;       // (t, b), wave-uniform
    if (w >= (long long)T * B) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(w / B), b = (int)(w - (long long)t * B);
    vote_walk<MAP, WEIGHTED>(logits, t, b, lane, E, E, B, C, tau, ma, mb, W, V, nonfinite, vote_p + (size_t)wv * E * 128 + lane);
}

__global__ __launch_bounds__(VOTE_THREADS) void finalize_votes_kernel(int rows, int C, const int* __restrict__ V, int* __restrict__ vote_class,
                                                                      double* __restrict__ ratio, double* __restrict__ entropy) {
#pragma clang fp contract(off)
    const int r = (int)(((long long)blockIdx.x * VOTE_THREADS + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;                                // (wave-uniform)
    const int* v = V + (size_t)r * C;
    long long n = 0;
    int m = 0;
    for (int c = lane; c < C; c += 64) {
        const int x = v[c];
        n += x;
        m = max(m, x);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        n += __shfl_xor(n, k);
        m = max(m, __shfl_xor(m, k));
    }
    if (n <= 0) {                                         // no vote cast (every pass bad, or nothing accumulated yet)
        if (lane == 0) { vote_class[r] = -1; ratio[r] = 1.0; entropy[r] = 0.0; }
        return;
    }
    int kc = INT_MAX;                                     // the lowest class with the modal count
    double h = 0.0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const int x = c < C ? v[c] : 0;
        if (c < C && x == m) kc = min(kc, c);
        const double f = (double)x / (double)n;
        const double term = x > 0 ? f * log(f) : 0.0;
        const int cn = min(64, C - c0);
        for (int j = 0; j < cn; ++j) h = h - __shfl(term, j);       // class order, every lane the same sum
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) kc = min(kc, __shfl_xor(kc, k));
    if (lane == 0) {
        vote_class[r] = kc;
        ratio[r] = 1.0 - (double)m / (double)n;
        entropy[r] = h;
    }
}

bool vote_counts_takes(int T, int E, int B, int C) {
    return T >= 1 && E >= 1 && B >= 1 && C >= 1 && C <= BMI_ENS_MAX_CLASSES && E <= BMI_ENS_MAX_EXITS &&
           (int64_t)T * B <= INT32_MAX / 64;             // (the launch grid: 64 threads per (t, b))
}

template <int MAP, bool WEIGHTED>
static void launch_votes(unsigned grid, unsigned threads, size_t lds, hipStream_t s, const float* logits, int T, int E, int B, int C,
                         const VoteTau& tau, const float* ma, const float* mb, const double* W, int* V, int* nonfinite) {
    hipLaunchKernelGGL((vote_counts_kernel<MAP, WEIGHTED>), dim3(grid), dim3(threads), lds, s, logits, T, E, B, C, tau, ma, mb, W, V, nonfinite);
}

int launch_vote_counts(const float* logits, int T, int E, int B, int C, const Calibration& cal, int* V, int* nonfinite, hipStream_t s) {
    if (cal.check() != BMI_OK) return BMI_ERR_INVALID;
    if (!vote_counts_takes(T, E, B, C)) return BMI_ERR_UNSUPPORTED;
    const VoteLaunch l = vote_launch_plan(cal, E, (int64_t)T * B);
    const VoteTau& tau = l.tau;
    const bool weighted = l.weighted;
    const unsigned grid = l.grid, threads = l.threads;
    const size_t lds = l.lds;
    const float *ma = l.ma, *mb = l.mb;
#define VOTE_CASE(M)                                                                                                              \
    case M:                                                                                                                       \
        if (weighted) launch_votes<M, true>(grid, threads, lds, s, logits, T, E, B, C, tau, ma, mb, cal.ens_w, V, nonfinite);    \
        else launch_votes<M, false>(grid, threads, lds, s, logits, T, E, B, C, tau, ma, mb, cal.ens_w, V, nonfinite);            \
        break;
    switch (l.map) {
        VOTE_CASE(VOTE_MAP_NONE)
        VOTE_CASE(VOTE_MAP_TEMP)
        VOTE_CASE(VOTE_MAP_VEC)
        VOTE_CASE(VOTE_MAP_MAT)
    }
#undef VOTE_CASE
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_finalize_votes(int n_rows, int C, const int* V, int* vote_class, double* ratio, double* entropy, hipStream_t s) {
    if (n_rows <= 0 || C <= 0) return BMI_ERR_INVALID;
    hipLaunchKernelGGL(finalize_votes_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(VOTE_THREADS), 0, s, n_rows, C, V, vote_class, ratio,
                       entropy);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
