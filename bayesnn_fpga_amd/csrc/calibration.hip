// The objective of a per-exit temperature fit (bmi_nll_temperature_grid): for G candidate temperatures per exit, the negative
// log-likelihood of the T-mean tempered softmax on per-sample logits [T][E][B][C] (bmi_forward_mcd_samples' layout),
//     z_tc = (double)l_tc * (1.0 / (double)tau),  a_t = z_{t,y} - max_c z_tc - log sum_c exp(z_tc - max_c z_tc),
//     term_b = -( logsumexp_t a_t - log T ),      nll[e][g] += sum_b term_b
// all in float64 and without fused multiply-adds, so that a numpy restatement gives the same numbers to the last few ulp
// (train/calibration.py: nll_grid_numpy).  The log-sum-exp form needs no clip: a_t is finite for any finite logits.
//
//   workgroup = one exit x a run of IMG consecutive images x a slice of NLL_GS candidates, 256 threads.  The run's logits are staged
//               in LDS once ([pair = (image, sample)][C], rows padded to an odd stride: lanes walk different rows at the same class)
//               and every candidate of the slice walks the staged rows; IMG is what fits: IMG * T <= NLL_PAIRS pairs and
//               IMG * T * stride <= NLL_SLAB floats.  A sample count beyond that runs one image per workgroup in chunks of samples,
//               the running (max, sum) of the log-sum-exp over samples carried from chunk to chunk.
//   per row     max_c l and the label's logit are found once: tau > 0, so max_c z = (max_c l) * inv exactly (a correctly rounded
//               product is monotone) — a candidate costs ONE pass of C float64 exponentials over its row.
//   per image   one thread adds the image's T values of a_t in sample order (T exponentials against the T * C above).
//   the sum over images: the per-image terms go to a scratch [E][G][B]; nll_sum_kernel adds them in a fixed order (one wavefront per
//               (exit, candidate): lane j takes images j, j + 64, .. in order, then a shuffle butterfly) — no floating-point atomics,
//               the same bits on every run, the way head_join_kernel joins the sample groups of the exit heads.
#include <cmath>

#include "kernels.h"

#define NLL_THREADS 256
#define NLL_PAIRS 256            // (image, sample) rows per staged chunk, at most
#define NLL_SLAB 9216            // floats of staged logits (36 KB)
#define NLL_GS 4                 // candidates per workgroup

__global__ __launch_bounds__(NLL_THREADS) void nll_terms_kernel(const float* __restrict__ logits, int T, int E, int B, int C, int CS, int IMG,
                                                                int TC, const int* __restrict__ labels, const float* __restrict__ tau_grid,
                                                                int G, double* __restrict__ terms) {
#pragma clang fp contract(off)
    __shared__ float slab[NLL_SLAB];                     // [pair][CS]: pair = bi * tcn + tl
    __shared__ float row_max[NLL_PAIRS], row_lab[NLL_PAIRS];
    __shared__ double a_s[NLL_GS][NLL_PAIRS];            // a_t of (candidate, pair)
    __shared__ double st_m[NLL_GS], st_s[NLL_GS];        // several sample chunks (IMG == 1): the running max / sum per candidate
    const int tid = threadIdx.x;
    const int e = blockIdx.y;
    const int b0 = blockIdx.x * IMG;
    const int imgs = min(IMG, B - b0);
    const int g0 = blockIdx.z * NLL_GS;
    const int gs = min(NLL_GS, G - g0);
    const double log_t = log((double)T);
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tcn = min(TC, T - t0);
        const int np = imgs * tcn;                       // <= NLL_PAIRS, np * CS <= NLL_SLAB (the launcher's IMG / TC)
        __syncthreads();                                 // the previous chunk's readers are done
        for (int i = tid; i < np * C; i += NLL_THREADS) {
            const int p = i / C, c = i - p * C;
            const int bi = p / tcn, tl = p - bi * tcn;
            slab[p * CS + c] = logits[(((size_t)(t0 + tl) * E + e) * B + (b0 + bi)) * C + c];
        }
        __syncthreads();
        if (tid < np) {
            const float* row = slab + tid * CS;
            float mx = row[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
            const int y = labels[b0 + tid / tcn];
            row_max[tid] = mx;
            row_lab[tid] = (y >= 0 && y < C) ? row[y] : NAN;      // (the callers check their labels: never an out-of-range read)
        }
        __syncthreads();
        for (int it = tid; it < gs * np; it += NLL_THREADS) {
            const int gl = it / np, p = it - gl * np;
            const double inv = 1.0 / (double)tau_grid[(size_t)e * G + g0 + gl];
            const double zmax = (double)row_max[p] * inv;
            const float* row = slab + p * CS;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += exp((double)row[c] * inv - zmax);
            a_s[gl][p] = ((double)row_lab[p] * inv - zmax) - log(s);
        }
        __syncthreads();
        // log-sum-exp over the samples, in sample order: thread (candidate, image)
        for (int it = tid; it < gs * imgs; it += NLL_THREADS) {
            const int gl = it / imgs, bi = it - gl * imgs;
            double m = -INFINITY, s = 0.0;
            if (t0 > 0) { m = st_m[gl]; s = st_s[gl]; }            // (more than one chunk: imgs == 1, it == gl)
            const double* a = &a_s[gl][bi * tcn];
            double cm = a[0];
            for (int tl = 1; tl < tcn; ++tl) cm = fmax(cm, a[tl]);
            const double nm = fmax(m, cm);
            s = s * exp(m - nm);
            for (int tl = 0; tl < tcn; ++tl) s += exp(a[tl] - nm);
            m = nm;
            if (t0 + tcn >= T) terms[((size_t)e * G + g0 + gl) * B + b0 + bi] = -((m + log(s)) - log_t);
            else { st_m[gl] = m; st_s[gl] = s; }
        }
    }
}

// nll[e][g] += sum_b terms[e][g][b], one wavefront per (e, g), in a fixed order
__global__ __launch_bounds__(64) void nll_sum_kernel(const double* __restrict__ terms, int B, double* __restrict__ nll) {
    const int lane = threadIdx.x;
    const double* t = terms + (size_t)blockIdx.x * B;
    double s = 0.0;
    for (int b = lane; b < B; b += 64) s += t[b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) nll[blockIdx.x] += s;
}

int launch_nll_temperature_grid(const float* logits, int T, int E, int B, int C, const int* labels, const float* tau_grid, int G, double* nll,
                                double* scratch, hipStream_t s) {
    const int CS = C | 1;                                // odd row stride
    if (CS > NLL_SLAB) return BMI_ERR_UNSUPPORTED;
    const int pairs = min(NLL_PAIRS, NLL_SLAB / CS);     // rows a chunk can stage, >= 1
    const int TC = min(T, pairs);
    const int IMG = T <= pairs ? pairs / T : 1;
    const unsigned gx = (unsigned)((B + IMG - 1) / IMG), gz = (unsigned)((G + NLL_GS - 1) / NLL_GS);
    if (E > 65535 || gz > 65535 || (int64_t)E * G > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nll_terms_kernel, dim3(gx, (unsigned)E, gz), dim3(NLL_THREADS), 0, s, logits, T, E, B, C, CS, IMG, TC, labels, tau_grid, G,
                       scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(nll_sum_kernel, dim3((unsigned)(E * G)), dim3(64), 0, s, scratch, B, nll);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
