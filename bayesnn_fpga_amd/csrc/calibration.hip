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
//
// The objective of a JOINT fit of the exit ensembles (bmi_nll_ensemble_temperature_grid, ens_nll_terms_kernel below): row e is the NLL
// of the mean over exits 0..e and over the T samples of the tempered softmax — the row ensemble.hip forms, as a likelihood —
//     a[t][i][b] as a_t above at tau_i(g),  L[i][b] = logsumexp_t a[t][i][b],  R[0] = L[0],  R[e] = logaddexp(R[e-1], L[e]),
//     nll[e][g] += sum_b -( R[e][b] - log(T * (e + 1)) ),      logaddexp(x, y) = m + log(exp(x - m) + exp(y - m)),  m = max(x, y)
// where tau_i(g) is the candidate tau_cand[g] for the exits in vary_mask and the current tau[i] for the others
// (train/calibration.py: ensemble_nll_grid_numpy).
//
//   workgroup = a run of IMG consecutive images x ALL E exits x a slice of at most ENS_GS candidates, 256 threads.  The run's logits are
//               staged once, slab row = (sample, exit, image) with the same odd stride; row max and label logit once per row.
//   a           ONE list of work items per chunk: (row) for the exits outside the mask — their a does not depend on the candidate and
//               is computed once per row and workgroup — and (candidate, row) for the exits in the mask.  A candidate of a coordinate
//               step costs C exponentials per (image, sample), not E * C; G = 33 candidates of a step at E = 4 cost 6 * 3C + 33C = 51C
//               against the 132C of a per-exit grid launch on the same logits.
//   join        one thread per (candidate, image) walks the exits in order: the log-sum-exp over the samples in sample order, then
//               logaddexp onto the running R, and writes the image's term of every row e.  Rows below the lowest varied exit come
//               from the same values by the same operations for every candidate: they hold the same bits.
//   chunks      T * E rows that do not fit run one image per workgroup in chunks of TC samples; the running (max, sum) of every
//               (candidate, exit) is carried in LDS from chunk to chunk.
//   limits      the slab stays at NLL_SLAB's 36 KB and a chunk at ENS_ROWS = 192 rows, ENS_GS = 6: with row_max / row_lab (1.5 KB), a of the
//               fixed rows (1.5 KB), a of (candidate, row) (9 KB) and the chunk state (3 KB) a workgroup holds 51 KB of LDS, so THREE
//               workgroups (12 wavefronts) share a CU's 160 KB — the kernel is bound by the latency of serial float64 exponentials,
//               which resident wavefronts hide.  The paper's shape (E = 4, C = 100, T = 10: 40 rows of 101 floats per image) fits two
//               images either way; a third would need a 48 KB slab and drop the CU to two workgroups.  E = 5, C = 100 fits 18
//               (image, sample) rows: T = 10 runs one image per workgroup, unchunked.  The balanced slice (G = 33: six slices of 6, 6, 6,
//               6, 6, 3) makes 750 workgroups of the paper's batch of 250, one resident wave of the chip's 768 slots.
//   the sum over images is nll_sum_kernel's, on the same [E][G][B] scratch.
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

#define ENS_SLAB BMI_NLL_ENS_SLAB      // floats of staged logits (36 KB, NLL_SLAB's)
#define ENS_ROWS BMI_NLL_ENS_ROWS      // (sample, exit, image) rows per staged chunk, at most
#define ENS_GS 6                       // candidates per workgroup, at most
#define ENS_MAX_EXITS 32               // vary_mask is 32 bits

__global__ __launch_bounds__(NLL_THREADS) void ens_nll_terms_kernel(const float* __restrict__ logits, int T, int E, int B, int C, int CS, int IMG,
                                                                    int TC, const int* __restrict__ labels, const float* __restrict__ tau,
                                                                    unsigned vary_mask, const float* __restrict__ tau_cand, int G, int GSL,
                                                                    double* __restrict__ terms) {
#pragma clang fp contract(off)
    __shared__ float slab[ENS_SLAB];                     // [row][CS]: row = (tl * E + i) * imgs + bi
    __shared__ float row_max[ENS_ROWS], row_lab[ENS_ROWS];
    __shared__ double a_f[ENS_ROWS];                     // a of (row), exits outside the mask
    __shared__ double a_v[ENS_GS][ENS_ROWS];             // a of (candidate, row), exits in the mask
    __shared__ double st_m[ENS_GS][ENS_MAX_EXITS], st_s[ENS_GS][ENS_MAX_EXITS];      // several sample chunks (IMG == 1): the running max / sum
    __shared__ int ex_of[ENS_MAX_EXITS];                 // the exits outside the mask in order, then the exits in the mask in order
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * IMG;
    const int imgs = min(IMG, B - b0);
    const int g0 = blockIdx.y * GSL;
    const int gs = min(GSL, G - g0);
    const int nv = __popc(vary_mask), nf = E - nv;
    if (tid < E) {
        const int below = __popc(vary_mask & ((1u << tid) - 1u));            // varied exits below this one
        ex_of[(vary_mask >> tid & 1u) ? nf + below : tid - below] = tid;
    }
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tcn = min(TC, T - t0);
        const int np = imgs * tcn;                       // (image, sample) pairs; rows = np * E <= ENS_ROWS, rows * CS <= ENS_SLAB (the launcher's IMG / TC)
        const int rows = np * E;
        __syncthreads();                                 // the previous chunk's readers are done (and ex_of is written)
        for (int idx = tid; idx < rows * C; idx += NLL_THREADS) {
            const int r = idx / C, c = idx - r * C;
            const int ti = r / imgs, bi = r - ti * imgs; // ti = tl * E + i
            slab[r * CS + c] = logits[((size_t)t0 * E + ti) * B * C + (size_t)(b0 + bi) * C + c];
        }
        __syncthreads();
        if (tid < rows) {
            const float* row = slab + tid * CS;
            float mx = row[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
            const int y = labels[b0 + tid % imgs];
            row_max[tid] = mx;
            row_lab[tid] = (y >= 0 && y < C) ? row[y] : NAN;      // (the callers check their labels: never an out-of-range read)
        }
        __syncthreads();
        const int n_fixed = np * nf, n_var = np * nv;
        for (int it = tid; it < n_fixed + gs * n_var; it += NLL_THREADS) {
            int gl = -1, k = it;
            if (it >= n_fixed) { gl = (it - n_fixed) / n_var; k = n_fixed + (it - n_fixed) - gl * n_var; }
            const int i = ex_of[k / np], p = k % np;     // p = tl * imgs + bi
            const int tl = p / imgs, bi = p - tl * imgs;
            const int r = (tl * E + i) * imgs + bi;
            const double inv = 1.0 / (double)(gl < 0 ? tau[i] : tau_cand[g0 + gl]);
            const double zmax = (double)row_max[r] * inv;
            const float* row = slab + r * CS;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += exp((double)row[c] * inv - zmax);
            const double a = ((double)row_lab[r] * inv - zmax) - log(s);
            if (gl < 0) a_f[r] = a;
            else a_v[gl][r] = a;
        }
        __syncthreads();
        // thread (candidate, image): per exit the log-sum-exp over the samples in sample order, then the exits in order
        for (int it = tid; it < gs * imgs; it += NLL_THREADS) {
            const int gl = it / imgs, bi = it - gl * imgs;
            const bool last = t0 + tcn >= T;
            double R = 0.0;
            for (int i = 0; i < E; ++i) {
                const double* a = ((vary_mask >> i & 1u) ? a_v[gl] : a_f) + i * imgs + bi;       // sample tl at a[tl * E * imgs]
                const int step = E * imgs;
                double m = -INFINITY, s = 0.0;
                if (t0 > 0) { m = st_m[gl][i]; s = st_s[gl][i]; }              // (more than one chunk: imgs == 1, it == gl)
                double cm = a[0];
                for (int tl = 1; tl < tcn; ++tl) cm = fmax(cm, a[tl * step]);
                const double nm = fmax(m, cm);
                s = s * exp(m - nm);
                for (int tl = 0; tl < tcn; ++tl) s += exp(a[tl * step] - nm);
                m = nm;
                if (last) {
                    const double L = m + log(s);
                    if (i == 0) R = L;
                    else {
                        const double mx = fmax(R, L);
                        R = mx + log(exp(R - mx) + exp(L - mx));
                    }
                    terms[((size_t)i * G + g0 + gl) * B + b0 + bi] = -(R - log((double)T * (double)(i + 1)));
                } else { st_m[gl][i] = m; st_s[gl][i] = s; }
            }
        }
    }
}

int launch_nll_ensemble_temperature_grid(const float* logits, int T, int E, int B, int C, const int* labels, const float* tau, unsigned vary_mask,
                                         const float* tau_cand, int G, double* nll, double* scratch, hipStream_t s) {
    const int CS = C | 1;                                // odd row stride
    if (E > ENS_MAX_EXITS || (int64_t)E * CS > ENS_SLAB) return BMI_ERR_UNSUPPORTED;
    const int per_t = min(ENS_ROWS, ENS_SLAB / CS) / E;  // samples of one image (E rows each) a chunk can stage, >= 1
    const int TC = min(T, per_t);
    const int IMG = T <= per_t ? min(per_t / T, B) : 1;
    const int slices = (G + ENS_GS - 1) / ENS_GS, GSL = (G + slices - 1) / slices;      // balanced: G = 7 runs as 4 + 3, not 6 + 1
    const unsigned gx = (unsigned)((B + IMG - 1) / IMG), gy = (unsigned)((G + GSL - 1) / GSL);
    if (gy > 65535 || (int64_t)E * G > INT32_MAX) return BMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ens_nll_terms_kernel, dim3(gx, gy), dim3(NLL_THREADS), 0, s, logits, T, E, B, C, CS, IMG, TC, labels, tau, vary_mask, tau_cand,
                       G, GSL, scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(nll_sum_kernel, dim3((unsigned)(E * G)), dim3(64), 0, s, scratch, B, nll);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// Value and gradient of a per-exit VECTOR-SCALING fit (bmi_nll_vector_scaling_grad): with z_tc = (double)l_tc * a_c + b_c (two rounded float64
// operations; a, b float64 [E][C] — the optimiser's smooth objective, the fp32 rounding of the head happens once, when a result is applied),
//     m_t = max_c z_tc,  s_t = sum_c exp(z_tc - m_t),  A_t = (z_ty - m_t) - log s_t,  nll_b = -( logsumexp_t A_t - log T ),
//     r_t = exp(A_t - M) / S  (M = max_t A_t, S = sum_t exp(A_t - M)),   p_tc = exp(z_tc - m_t) / s_t,
//     d nll_b / d b_c = sum_t r_t (p_tc - [c == y]),      d nll_b / d a_c = sum_t r_t (p_tc - [c == y]) l_tc
// (train/calibration.py: nll_vector_numpy).  float64 throughout, no fused multiply-adds, no floating-point atomics.
//
//   workgroup = one image x one exit, 256 threads; the samples go through LDS in chunks of TC rows ([row][C | 1] floats, odd stride, and the
//               float64 exponentials beside them), in sample order.
//   pass 1      a group of L = min(64, pow2 >= C) lanes per row: max of z, the exponentials to LDS, their sum by shuffle butterfly (a fixed
//               tree), A_t.
//   join        one thread: the chunk's max of A, the running (M, S) of the log-sum-exp over samples moved onto the new max, the weights
//               w_t = exp(A_t - M) of the chunk — the state ens_nll_terms_kernel carries, so T is not bounded by what a chunk stages.
//   pass 2      thread c owns class c: its two running sums (registers, carried from chunk to chunk, rescaled by exp(M_old - M_new) with
//               S) take the chunk's samples in sample order; divided by S once, at the end.
//   terms       [E][B][2C + 1] float64: the image's nll, then C entries of d / d a, then C of d / d b; nll_vec_sum_kernel adds them over the
//               images in nll_sum_kernel's fixed order INTO the outputs, so a fit accumulates over loader batches in call order.
#define NLLV_SLAB 3456           // staged logits (floats, 13.5 KB) and exponentials (float64, 27 KB) per chunk
#define NLLV_ROWS 64             // samples per staged chunk, at most: the kernel's staging limit is min(NLLV_ROWS, NLLV_SLAB / (C | 1))
#define NLLV_MAX_C 256           // thread c owns class c

__global__ __launch_bounds__(NLL_THREADS) void nll_vec_terms_kernel(const float* __restrict__ logits, int T, int E, int B, int C, int CS, int TC,
                                                                    int L, const int* __restrict__ labels, const double* __restrict__ scale,
                                                                    const double* __restrict__ bias, double* __restrict__ terms) {
#pragma clang fp contract(off)
    __shared__ float slab[NLLV_SLAB];                    // [tl][CS] raw logits
    __shared__ double pe[NLLV_SLAB];                     // [tl][CS] exp(z - m_t)
    __shared__ double a_s[NLLV_MAX_C], b_s[NLLV_MAX_C];
    __shared__ double row_s[NLLV_ROWS], row_a[NLLV_ROWS], wt[NLLV_ROWS];
    __shared__ double st[3];                             // running M, S and the chunk's rescale factor exp(M_old - M_new)
    const int tid = threadIdx.x;
    const int b = blockIdx.x, e = blockIdx.y;
    const int lane = tid & (L - 1), grp = tid / L, ngrp = NLL_THREADS / L;
    const int y = labels[b];
    const bool y_ok = y >= 0 && y < C;                   // (the callers check their labels: never an out-of-range read)
    if (tid < C) { a_s[tid] = scale[(size_t)e * C + tid]; b_s[tid] = bias[(size_t)e * C + tid]; }
    if (tid == 0) { st[0] = -INFINITY; st[1] = 0.0; st[2] = 0.0; }
    double ga = 0.0, gb = 0.0;                           // thread c < C: the unnormalised sums of class c
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tcn = min(TC, T - t0);                 // <= NLLV_ROWS, tcn * CS <= NLLV_SLAB (the launcher's TC)
        __syncthreads();                                 // the previous chunk's readers are done (first chunk: a_s / b_s / st are written)
        for (int i = tid; i < tcn * C; i += NLL_THREADS) {
            const int tl = i / C, c = i - tl * C;
            slab[tl * CS + c] = logits[(((size_t)(t0 + tl) * E + e) * B + b) * C + c];
        }
        __syncthreads();
        for (int r0 = 0; r0 < tcn; r0 += ngrp) {         // (every lane walks every step: the shuffles below need whole groups)
            const int r = r0 + grp;
            const bool live = r < tcn;
            const float* row = slab + (live ? r : 0) * CS;
            double mx = -INFINITY;
            if (live)
                for (int c = lane; c < C; c += L) mx = fmax(mx, (double)row[c] * a_s[c] + b_s[c]);
            for (int m = L >> 1; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m));
            double s = 0.0;
            if (live)
                for (int c = lane; c < C; c += L) {
                    const double ex = exp(((double)row[c] * a_s[c] + b_s[c]) - mx);
                    pe[r * CS + c] = ex;
                    s += ex;
                }
            for (int m = L >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (live && lane == 0) {
                row_s[r] = s;
                row_a[r] = y_ok ? (((double)row[y] * a_s[y] + b_s[y]) - mx) - log(s) : (double)NAN;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double cm = row_a[0];
            for (int tl = 1; tl < tcn; ++tl) cm = fmax(cm, row_a[tl]);
            const double m = st[0], nm = fmax(m, cm);
            const double f = exp(m - nm);                // first chunk: exp(-inf) = 0 against sums that are 0
            double s = st[1] * f;
            for (int tl = 0; tl < tcn; ++tl) {
                const double w = exp(row_a[tl] - nm);
                wt[tl] = w;
                s += w;
            }
            st[0] = nm; st[1] = s; st[2] = f;
        }
        __syncthreads();
        if (tid < C) {
            const double f = st[2];
            ga = ga * f;
            gb = gb * f;
            const double hot = tid == y ? 1.0 : 0.0;
            for (int tl = 0; tl < tcn; ++tl) {
                const double d = wt[tl] * (pe[tl * CS + tid] / row_s[tl] - hot);
                gb += d;
                ga += d * (double)slab[tl * CS + tid];
            }
        }
    }
    __syncthreads();
    double* const out = terms + ((size_t)e * B + b) * (size_t)(2 * C + 1);
    const double S = st[1];
    if (tid == 0) out[0] = -((st[0] + log(S)) - log((double)T));
    if (tid < C) { out[1 + tid] = ga / S; out[1 + C + tid] = gb / S; }
}

// nll[e] / grad_scale[e][c] / grad_bias[e][c] += sum_b terms[e][b][k], one wavefront per (e, k), in nll_sum_kernel's fixed order
__global__ __launch_bounds__(64) void nll_vec_sum_kernel(const double* __restrict__ terms, int B, int C, double* __restrict__ nll,
                                                         double* __restrict__ grad_scale, double* __restrict__ grad_bias) {
    const int lane = threadIdx.x, k = blockIdx.x, e = blockIdx.y;
    const size_t row = (size_t)(2 * C + 1);
    const double* t = terms + (size_t)e * B * row + k;
    double s = 0.0;
    for (int b = lane; b < B; b += 64) s += t[(size_t)b * row];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) {
        if (k == 0) nll[e] += s;
        else if (k <= C) grad_scale[(size_t)e * C + k - 1] += s;
        else grad_bias[(size_t)e * C + k - 1 - C] += s;
    }
}

bool nll_vector_takes(int E, int B, int C) {
    return E >= 1 && B >= 1 && C >= 1 && C <= NLLV_MAX_C && E <= 65535 && 2 * C + 1 <= 65535;
}

int launch_nll_vector_scaling_grad(const float* logits, int T, int E, int B, int C, const int* labels, const double* scale, const double* bias,
                                   double* nll, double* grad_scale, double* grad_bias, double* scratch, hipStream_t s) {
    if (!nll_vector_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    const int CS = C | 1;                                // odd row stride
    const int TC = min(T, min(NLLV_ROWS, NLLV_SLAB / CS));           // >= 1: CS <= 257
    int L = 1;
    while (L < C && L < 64) L <<= 1;
    hipLaunchKernelGGL(nll_vec_terms_kernel, dim3((unsigned)B, (unsigned)E), dim3(NLL_THREADS), 0, s, logits, T, E, B, C, CS, TC, L, labels, scale,
                       bias, scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(nll_vec_sum_kernel, dim3((unsigned)(2 * C + 1), (unsigned)E), dim3(64), 0, s, scratch, B, C, nll, grad_scale, grad_bias);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// Value and gradient of a per-exit MATRIX-SCALING fit (bmi_nll_matrix_scaling_grad): nll_vec_terms_kernel with
//     z_tc = ((0.0 + (double)l_t0 * M[c][0]) + (double)l_t1 * M[c][1] + ...) + b[c]       j ascending, every operation rounded
// (M float64 [E][C][C] row-major, row = output class; b float64 [E][C]) in place of l * a + b, and the gradient of the matrix,
//     d nll_b / d M[c][j] = sum_t r_t (p_tc - [c == y]) l_tj,
// beside the bias's (train/calibration.py: nll_matrix_numpy).  float64 throughout, no fused multiply-adds, no floating-point atomics.
//
//   workgroup = one image x one exit, 256 threads; the samples go through LDS in chunks of TC rows, in sample order.
//   z           a thread per (sample, class) of the chunk walks its row of M (through L1 / L2: 80 KB per exit at C = 100 do not fit in LDS
//               beside the chunk) against the staged logits, j ascending, and leaves z in pe.
//   pass 1      a group of L lanes per row, as in the vector kernel: max of z, the exponentials over z in place, their sum by shuffle
//               butterfly, A_t (by the lane that met class y).
//   join        one thread: the running (M, S) of the log-sum-exp over samples, the chunk's weights w_t — the vector kernel's.
//   d           a thread per (sample, class): d_tc = w_t (p_tc - [c == y]) over the exponential in place.
//   sums        a thread per entry k of [C * C + C] adds the chunk's samples in sample order onto ITS OWN running sum, which lives in the
//               image's row of `terms` (read back by the thread that wrote it; rescaled by exp(M_old - M_new) from the second chunk on, divided
//               by S in the last one): 10 100 running sums at C = 100 are neither 256 threads' registers nor this workgroup's LDS.
//   terms       [E][B][1 + C * C + C] float64: the image's nll, the C * C entries of d / d M, the C of d / d b; nll_mat_sum_kernel adds
//               them over the images in nll_sum_kernel's fixed order INTO the outputs.
#define NLLM_SLAB 3456           // staged logits (floats, 13.5 KB) and z / exponentials / d (float64, 27 KB) per chunk
#define NLLM_ROWS 64             // samples per staged chunk, at most: the kernel's staging limit is min(NLLM_ROWS, NLLM_SLAB / (C | 1))
#define NLLM_MAX_C 128           // the head's own limit

__global__ __launch_bounds__(NLL_THREADS) void nll_mat_terms_kernel(const float* __restrict__ logits, int T, int E, int B, int C, int CS, int TC,
                                                                    int L, const int* __restrict__ labels, const double* __restrict__ matrix,
                                                                    const double* __restrict__ bias, double* __restrict__ terms) {
#pragma clang fp contract(off)
    __shared__ float slab[NLLM_SLAB];                    // [tl][CS] raw logits
    __shared__ double pe[NLLM_SLAB];                     // [tl][CS] z, then exp(z - m_t), then d
    __shared__ double row_s[NLLM_ROWS], row_a[NLLM_ROWS], wt[NLLM_ROWS];
    __shared__ double st[3];                             // running M, S and the chunk's rescale factor exp(M_old - M_new)
    const int tid = threadIdx.x;
    const int b = blockIdx.x, e = blockIdx.y;
    const int lane = tid & (L - 1), grp = tid / L, ngrp = NLL_THREADS / L;
    const int y = labels[b];
    const bool y_ok = y >= 0 && y < C;                   // (the callers check their labels: never an out-of-range read)
    const double* const mat = matrix + (size_t)e * C * C;
    const double* const bi = bias + (size_t)e * C;
    const int NK = C * C + C;
    double* const out = terms + ((size_t)e * B + b) * (size_t)(NK + 1);
    if (tid == 0) { st[0] = -INFINITY; st[1] = 0.0; st[2] = 0.0; }
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tcn = min(TC, T - t0);                 // <= NLLM_ROWS, tcn * CS <= NLLM_SLAB (the launcher's TC)
        __syncthreads();                                 // the previous chunk's readers are done (first chunk: st is written)
        for (int i = tid; i < tcn * C; i += NLL_THREADS) {
            const int tl = i / C, c = i - tl * C;
            slab[tl * CS + c] = logits[(((size_t)(t0 + tl) * E + e) * B + b) * C + c];
        }
        __syncthreads();
        for (int i = tid; i < tcn * C; i += NLL_THREADS) {
            const int tl = i / C, c = i - tl * C;
            const float* row = slab + tl * CS;
            const double* mrow = mat + (size_t)c * C;
            double z = 0.0;
            for (int j = 0; j < C; ++j) {
                const double prod = (double)row[j] * mrow[j];
                z = z + prod;
            }
            pe[tl * CS + c] = z + bi[c];
        }
        __syncthreads();
        for (int r0 = 0; r0 < tcn; r0 += ngrp) {         // (every lane walks every step: the shuffles below need whole groups)
            const int r = r0 + grp;
            const bool live = r < tcn;
            double* zrow = pe + (live ? r : 0) * CS;
            double mx = -INFINITY;
            if (live)
                for (int c = lane; c < C; c += L) mx = fmax(mx, zrow[c]);
            for (int m = L >> 1; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m));
            double s = 0.0, zy = 0.0;
            bool mine = false;                           // this lane met class y
            if (live)
                for (int c = lane; c < C; c += L) {
                    const double z = zrow[c];
                    if (c == y) { zy = z; mine = true; }
                    const double ex = exp(z - mx);
                    zrow[c] = ex;
                    s += ex;
                }
            for (int m = L >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (live && lane == 0) {
                row_s[r] = s;
                if (!y_ok) row_a[r] = (double)NAN;
            }
            if (live && mine) row_a[r] = (zy - mx) - log(s);
        }
        __syncthreads();
        if (tid == 0) {
            double cm = row_a[0];
            for (int tl = 1; tl < tcn; ++tl) cm = fmax(cm, row_a[tl]);
            const double m = st[0], nm = fmax(m, cm);
            const double f = exp(m - nm);                // first chunk: exp(-inf) = 0 against sums that are 0
            double s = st[1] * f;
            for (int tl = 0; tl < tcn; ++tl) {
                const double w = exp(row_a[tl] - nm);
                wt[tl] = w;
                s += w;
            }
            st[0] = nm; st[1] = s; st[2] = f;
        }
        __syncthreads();
        for (int i = tid; i < tcn * C; i += NLL_THREADS) {
            const int tl = i / C, c = i - tl * C;
            const double hot = c == y ? 1.0 : 0.0;
            pe[tl * CS + c] = wt[tl] * (pe[tl * CS + c] / row_s[tl] - hot);
        }
        __syncthreads();
        const bool first = t0 == 0, last = t0 + TC >= T;
        const double f = st[2], S = st[1];
        for (int k = tid; k < NK; k += NLL_THREADS) {
            double g = first ? 0.0 : out[1 + k] * f;     // (this thread's own store of the previous chunk)
            if (k < C * C) {
                const int c = k / C, j = k - c * C;
                for (int tl = 0; tl < tcn; ++tl) {
                    const double term = pe[tl * CS + c] * (double)slab[tl * CS + j];
                    g = g + term;
                }
            } else {
                const int c = k - C * C;
                for (int tl = 0; tl < tcn; ++tl) g += pe[tl * CS + c];
            }
            out[1 + k] = last ? g / S : g;
        }
    }
    __syncthreads();
    if (tid == 0) out[0] = -((st[0] + log(st[1])) - log((double)T));
}

// nll[e] / grad_matrix[e][c][j] / grad_bias[e][c] += sum_b terms[e][b][k], one wavefront per (e, k), in nll_sum_kernel's fixed order
__global__ __launch_bounds__(64) void nll_mat_sum_kernel(const double* __restrict__ terms, int B, int C, double* __restrict__ nll,
                                                         double* __restrict__ grad_matrix, double* __restrict__ grad_bias) {
    const int lane = threadIdx.x, k = blockIdx.x, e = blockIdx.y;
    const int CC = C * C;
    const size_t row = (size_t)(CC + C + 1);
    const double* t = terms + (size_t)e * B * row + k;
    double s = 0.0;
    for (int b = lane; b < B; b += 64) s += t[(size_t)b * row];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) {
        if (k == 0) nll[e] += s;
        else if (k <= CC) grad_matrix[(size_t)e * CC + k - 1] += s;
        else grad_bias[(size_t)e * C + k - 1 - CC] += s;
    }
}

bool nll_matrix_takes(int E, int B, int C) {
    return E >= 1 && B >= 1 && C >= 1 && C <= NLLM_MAX_C && E <= 65535;
}

int launch_nll_matrix_scaling_grad(const float* logits, int T, int E, int B, int C, const int* labels, const double* matrix, const double* bias,
                                   double* nll, double* grad_matrix, double* grad_bias, double* scratch, hipStream_t s) {
    if (!nll_matrix_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    const int CS = C | 1;                                // odd row stride
    const int TC = min(T, min(NLLM_ROWS, NLLM_SLAB / CS));           // >= 1: CS <= 129
    int L = 1;
    while (L < C && L < 64) L <<= 1;
    hipLaunchKernelGGL(nll_mat_terms_kernel, dim3((unsigned)B, (unsigned)E), dim3(NLL_THREADS), 0, s, logits, T, E, B, C, CS, TC, L, labels, matrix,
                       bias, scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(nll_mat_sum_kernel, dim3((unsigned)(C * C + C + 1), (unsigned)E), dim3(64), 0, s, scratch, B, C, nll, grad_matrix, grad_bias);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
