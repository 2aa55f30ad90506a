// Classwise reliability tables (bmi_classwise_record / bmi_classwise_table): per exit, per exit ensemble AND PER CLASS the confidence histogram
// behind the classwise ECE (Kull et al. 2019; Nixon et al. 2019's static calibration error) — what vector and matrix scaling are fitted to
// correct and the top-label tables of reliability.hip cannot show —, from the T-mean probabilities, without a host copy of them.  THE
// ARITHMETIC CONTRACT (restated in numpy, loop by loop, as train.reliability.classwise_numpy):
//
// Input    mean float64 [E][B][C], the T-mean probabilities (bmi_finalize's `mean`); labels int32 [B] — as bmi_reliability_record takes them.
// Rows     R = 2 E rows r = kind * E + e:  kind 0 is p_e = mean[e];  kind 1 is the exit ensemble q_e = (p_0 + ... + p_e) / (e + 1), added in
//          exit order from exit 0 onto 0.0, then divided once (reliability.hip's own definition).
// Per row and image, v = the row's C values; float64 and no fused multiply-add wherever a number is formed:
//     pc_c   = max(v_c, 1e-256)
//     s      = ((0.0 + pc_0) + pc_1) + ...            ascending class order: the same s the top-label record forms
//     q_c    = pc_c / s                               for EVERY class c
//     conf_c = 0.0f if q_c < 2^-126, else (float) q_c the flush is an explicit compare on the double: no denormal mode of device or host
//                                                     has a say.  s >= pc_c in floating point, so conf_c <= 1.0f
//     key_c  = the float32 bit pattern of conf_c (uint32; for non-negative floats the unsigned order of the keys is the float order)
//          At the arg-max class the key is bit for bit the key bmi_reliability_record writes for that (row, image): the same quotient, and
//          the flush never applies there (conf >= 1 / C).
// Invalid  an image whose label is outside [0, C): all R C keys of it are INVALID (0xFFFFFFFF, ranking.hip's convention), its label record is
//          -1, counters[1] += 1, nothing of it is read.  Otherwise a (row, image) with a non-finite v_c: that row's C keys are INVALID and
//          counters[0] += 1 (an exit with a non-finite value makes every ensemble from it on non-finite).  Key 0 is a VALID key here
//          (confidence zero), unlike in the top-label records.
// Records  pkeys uint32 [R][C][N_cap], the image index fastest: the table kernels stream a (row, class) line; labels_rec int32 [N_cap];
//          counters int32 [2], ADDED to, or null.  4 R C bytes per image: 32 MB at E = 4, C = 100, N = 10 000.
// Edges    float32 [R][C][n_bins + 1].  By mass, per (row, class): per = N / n_bins (integer), edges[0] = 0, edges[i + 1] = the order
//          statistic of rank min((i + 1) * per, N - 1) (0-based, ascending) of the line's N keys in unsigned order — INVALID keys sort last,
//          a selected INVALID key gives the edge 1.0f —, edges[n_bins] = 1.  Fixed: the caller's, copied to every (row, class).
// Bins     a valid pair (image n, class c) with conf >= edges[0] is in the one bin j that is the lowest with conf <= edges[j + 1]; a pair
//          below edges[0] or above edges[n_bins] is in none.  BIN 0 IS CLOSED AT ITS LOWER EDGE — unlike the top-label table, whose bins are
//          (lo, hi] and which drops key 0 —: most of the C - 1 other classes' confidences are zero or nearly so, they are data here, and the
//          published classwise ECE counts them.  A caller's edges[0] > 0 is the thresholded variant that ignores negligible probabilities.
// Table    per (row, class, bin) int64 [R][C][n_bins]: count; hits = the pairs with labels_rec[n] == c; conf_fix = sum (int64) ((double) conf
//          * 2^40), TRUNCATING.  Not an exact sum of the confidences as in the top-label table (a classwise confidence can lie below 2^-8,
//          where a float32 need not be a multiple of 2^-40): an exact, order-free INTEGER definition within count * 2^-40 of the true sum.
//          valid int64 [R]: the images of the row whose keys are not INVALID.  N < 2^22 keeps every sum below 2^62.
// Integer atomics only (LDS); no floating-point output but the edges; every output is OVERWRITTEN; the same bits on every run, however the
// N images were cut into record calls.
//
// The shared pieces are record_common.h's: walk_exit_rows and class_sums (the very functions reliability_records_kernel runs: the same s,
// the same key at the arg-max), radix_select_u32 (reliability.hip's line_edges_kernel, over the R C lines), bin_of / conf_fix40.
//
//   classwise_records_kernel  one wave per image walks its rows (walk_exit_rows).  Each lane writes the keys of its own classes for the
//                             2 E rows at column n0 + b; lane 0 writes the label record.
//   classwise_bins_kernel     one workgroup per line: the three integer bin sums in LDS (a thread adds a run of pairs of one bin at once),
//                             written straight to the outputs — no scratch —; the workgroups of class 0 count the row's valid images.
#include <cmath>
#include <cstdint>

#include "record_common.h"

#define CW_THREADS RECORD_THREADS
#define CW_INVALID 0xFFFFFFFFu

__global__ __launch_bounds__(CW_THREADS) void classwise_records_kernel(const double* __restrict__ mean, int E, int B, int C,
                                                                       const int* __restrict__ labels, size_t n0, size_t N_cap,
                                                                       uint32_t* __restrict__ pkeys, int* __restrict__ labels_rec, int* counters) {
#pragma clang fp contract(off)
    const long long w = ((long long)blockIdx.x * CW_THREADS + threadIdx.x) >> 6;       // the image, wave-uniform
    if (w >= B) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)w;
    const int y = labels[b];
    const size_t col = n0 + (size_t)b;
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < C, in1 = c1 < C;
    const size_t plane = (size_t)C * N_cap;                                            // the keys of one row
    uint32_t* k0 = pkeys + (size_t)c0 * N_cap + col;                                   // (dereferenced under in0 / in1 only)
    uint32_t* k1 = pkeys + (size_t)c1 * N_cap + col;
    if ((unsigned)y >= (unsigned)C) {       // (wave-uniform)
        for (int r = 0; r < 2 * E; ++r) {
            if (in0) k0[r * plane] = CW_INVALID;
            if (in1) k1[r * plane] = CW_INVALID;
        }
        if (lane == 0) {
            labels_rec[col] = -1;
            if (counters) atomicAdd(counters + 1, 1);
        }
        return;
    }
    int bad_rows = 0;
    walk_exit_rows(mean, E, B, C, b, lane, [&](int r, bool bad, double, double, double pc0, double pc1) {
        uint32_t key0 = CW_INVALID, key1 = CW_INVALID;
        if (bad) {                          // (wave-uniform)
            ++bad_rows;
        } else {                            // (the pc of a class beyond C is never read)
            const double lo[1] = {pc0}, hi[1] = {pc1};
            double s[1];
            class_sums<1>(lo, hi, C, s);
            const double q0 = pc0 / s[0], q1 = pc1 / s[0];
            key0 = q0 < 0x1p-126 ? 0u : __float_as_uint((float)q0);
            key1 = q1 < 0x1p-126 ? 0u : __float_as_uint((float)q1);
        }
        if (in0) k0[r * plane] = key0;
        if (in1) k1[r * plane] = key1;
    });
    if (lane == 0) {
        labels_rec[col] = y;
        if (counters && bad_rows) atomicAdd(counters, bad_rows);
    }
}

// grid (L): workgroup l = r * C + c writes count / hits / conf_fix [l][n_bins]; the workgroups of class 0 write valid[r]
__global__ __launch_bounds__(CW_THREADS) void classwise_bins_kernel(const uint32_t* __restrict__ pkeys, const int* __restrict__ labels_rec, int C,
                                                                    int N, size_t N_cap, int n_bins, const float* __restrict__ edges,
                                                                    long long* __restrict__ count, long long* __restrict__ hits,
                                                                    long long* __restrict__ conf_fix, long long* __restrict__ valid) {
    __shared__ float ed[BMI_REL_MAX_BINS + 1];
    __shared__ unsigned long long acc[3][BMI_REL_MAX_BINS];
    __shared__ int n_valid;
    const size_t l = blockIdx.x;
    const int c = (int)(l % (size_t)C), tid = threadIdx.x;
    if (tid <= n_bins) ed[tid] = edges[l * (n_bins + 1) + tid];
    if (tid < n_bins) acc[0][tid] = acc[1][tid] = acc[2][tid] = 0ull;
    if (tid == 0) n_valid = 0;
    __syncthreads();
    const uint32_t* k = pkeys + l * N_cap;
    int cur = -1, seen = 0;                 // the thread's run of pairs of one bin, added at once
    unsigned long long a = 0ull, h = 0ull, f = 0ull;
    for (int n = tid; n < N; n += CW_THREADS) {
        const uint32_t key = k[n];
        if (key == CW_INVALID) continue;
        ++seen;
        const float conf = __uint_as_float(key);
        const int j = bin_of(conf, ed, n_bins, true);
        if (j == n_bins) continue;
        if (j != cur) {
            if (a) {
                atomicAdd(&acc[0][cur], a);
                atomicAdd(&acc[1][cur], h);
                atomicAdd(&acc[2][cur], f);
            }
            cur = j;
            a = h = f = 0ull;
        }
        ++a;
        h += labels_rec[n] == c ? 1ull : 0ull;
        f += conf_fix40(conf);
    }
    if (a) {
        atomicAdd(&acc[0][cur], a);
        atomicAdd(&acc[1][cur], h);
        atomicAdd(&acc[2][cur], f);
    }
    if (c == 0 && seen) atomicAdd(&n_valid, seen);
    __syncthreads();
    if (tid < n_bins) {
        count[l * n_bins + tid] = (long long)acc[0][tid];
        hits[l * n_bins + tid] = (long long)acc[1][tid];
        conf_fix[l * n_bins + tid] = (long long)acc[2][tid];
    }
    if (c == 0 && tid == 0) valid[l / (size_t)C] = (long long)n_valid;
}

bool classwise_table_takes(int R, int C, int N, int n_bins) {
    return R >= 1 && C >= 1 && N >= 1 && n_bins >= 1 && n_bins <= BMI_REL_MAX_BINS && R <= 2 * BMI_ENS_MAX_EXITS && C <= BMI_ENS_MAX_CLASSES &&
           N < BMI_REL_MAX_IMAGES;
}

int launch_classwise_record(const double* mean, int E, int B, int C, const int* labels, int n0, int N_cap, uint32_t* pkeys, int* labels_rec,
                            int* counters, hipStream_t s) {
    if (!reliability_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)(((int64_t)B * 64 + CW_THREADS - 1) / CW_THREADS);
    hipLaunchKernelGGL(classwise_records_kernel, dim3(grid), dim3(CW_THREADS), 0, s, mean, E, B, C, labels, (size_t)n0, (size_t)N_cap, pkeys,
                       labels_rec, counters);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_classwise_table(const uint32_t* pkeys, const int* labels_rec, int R, int C, int N, int N_cap, int n_bins, const float* edges_in,
                           float* edges_out, long long* count, long long* hits, long long* conf_fix, long long* valid, hipStream_t s) {
    if (!classwise_table_takes(R, C, N, n_bins)) return BMI_ERR_UNSUPPORTED;
    const unsigned L = (unsigned)(R * C);   // at most 64 * 128 lines
    const int rc = launch_line_edges(pkeys, (int)L, N, N_cap, n_bins, edges_in, edges_out, s);
    if (rc != BMI_OK) return rc;
    hipLaunchKernelGGL(classwise_bins_kernel, dim3(L), dim3(CW_THREADS), 0, s, pkeys, labels_rec, C, N, (size_t)N_cap, n_bins,
                       (const float*)edges_out, count, hits, conf_fix, valid);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
