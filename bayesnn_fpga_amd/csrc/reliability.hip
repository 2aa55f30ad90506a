// Reliability tables (bmi_reliability_record / bmi_reliability_table): per exit and per exit ensemble the equal-mass (or fixed-edge) confidence
// histogram behind the top-label ECE, and the NLL and Brier sums — the read-out of the reference's `ECE, NLL, MSE` row
// (SA/train/results_analyzer.py:446-503) from the T-mean probabilities, without a host copy of them.  THE ARITHMETIC CONTRACT (restated in
// numpy, loop by loop, as train.reliability.reliability_numpy):
//
// Input    mean float64 [E][B][C], the T-mean probabilities (bmi_finalize's `mean`); labels int32 [B].
// Rows     R = 2 E rows r = kind * E + e:  kind 0 is p_e = mean[e];  kind 1 is the exit ensemble q_e = (p_0 + ... + p_e) / (e + 1), added in
//          exit order from exit 0 onto 0.0, then divided once (results_analyzer.exit_ensembles).
// Per row and image, v = the row's C values, y = labels[b]; float64 and no fused multiply-add wherever a number is formed:
//     pc_c  = max(v_c, 1e-256)                       (the reference's upper clip 1 - 1e-256 is 1.0 in float64: a no-op)
//     s     = ((0.0 + pc_0) + pc_1) + ...            ascending class order
//     pred  = the lowest c with pc_c = max_c pc      (numpy's argmax)
//     conf  = (float) (pc_pred / s),   key = the float32 bit pattern of conf as a uint32 (for positive floats the unsigned order of the
//                                      keys is the float order)
//     hit   = (pred == y),   nll = -log(pc_y),   brier = ((0.0 + d_0^2) + d_1^2) + ...,  d_c = v_c - [c == y]     (the unclipped v)
// Invalid  an image whose label is outside [0, C): key 0, hit 0, nll = brier = 0.0 in all R rows, counters[1] += 1, nothing of it is read.
//          Otherwise a row with a non-finite v_c: key 0, hit 0, nll = brier = 0.0 for that (row, image), counters[0] += 1 (an exit with a
//          non-finite value makes every ensemble from it on non-finite).  No NaN reaches an output.
// Edges    binning by mass (train.metrics.ece_hist_binary): per = N / n_bins (integer), edges[0] = 0, edges[i + 1] = the order statistic of
//          rank min((i + 1) * per, N - 1) (0-based, ascending) of the row's N keys, edges[n_bins] = 1.  Fixed edges: the caller's, as given.
// Bins     image n is in the one bin i with edges[i] < conf <= edges[i + 1]; a zero-width bin stays empty; key 0 is in none.
// Table    per row: int64 count[n_bins], hits[n_bins], conf_fix[n_bins] = sum (int64) (conf * 2^40) — exact: C <= 128 keeps conf above 2^-8,
//          where the float32 ulp is 2^-31, so every conf is a multiple of 2^-40; the sum fits for N < 2^22 —, float32 edges[n_bins + 1],
//          float64 nll_sum and brier_sum, each added in image order n = 0, 1, ... from 0.0.
// Integer atomics only (LDS); every output is OVERWRITTEN; the same bits on every run, however the N images were cut into record calls.
//
// The shared pieces are record_common.h's: walk_exit_rows, class_sums, radix_select_u32, bin_of / conf_fix40, ordered_sum.
//
//   reliability_records_kernel  one wave per image walks its rows (walk_exit_rows); s and the Brier term are one pass of class_sums<2>, the
//                               arg-max a butterfly on (value, lower index).  Lane 0 writes the 2 E records of the image at column n0 + b.
//   line_edges_kernel           one workgroup per (edge, line of N_cap keys): the order statistic by radix_select_u32.  The lines are the R
//                               rows here and the R C (row, class) lines of reliability_classwise.hip (launch_line_edges); a line is read
//                               4 (n_bins - 1) times.
//   reliability_partial_kernel  one workgroup per (chunk of RL_CHUNK images, row): the three integer bin sums of the chunk in LDS, written to
//                               the scratch.
//   reliability_bins_kernel     one workgroup per row: the chunks' integers added up (order-free); the two float64 sums by ordered_sum<2>.
#include <cmath>
#include <cstdint>

#include "record_common.h"

#define RL_THREADS RECORD_THREADS
#define RL_CHUNK 4096

__global__ __launch_bounds__(RL_THREADS) void reliability_records_kernel(const double* __restrict__ mean, int E, int B, int C,
                                                                         const int* __restrict__ labels, size_t n0, size_t N_cap,
                                                                         uint32_t* __restrict__ keys, uint8_t* __restrict__ hit,
                                                                         double* __restrict__ nll, double* __restrict__ brier, int* counters) {
#pragma clang fp contract(off)
    const long long w = ((long long)blockIdx.x * RL_THREADS + threadIdx.x) >> 6;       // the image, wave-uniform
    if (w >= B) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)w;
    const int y = labels[b];
    const size_t col = n0 + (size_t)b;
    if ((unsigned)y >= (unsigned)C) {       // (wave-uniform)
        for (int r = lane; r < 2 * E; r += 64) {
            keys[r * N_cap + col] = 0u;
            hit[r * N_cap + col] = 0;
            nll[r * N_cap + col] = 0.0;
            brier[r * N_cap + col] = 0.0;
        }
        if (lane == 0 && counters) atomicAdd(counters + 1, 1);
        return;
    }
    const int c0 = lane, c1 = lane + 64;
    const double t0 = c0 == y ? 1.0 : 0.0, t1 = c1 == y ? 1.0 : 0.0;
    int bad_rows = 0;
    walk_exit_rows(mean, E, B, C, b, lane, [&](int r, bool bad, double v0, double v1, double pc0, double pc1) {
        uint32_t key = 0u;
        uint8_t h = 0;
        double nl = 0.0, br = 0.0;
        if (bad) {                          // (wave-uniform)
            ++bad_rows;
        } else {
            const double d0 = v0 - t0, d1 = v1 - t1;
            const double lo[2] = {pc0, d0 * d0}, hi[2] = {pc1, d1 * d1};
            double sum[2];                  // s and the Brier term, in one pass over the classes
            class_sums<2>(lo, hi, C, sum);
            br = sum[1];
            double bv = pc0;
            int bi = c0;
            if (pc1 > bv) { bv = pc1; bi = c1; }
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const double ov = __shfl_xor(bv, k);
                const int oi = __shfl_xor(bi, k);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            key = __float_as_uint((float)(bv / sum[0]));
            h = bi == y;
            nl = -log(__shfl(y < 64 ? pc0 : pc1, y & 63));
        }
        if (lane == 0) {
            const size_t at = (size_t)r * N_cap + col;
            keys[at] = key;
            hit[at] = h;
            nll[at] = nl;
            brier[at] = br;
        }
    });
    if (lane == 0 && counters && bad_rows) atomicAdd(counters, bad_rows);
}

// grid (n_bins, L) by mass: workgroup (i, l) writes edges[l][i + 1] for i < n_bins - 1; workgroup (n_bins - 1, l) writes edges[l][0] and
// [n_bins].  grid (1, L) with fixed edges: workgroup (0, l) copies them.  A selected INVALID key (all ones: classwise lines only) is the
// edge 1.0f.
__global__ __launch_bounds__(RL_THREADS) void line_edges_kernel(const uint32_t* __restrict__ keys, int N, size_t N_cap, int n_bins,
                                                                BinEdges fixed, int use_fixed, float* __restrict__ edges) {
    __shared__ int hist[256];
    __shared__ int chosen[2];
    const int i = blockIdx.x, tid = threadIdx.x;
    const size_t l = blockIdx.y;
    float* out = edges + l * (n_bins + 1);
    if (use_fixed) {
        if (tid <= n_bins) out[tid] = fixed.v[tid];
        return;
    }
    if (i == n_bins - 1) {
        if (tid == 0) {
            out[0] = 0.f;
            out[n_bins] = 1.f;
        }
        return;
    }
    const long long want = (long long)(i + 1) * (N / n_bins);
    const uint32_t key = radix_select_u32(keys + l * N_cap, N, (int)(want < N - 1 ? want : N - 1), hist, chosen);
    if (tid == 0) out[i + 1] = key == 0xFFFFFFFFu ? 1.f : __uint_as_float(key);
}

// grid (chunks, R); part int64 [R][chunks][3][n_bins]: count, hits, conf_fix of the chunk's images
__global__ __launch_bounds__(RL_THREADS) void reliability_partial_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ hit, int N,
                                                                         size_t N_cap, int n_bins, const float* __restrict__ edges,
                                                                         long long* __restrict__ part) {
    __shared__ float ed[BMI_REL_MAX_BINS + 1];
    __shared__ unsigned long long acc[3][BMI_REL_MAX_BINS];
    const int chunk = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (tid <= n_bins) ed[tid] = edges[(size_t)r * (n_bins + 1) + tid];
    if (tid < n_bins) acc[0][tid] = acc[1][tid] = acc[2][tid] = 0ull;
    __syncthreads();
    const int begin = chunk * RL_CHUNK, end = min(N, begin + RL_CHUNK);
    for (int n = begin + tid; n < end; n += RL_THREADS) {
        const uint32_t key = keys[(size_t)r * N_cap + n];
        if (key == 0u) continue;
        const float conf = __uint_as_float(key);
        const int j = bin_of(conf, ed, n_bins, false);
        if (j == n_bins) continue;
        atomicAdd(&acc[0][j], 1ull);
        if (hit[(size_t)r * N_cap + n]) atomicAdd(&acc[1][j], 1ull);
        atomicAdd(&acc[2][j], conf_fix40(conf));
    }
    __syncthreads();
    if (tid < n_bins) {
        long long* p = part + ((size_t)r * gridDim.x + chunk) * 3 * n_bins;
        p[tid] = (long long)acc[0][tid];
        p[n_bins + tid] = (long long)acc[1][tid];
        p[2 * n_bins + tid] = (long long)acc[2][tid];
    }
}

__global__ __launch_bounds__(RL_THREADS) void reliability_bins_kernel(const double* __restrict__ nll, const double* __restrict__ brier, int N,
                                                                      size_t N_cap, int n_bins, int chunks, const long long* __restrict__ part,
                                                                      long long* __restrict__ count, long long* __restrict__ hits,
                                                                      long long* __restrict__ conf_fix, double* __restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double tile[2][RL_TILE];     // the next RL_TILE nll and brier records of the row
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid < n_bins) {
        long long a = 0, h = 0, f = 0;
        for (int c = 0; c < chunks; ++c) {
            const long long* p = part + ((size_t)r * chunks + c) * 3 * n_bins;
            a += p[tid];
            h += p[n_bins + tid];
            f += p[2 * n_bins + tid];
        }
        count[(size_t)r * n_bins + tid] = a;
        hits[(size_t)r * n_bins + tid] = h;
        conf_fix[(size_t)r * n_bins + tid] = f;
    }
    const double* nl = nll + (size_t)r * N_cap;
    const double* br = brier + (size_t)r * N_cap;
    double sum[2] = {0.0, 0.0};             // image order
    ordered_sum<2>(N, tile, sum, [&](int n, double (&t)[2]) {
        t[0] = nl[n];
        t[1] = br[n];
    });
    if (tid == 0) {
        sums[2 * r] = sum[0];
        sums[2 * r + 1] = sum[1];
    }
}

bool reliability_record_takes(int E, int B, int C) {
    return E >= 1 && B >= 1 && C >= 1 && C <= BMI_ENS_MAX_CLASSES && E <= BMI_ENS_MAX_EXITS && B <= INT32_MAX / 64;       // (64 threads per image)
}

bool reliability_table_takes(int R, int N, int n_bins) {
    return R >= 1 && N >= 1 && n_bins >= 1 && n_bins <= BMI_REL_MAX_BINS && R <= 2 * BMI_ENS_MAX_EXITS && N < BMI_REL_MAX_IMAGES;
}

size_t reliability_scratch_bytes(int R, int N, int n_bins) {
    if (!reliability_table_takes(R, N, n_bins)) return 0;
    return (size_t)R * ((N + RL_CHUNK - 1) / RL_CHUNK) * 3 * n_bins * sizeof(long long);
}

int launch_reliability_record(const double* mean, int E, int B, int C, const int* labels, int n0, int N_cap, uint32_t* keys, uint8_t* hit,
                              double* nll, double* brier, int* counters, hipStream_t s) {
    if (!reliability_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)(((int64_t)B * 64 + RL_THREADS - 1) / RL_THREADS);
    hipLaunchKernelGGL(reliability_records_kernel, dim3(grid), dim3(RL_THREADS), 0, s, mean, E, B, C, labels, (size_t)n0, (size_t)N_cap, keys, hit,
                       nll, brier, counters);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_line_edges(const uint32_t* keys, int L, int N, int N_cap, int n_bins, const float* edges_in, float* edges_out, hipStream_t s) {
    BinEdges fixed = {};
    if (edges_in)
        for (int i = 0; i <= n_bins; ++i) fixed.v[i] = edges_in[i];
    hipLaunchKernelGGL(line_edges_kernel, dim3(edges_in ? 1u : (unsigned)n_bins, (unsigned)L), dim3(RL_THREADS), 0, s, keys, N, (size_t)N_cap, n_bins,
                       fixed, edges_in ? 1 : 0, edges_out);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_reliability_table(const uint32_t* keys, const uint8_t* hit, const double* nll, const double* brier, int R, int N, int N_cap, int n_bins,
                             const float* edges_in, float* edges_out, long long* count, long long* hits, long long* conf_fix, double* sums,
                             void* scratch, hipStream_t s) {
    if (!reliability_table_takes(R, N, n_bins)) return BMI_ERR_UNSUPPORTED;
    const int chunks = (N + RL_CHUNK - 1) / RL_CHUNK;
    long long* part = (long long*)scratch;
    const int rc = launch_line_edges(keys, R, N, N_cap, n_bins, edges_in, edges_out, s);
    if (rc != BMI_OK) return rc;
    hipLaunchKernelGGL(reliability_partial_kernel, dim3((unsigned)chunks, (unsigned)R), dim3(RL_THREADS), 0, s, keys, hit, N, (size_t)N_cap, n_bins,
                       (const float*)edges_out, part);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(reliability_bins_kernel, dim3((unsigned)R), dim3(RL_THREADS), 0, s, nll, brier, N, (size_t)N_cap, n_bins, chunks,
                       (const long long*)part, count, hits, conf_fix, sums);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
