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
//   reliability_records_kernel  one wave per image walks the exits and keeps the running exit sum; lane i owns classes i and i + 64.  The two
//                               ascending sums are formed by every lane from the same broadcast values (v_readlane: the class index is
//                               wave-uniform), the arg-max by a butterfly on (value, lower index).  Lane 0 writes the 2 E records of the
//                               image at column n0 + b.
//   reliability_edges_kernel    one workgroup per (row, edge): the order statistic by radix select over the uint32 keys, four passes of eight
//                               bits, each a 256-bin LDS histogram (integer atomics) of the keys that match the digits chosen so far and a
//                               one-wave scan for the digit that holds the rank.  Exact under any number of duplicate keys; no sort.
//   reliability_partial_kernel  one workgroup per (chunk of RL_CHUNK images, row): the three integer bin sums of the chunk in LDS, written to
//                               the scratch.
//   reliability_bins_kernel     one workgroup per row: the chunks' integers added up (order-free); the two float64 sums added in image order
//                               by ONE wave, from tiles of RL_TILE records the workgroup stages in LDS (every lane adds the same values).
#include <cmath>
#include <cstdint>

#include "kernels.h"

#define RL_THREADS 256
#define RL_CHUNK 4096

// lane `from`'s value in every lane; `from` is the same in every lane
__device__ __forceinline__ double rl_broadcast(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}

struct RlEdges { float v[BMI_REL_MAX_BINS + 1]; };

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
    const bool in0 = c0 < C, in1 = c1 < C;
    const double t0 = c0 == y ? 1.0 : 0.0, t1 = c1 == y ? 1.0 : 0.0;
    const int n_lo = min(C, 64);
    double a0 = 0.0, a1 = 0.0;              // the running exit sum of the two owned classes
    int bad_rows = 0;
    for (int e = 0; e < E; ++e) {
        const double* row = mean + ((size_t)e * B + b) * C;
        const double p0 = in0 ? row[c0] : 0.0, p1 = in1 ? row[c1] : 0.0;
        a0 = a0 + p0;
        a1 = a1 + p1;
        const double div = (double)(e + 1);
        for (int kind = 0; kind < 2; ++kind) {
            const double v0 = kind ? a0 / div : p0, v1 = kind ? a1 / div : p1;
            const bool bad = __ballot((in0 && !__builtin_isfinite(v0)) || (in1 && !__builtin_isfinite(v1))) != 0ull;
            uint32_t key = 0u;
            uint8_t h = 0;
            double nl = 0.0, br = 0.0;
            if (bad) {                      // (wave-uniform)
                ++bad_rows;
            } else {
                // (a class beyond C: -1.0, below every clipped value)
                const double pc0 = in0 ? (v0 < 1e-256 ? 1e-256 : v0) : -1.0, pc1 = in1 ? (v1 < 1e-256 ? 1e-256 : v1) : -1.0;
                const double d0 = v0 - t0, d1 = v1 - t1;
                const double q0 = d0 * d0, q1 = d1 * d1;
                double s = 0.0;
                for (int c = 0; c < n_lo; ++c) {           // ascending class order, the same values in every lane
                    s = s + rl_broadcast(pc0, c);
                    br = br + rl_broadcast(q0, c);
                }
                for (int c = 64; c < C; ++c) {
                    s = s + rl_broadcast(pc1, c - 64);
                    br = br + rl_broadcast(q1, c - 64);
                }
                double bv = pc0;
                int bi = c0;
                if (pc1 > bv) { bv = pc1; bi = c1; }
#pragma unroll
                for (int k = 32; k >= 1; k >>= 1) {
                    const double ov = __shfl_xor(bv, k);
                    const int oi = __shfl_xor(bi, k);
                    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                key = __float_as_uint((float)(bv / s));
                h = bi == y;
                nl = -log(__shfl(y < 64 ? pc0 : pc1, y & 63));
            }
            if (lane == 0) {
                const size_t at = (size_t)(kind * E + e) * N_cap + col;
                keys[at] = key;
                hit[at] = h;
                nll[at] = nl;
                brier[at] = br;
            }
        }
    }
    if (lane == 0 && counters && bad_rows) atomicAdd(counters, bad_rows);
}

// grid (n_bins, R): workgroup (i, r) writes edges[r][i + 1] for i < n_bins - 1; workgroup (n_bins - 1, r) writes edges[r][0] and [n_bins]
__global__ __launch_bounds__(RL_THREADS) void reliability_edges_kernel(const uint32_t* __restrict__ keys, int N, size_t N_cap, int n_bins,
                                                                       RlEdges fixed, int use_fixed, float* __restrict__ edges) {
    __shared__ int hist[256];
    __shared__ int chosen[2];               // the digit that holds the rank, the rank inside it
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    float* out = edges + (size_t)r * (n_bins + 1);
    if (i == n_bins - 1) {
        if (tid == 0) {
            out[0] = use_fixed ? fixed.v[0] : 0.f;
            out[n_bins] = use_fixed ? fixed.v[n_bins] : 1.f;
        }
        return;
    }
    if (use_fixed) {
        if (tid == 0) out[i + 1] = fixed.v[i + 1];
        return;
    }
    const uint32_t* k = keys + (size_t)r * N_cap;
    const long long want = (long long)(i + 1) * (N / n_bins);
    int rank = (int)(want < N - 1 ? want : N - 1);
    uint32_t prefix = 0u, mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int n = tid; n < N; n += RL_THREADS) {
            const uint32_t key = k[n];
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < 64) {                     // lane l owns digits 4 l .. 4 l + 3; the keys that match the prefix number more than rank
            const int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const int tot = h0 + h1 + h2 + h3;
            int incl = tot;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (tid >= d) incl += up;
            }
            const int excl = incl - tot;
            if (excl <= rank && rank < incl) {       // exactly one lane
                int digit = 4 * tid, left = rank - excl;
                if (left >= h0) {
                    left -= h0; ++digit;
                    if (left >= h1) {
                        left -= h1; ++digit;
                        if (left >= h2) { left -= h2; ++digit; }
                    }
                }
                chosen[0] = digit;
                chosen[1] = left;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)chosen[0] << shift;
        mask |= 255u << shift;
        rank = chosen[1];
        __syncthreads();                    // (chosen and hist are rewritten by the next pass)
    }
    if (tid == 0) out[i + 1] = __uint_as_float(prefix);
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
        if (!(conf > ed[0])) continue;
        int j = 1;                          // the lowest edge conf does not exceed
        while (j <= n_bins && conf > ed[j]) ++j;
        if (j > n_bins) continue;
        atomicAdd(&acc[0][j - 1], 1ull);
        if (hit[(size_t)r * N_cap + n]) atomicAdd(&acc[1][j - 1], 1ull);
        atomicAdd(&acc[2][j - 1], (unsigned long long)(long long)((double)conf * 1099511627776.0));
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
    double s = 0.0, t = 0.0;                // (wave 0's; every lane of it adds the same values)
    for (int n0 = 0; n0 < N; n0 += RL_TILE) {
        const int len = min(RL_TILE, N - n0);
        for (int j = tid; j < len; j += RL_THREADS) {
            tile[0][j] = nl[n0 + j];
            tile[1][j] = br[n0 + j];
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll 8
            for (int j = 0; j < len; ++j) {  // image order
                s = s + tile[0][j];
                t = t + tile[1][j];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        sums[2 * r] = s;
        sums[2 * r + 1] = t;
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

int launch_reliability_table(const uint32_t* keys, const uint8_t* hit, const double* nll, const double* brier, int R, int N, int N_cap, int n_bins,
                             const float* edges_in, float* edges_out, long long* count, long long* hits, long long* conf_fix, double* sums,
                             void* scratch, hipStream_t s) {
    if (!reliability_table_takes(R, N, n_bins)) return BMI_ERR_UNSUPPORTED;
    RlEdges fixed = {};
    if (edges_in)
        for (int i = 0; i <= n_bins; ++i) fixed.v[i] = edges_in[i];
    const int chunks = (N + RL_CHUNK - 1) / RL_CHUNK;
    long long* part = (long long*)scratch;
    hipLaunchKernelGGL(reliability_edges_kernel, dim3((unsigned)n_bins, (unsigned)R), dim3(RL_THREADS), 0, s, keys, N, (size_t)N_cap, n_bins, fixed,
                       edges_in ? 1 : 0, edges_out);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(reliability_partial_kernel, dim3((unsigned)chunks, (unsigned)R), dim3(RL_THREADS), 0, s, keys, hit, N, (size_t)N_cap, n_bins,
                       (const float*)edges_out, part);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(reliability_bins_kernel, dim3((unsigned)R), dim3(RL_THREADS), 0, s, nll, brier, N, (size_t)N_cap, n_bins, chunks,
                       (const long long*)part, count, hits, conf_fix, sums);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
