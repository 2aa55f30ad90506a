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
//   classwise_records_kernel  one wave per image walks the exits and keeps the running exit sum; lane i owns classes i and i + 64.  The
//                             ascending sum is formed by every lane from the same broadcast values (v_readlane: the class index is
//                             wave-uniform), as reliability_records_kernel forms it.  Each lane writes the keys of its own classes for the
//                             2 E rows at column n0 + b; lane 0 writes the label record.
//   classwise_edges_kernel    one workgroup per (edge, line), line = (row, class): the order statistic by radix select over the uint32 keys,
//                             four passes of eight bits, each a 256-bin LDS histogram (integer atomics) of the keys that match the digits
//                             chosen so far and a one-wave scan for the digit that holds the rank.  Exact under any number of duplicate
//                             keys; no sort.  A thread adds a run of equal digits with ONE atomic (near-zero probabilities share their top
//                             digits: every lane would otherwise hit one address).  The simple form: a line is read 4 (n_bins - 1) times.
//   classwise_bins_kernel     one workgroup per line: the three integer bin sums in LDS (a thread adds a run of pairs of one bin at once),
//                             written straight to the outputs — no scratch —; the workgroups of class 0 count the row's valid images.
#include <cmath>
#include <cstdint>

#include "kernels.h"

#define CW_THREADS 256
#define CW_INVALID 0xFFFFFFFFu

// lane `from`'s value in every lane; `from` is the same in every lane
__device__ __forceinline__ double cw_broadcast(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}

struct CwEdges { float v[BMI_REL_MAX_BINS + 1]; };

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
            uint32_t key0 = CW_INVALID, key1 = CW_INVALID;
            if (bad) {                      // (wave-uniform)
                ++bad_rows;
            } else {
                const double pc0 = v0 < 1e-256 ? 1e-256 : v0, pc1 = v1 < 1e-256 ? 1e-256 : v1;       // (a class beyond C: never read)
                double s = 0.0;
                for (int c = 0; c < n_lo; ++c) s = s + cw_broadcast(pc0, c);           // ascending class order, the same values in every lane
                for (int c = 64; c < C; ++c) s = s + cw_broadcast(pc1, c - 64);
                const double q0 = pc0 / s, q1 = pc1 / s;
                key0 = q0 < 0x1p-126 ? 0u : __float_as_uint((float)q0);
                key1 = q1 < 0x1p-126 ? 0u : __float_as_uint((float)q1);
            }
            const size_t at = (size_t)(kind * E + e) * plane;
            if (in0) k0[at] = key0;
            if (in1) k1[at] = key1;
        }
    }
    if (lane == 0) {
        labels_rec[col] = y;
        if (counters && bad_rows) atomicAdd(counters, bad_rows);
    }
}

// grid (n_bins, L) by mass: workgroup (i, l) writes edges[l][i + 1] for i < n_bins - 1; workgroup (n_bins - 1, l) writes edges[l][0] and
// [n_bins].  grid (1, L) with fixed edges: workgroup (0, l) copies them.
__global__ __launch_bounds__(CW_THREADS) void classwise_edges_kernel(const uint32_t* __restrict__ pkeys, int N, size_t N_cap, int n_bins,
                                                                     CwEdges fixed, int use_fixed, float* __restrict__ edges) {
    __shared__ int hist[256];
    __shared__ int chosen[2];               // the digit that holds the rank, the rank inside it
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
    const uint32_t* k = pkeys + l * N_cap;
    const long long want = (long long)(i + 1) * (N / n_bins);
    int rank = (int)(want < N - 1 ? want : N - 1);
    uint32_t prefix = 0u, mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        int cur = -1, run = 0;              // the thread's run of equal digits, added at once
        for (int n = tid; n < N; n += CW_THREADS) {
            const uint32_t key = k[n];
            if ((key & mask) != prefix) continue;
            const int d = (int)((key >> shift) & 255u);
            if (d != cur) {
                if (run) atomicAdd(&hist[cur], run);
                cur = d;
                run = 0;
            }
            ++run;
        }
        if (run) atomicAdd(&hist[cur], run);
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
    if (tid == 0) out[i + 1] = prefix == CW_INVALID ? 1.f : __uint_as_float(prefix);
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
        if (!(conf >= ed[0])) continue;
        int j = 1;                          // the lowest edge conf does not exceed
        while (j <= n_bins && conf > ed[j]) ++j;
        if (j > n_bins) continue;
        if (j - 1 != cur) {
            if (a) {
                atomicAdd(&acc[0][cur], a);
                atomicAdd(&acc[1][cur], h);
                atomicAdd(&acc[2][cur], f);
            }
            cur = j - 1;
            a = h = f = 0ull;
        }
        ++a;
        h += labels_rec[n] == c ? 1ull : 0ull;
        f += (unsigned long long)(long long)((double)conf * 1099511627776.0);
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
    CwEdges fixed = {};
    if (edges_in)
        for (int i = 0; i <= n_bins; ++i) fixed.v[i] = edges_in[i];
    const unsigned L = (unsigned)(R * C);   // at most 64 * 128 lines
    hipLaunchKernelGGL(classwise_edges_kernel, dim3(edges_in ? 1u : (unsigned)n_bins, L), dim3(CW_THREADS), 0, s, pkeys, N, (size_t)N_cap, n_bins,
                       fixed, edges_in ? 1 : 0, edges_out);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(classwise_bins_kernel, dim3(L), dim3(CW_THREADS), 0, s, pkeys, labels_rec, C, N, (size_t)N_cap, n_bins,
                       (const float*)edges_out, count, hits, conf_fix, valid);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
