// What the evaluation read-outs over the T-mean probabilities share (reliability.hip, reliability_classwise.hip, reliability_kde.hip,
// ranking.hip), defined once so that the contracts their headers state of each other — "the same s", "bit for bit the key" — hold by
// construction: the exit-row walk of a record kernel, the ascending class sum, the key select behind the mass edges, the bin search and
// the ordered sum.  Device functions and small templates, no state.  Every workgroup here has RECORD_THREADS threads.
#pragma once
#include <cstdint>

#include "kernels.h"

#define RECORD_THREADS 256
#define RL_TILE 1024        // terms a workgroup stages in LDS per step of an ordered sum

struct BinEdges { float v[BMI_REL_MAX_BINS + 1]; };

// lane `from`'s value in every lane; `from` is the same in every lane
__device__ __forceinline__ double wave_broadcast(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}

// The rows of one image, walked by ONE wave; lane i owns classes i and i + 64.  Per exit e the two owned classes of mean[e][b] are loaded
// (0.0 beyond C) and added onto the running exit sum; per row r = kind * E + e the row's values are v = p (kind 0) or a / (e + 1) (kind 1).
// body(r, bad, v0, v1, pc0, pc1): bad (wave-uniform) when a v_c of the row is non-finite — the caller counts the row and reads no pc —, else
// pc = max(v, 1e-256), -1.0 (below every clipped value) for a class beyond C.  float64, no fused multiply-add.
template <class Body>
__device__ __forceinline__ void walk_exit_rows(const double* __restrict__ mean, int E, int B, int C, int b, int lane, Body body) {
#pragma clang fp contract(off)
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < C, in1 = c1 < C;
    double a0 = 0.0, a1 = 0.0;              // the running exit sum of the two owned classes
    for (int e = 0; e < E; ++e) {
        const double* row = mean + ((size_t)e * B + b) * C;
        const double p0 = in0 ? row[c0] : 0.0, p1 = in1 ? row[c1] : 0.0;
        a0 = a0 + p0;
        a1 = a1 + p1;
        const double div = (double)(e + 1);
        for (int kind = 0; kind < 2; ++kind) {
            const double v0 = kind ? a0 / div : p0, v1 = kind ? a1 / div : p1;
            const bool bad = __ballot((in0 && !__builtin_isfinite(v0)) || (in1 && !__builtin_isfinite(v1))) != 0ull;
            body(kind * E + e, bad, v0, v1, in0 ? (v0 < 1e-256 ? 1e-256 : v0) : -1.0, in1 ? (v1 < 1e-256 ? 1e-256 : v1) : -1.0);
        }
    }
}

// K sums at once over the classes, each ((0.0 + x_0) + x_1) + ... in ascending class order: lo[k] is the lane's value of class `lane`,
// hi[k] of class `lane + 64`.  Every lane adds the same broadcast values (v_readlane: the class index is wave-uniform).
template <int K>
__device__ __forceinline__ void class_sums(const double (&lo)[K], const double (&hi)[K], int C, double (&sum)[K]) {
#pragma clang fp contract(off)
    const int n_lo = min(C, 64);
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] = 0.0;
    for (int c = 0; c < n_lo; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) sum[k] = sum[k] + wave_broadcast(lo[k], c);
    for (int c = 64; c < C; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) sum[k] = sum[k] + wave_broadcast(hi[k], c - 64);
}

// The order statistic of `rank` (0-based, ascending, unsigned order) of line[0 .. N-1], by the whole workgroup, in every thread: a radix
// select, four passes of eight bits, each a 256-bin LDS histogram (integer atomics) of the keys that match the digits chosen so far and a
// one-wave scan for the digit that holds the rank.  Exact under any number of duplicate keys; no sort.  A thread adds a run of equal
// digits with ONE atomic (keys that share their top digits would otherwise send every lane to one address).  hist [256], chosen [2]: LDS.
__device__ __forceinline__ uint32_t radix_select_u32(const uint32_t* __restrict__ line, int N, int rank, int* hist, int* chosen) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0u, mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        int cur = -1, run = 0;              // the thread's run of equal digits, added at once
        for (int n = tid; n < N; n += RECORD_THREADS) {
            const uint32_t key = line[n];
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
                chosen[0] = digit;           // the digit that holds the rank, the rank inside it
                chosen[1] = left;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)chosen[0] << shift;
        mask |= 255u << shift;
        rank = chosen[1];
        __syncthreads();                    // (chosen and hist are rewritten by the next pass)
    }
    return prefix;
}

// the bin of conf among ed[0 .. n_bins]: the lowest j with conf <= ed[j + 1], for conf above ed[0] — or at it, where bin 0 is closed at
// its lower edge —; n_bins for a conf in no bin
__device__ __forceinline__ int bin_of(float conf, const float* ed, int n_bins, bool closed_low) {
    if (!(closed_low ? conf >= ed[0] : conf > ed[0])) return n_bins;
    int j = 0;                              // one below the lowest edge conf does not exceed
    while (j < n_bins && conf > ed[j + 1]) ++j;
    return j;
}

// (int64) (conf * 2^40), truncating, as the unsigned word the integer atomics add
__device__ __forceinline__ unsigned long long conf_fix40(float conf) {
    return (unsigned long long)(long long)((double)conf * 1099511627776.0);
}

// K sums at once of n terms each, acc[k] = (acc[k] + t_0[k]) + t_1[k] + ... in index order, the same bits however the work is spread:
// the workgroup stages tiles of RL_TILE terms in LDS — term(i, t) forms the K terms of index i —, and ONE wave adds a tile in order, every
// lane of it adding the same values.  acc is wave 0's.  term runs exactly ONCE per index, in the thread that stages it (index i in thread
// i % RECORD_THREADS): it may count on the side.  float64, no fused multiply-add.
template <int K, class Term>
__device__ __forceinline__ void ordered_sum(int n, double (*tile)[RL_TILE], double (&acc)[K], Term term) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int i0 = 0; i0 < n; i0 += RL_TILE) {
        const int len = min(RL_TILE, n - i0);
        for (int j = tid; j < len; j += RECORD_THREADS) {
            double t[K];
            term(i0 + j, t);
#pragma unroll
            for (int k = 0; k < K; ++k) tile[k][j] = t[k];
        }
        __syncthreads();
        if (tid < 64) {
#pragma unroll 8
            for (int j = 0; j < len; ++j)
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = acc[k] + tile[k][j];
        }
        __syncthreads();
    }
}
