// The exit walk of one (pass, image) of the vote kernels, shared by votes.hip (vote_counts_kernel: every image, every exit) and
// votes_rows.hip (vote_counts_rows_kernel: the images of a list, of each its first n_e[b] exits) — head_fused_body.h's arrangement: one
// body, the kernels keep their own names and arguments.  The arithmetic is stated at the top of votes.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels.h"

#define VOTE_THREADS 256
#define VOTE_LDS_BYTES 65536      // what a launch may ask for without an attribute: the weighted form's waves per block follow from it

enum { VOTE_MAP_NONE = 0, VOTE_MAP_TEMP = 1, VOTE_MAP_VEC = 2, VOTE_MAP_MAT = 3 };

struct VoteTau { float inv[BMI_ENS_MAX_EXITS]; };

// The lowest class of a row whose value equals the row's maximum `mx`: hit0 / hit1 = this lane's class c0 = lane / c1 = lane + 64 holds it.
// -1: nobody does (a row of NaNs)
__device__ __forceinline__ int vote_winner(bool hit0, bool hit1) {
    const unsigned long long b0 = __ballot(hit0);
    if (b0) return __ffsll(b0) - 1;
    const unsigned long long b1 = __ballot(hit1);
    return b1 ? 64 + __ffsll(b1) - 1 : -1;
}

// One wave walks exits 0 .. En-1 of pass t and image b (both wave-uniform) of logits / V laid out for E exits and B images; pw = this
// lane's word of the wave's [E][2][64] float64 LDS (WEIGHTED only).  Exits e >= En are neither read nor written.
template <int MAP, bool WEIGHTED>
__device__ __forceinline__ void vote_walk(const float* __restrict__ logits, int t, int b, int lane, int E, int En, int B, int C, const VoteTau& tau,
                                          const float* __restrict__ ma, const float* __restrict__ mb, const double* __restrict__ W,
                                          int* __restrict__ V, int* nonfinite, double* const pw) {
#pragma clang fp contract(off)
    const int c0 = lane, c1 = lane + 64;
    const bool in0 = c0 < C, in1 = c1 < C;
    const bool two = C > 64;                              // (wave-uniform: the upper half exists)
    double s0 = 0.0, s1 = 0.0;                            // the running exit sum of the two owned classes
    bool ens_ok = true;                                   // no bad row among the exits so far
    int bad_rows = 0;
    for (int e = 0; e < En; ++e) {
        const float* row = logits + (((size_t)t * E + e) * B + b) * C;
        float z0 = -INFINITY, z1 = -INFINITY;
        if constexpr (MAP == VOTE_MAP_MAT) {
            // (the rows of M of this lane's classes; an absent class reads row 0 of the exit and is dropped below)
            const float* m0 = ma + ((size_t)e * C + (in0 ? c0 : 0)) * C;
            const float* m1 = ma + ((size_t)e * C + (in1 ? c1 : 0)) * C;
            const float l_0 = row[0];
            float a0 = m0[0] * l_0, a1 = two ? m1[0] * l_0 : 0.f;
            for (int j = 1; j < C; ++j) {
                const float lj = row[j];
                const float pr0 = m0[j] * lj;
                a0 = a0 + pr0;
                if (two) {
                    const float pr1 = m1[j] * lj;
                    a1 = a1 + pr1;
                }
            }
            if (in0) z0 = a0 + mb[(size_t)e * C + c0];
            if (in1) z1 = a1 + mb[(size_t)e * C + c1];
        } else {
            const float l0 = in0 ? row[c0] : 0.f, l1 = in1 ? row[c1] : 0.f;
            if constexpr (MAP == VOTE_MAP_NONE) {
                if (in0) z0 = l0;
                if (in1) z1 = l1;
            } else if constexpr (MAP == VOTE_MAP_TEMP) {
                const float inv = tau.inv[e];
                if (in0) z0 = l0 * inv;
                if (in1) z1 = l1 * inv;
            } else {
                if (in0) { const float pr = l0 * ma[(size_t)e * C + c0]; z0 = pr + mb[(size_t)e * C + c0]; }
                if (in1) { const float pr = l1 * ma[(size_t)e * C + c1]; z1 = pr + mb[(size_t)e * C + c1]; }
            }
        }
        const bool bad = __ballot((in0 && !__builtin_isfinite(z0)) || (in1 && !__builtin_isfinite(z1))) != 0ull;
        if (bad) {                                        // (wave-uniform)
            ++bad_rows;
            ens_ok = false;
            continue;
        }
        float mx = fmaxf(z0, z1);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) mx = fmaxf(mx, __shfl_xor(mx, k));
        const int kc = vote_winner(in0 && z0 == mx, in1 && z1 == mx);
        if (kc >= 0 && kc < C && lane == (kc & 63)) atomicAdd(V + (((size_t)0 * E + e) * B + b) * C + kc, 1);
        if (!ens_ok) continue;                            // (wave-uniform: no ensemble vote behind a bad row, so no member either)
        const double e0 = in0 ? exp((double)z0 - (double)mx) : 0.0;
        double e1 = 0.0;
        if (two) e1 = in1 ? exp((double)z1 - (double)mx) : 0.0;       // (C <= 64: the upper half costs no exponential and no division)
        double s = e0 + e1;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k);
        const double p0 = e0 / s;
        double p1 = 0.0;
        if (two) p1 = e1 / s;
        double q0, q1;
        if constexpr (WEIGHTED) {
            pw[(e * 2 + 0) * 64] = p0;
            pw[(e * 2 + 1) * 64] = p1;
            const double* wr = W + (size_t)e * E;
            q0 = 0.0;
            q1 = 0.0;
            for (int i = 0; i <= e; ++i) {
                const double wi = wr[i];
                const double t0 = wi * pw[(i * 2 + 0) * 64], t1 = wi * pw[(i * 2 + 1) * 64];
                q0 = q0 + t0;
                q1 = q1 + t1;
            }
        } else {
            s0 += p0;
            s1 += p1;
            q0 = s0 / (double)(e + 1);
            q1 = s1 / (double)(e + 1);
        }
        double qm = fmax(in0 ? q0 : -INFINITY, in1 ? q1 : -INFINITY);
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) qm = fmax(qm, __shfl_xor(qm, k));
        const int kq = vote_winner(in0 && q0 == qm, in1 && q1 == qm);
        if (kq >= 0 && kq < C && lane == (kq & 63)) atomicAdd(V + (((size_t)1 * E + e) * B + b) * C + kq, 1);
    }
    if (lane == 0 && nonfinite && bad_rows) atomicAdd(nonfinite, bad_rows);
}

// What a count launch over n_waves (pass, image) pairs needs beside the kernel's own arguments (host side)
struct VoteLaunch {
    VoteTau tau;
    const float *ma, *mb;
    int map;
    bool weighted;
    unsigned grid, threads;
    size_t lds;
};

inline VoteLaunch vote_launch_plan(const Calibration& cal, int E, int64_t n_waves) {
    VoteLaunch l;
    for (int e = 0; e < BMI_ENS_MAX_EXITS; ++e) l.tau.inv[e] = e < E && e < (int)cal.inv_tau.size() ? cal.inv_tau[e] : 1.f;
    l.weighted = cal.ens_w != nullptr;
    // the weighted form keeps E x 128 float64 per wave in LDS: as many waves per block as VOTE_LDS_BYTES holds (E = 32: 2), at most 4
    const size_t wave_lds = l.weighted ? (size_t)E * 128 * sizeof(double) : 0;
    const int waves = l.weighted ? (int)std::min<size_t>(VOTE_THREADS / 64, VOTE_LDS_BYTES / wave_lds) : VOTE_THREADS / 64;
    l.grid = (unsigned)((n_waves + waves - 1) / waves);
    l.threads = (unsigned)waves * 64;
    l.lds = wave_lds * waves;
    l.ma = cal.mat ? cal.mat : cal.vec_scale;
    l.mb = cal.mat ? cal.mat_bias : cal.vec_bias;
    l.map = cal.mat ? VOTE_MAP_MAT : cal.vec_scale ? VOTE_MAP_VEC : !cal.inv_tau.empty() ? VOTE_MAP_TEMP : VOTE_MAP_NONE;
    return l;
}
