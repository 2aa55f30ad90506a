// KDE-ECE from the reliability records (bmi_reliability_kde): per exit and per exit ensemble the top-label KDE calibration error the reference
// reports as `ECE` (ece_kde_binary, SA/train/results_analyzer.py:351-443 via ece_eval_binary :497-505) — triweight kernel, bandwidth
// std(correct confidences) * (2N)^-0.2, data mirrored at 0 and 1, a grid on [-0.6, 1.6], the carry-forward rule for low-density points, a
// ratio of two trapezoids — with the densities evaluated exactly (un-binned), from the keys and hit bits bmi_reliability_record wrote.
// THE ARITHMETIC CONTRACT (restated in numpy as train.reliability.reliability_kde_numpy):
//
// Input    keys uint32 [R][N_cap], hit uint8 [R][N_cap] (columns 0 .. N-1 are read), G grid points, order in {1, 2}, bw_scale (the callers pass
//          (double)(2 N) ^ -0.2, formed on the host: no pow runs here).  All arithmetic is float64 with no fused multiply-add; division and
//          sqrt are the correctly rounded IEEE ones; no other library function is used.
// Per row r:
// Data       image n is data iff keys[r][n] != 0;  d_n = (double) float(keys[r][n]);  n = the number of data, n1 = the number of data whose
//            hit bit is set.
// Bandwidth  over the hit data, in image order, from 0.0:  s = s + d, then mu = s / n1;  q = q + (d - mu) * (d - mu), then
//            sd = sqrt(q / n1);  n1 = 0: sd = 0.  bw = (sd != 0 ? sd : 1e-16) * bw_scale,  h = 3.0 * bw.
// Grid       step = 2.2 / (G - 1),  x_i = (double) i * step + (-0.6)  (numpy's linspace formula; the last point is never inside (0, 1)).
// Sums       per grid point S1 over the hit data and S2 over all data, both in image order from 0.0.  A datum contributes two centres:
//            c = d, then its mirror, -d if d < 0.5, else 2.0 - d.  Per centre u = (x_i - c) / h, t = 1.0 - u * u; the term is t * t * t if
//            t > 0.0, else nothing.  (Adding +0.0 is the identity: a centre out of reach may be skipped without changing a bit.)
// Densities  inside = (x_i > 0.0) && (x_i < 1.0);  pp2_i = inside ? S2_i * (35.0 / 32.0) / (h * (double)(2 n)) * 2.0 : 0 — the mirrored sample
//            has 2 n points, the divisor of the reference's estimator —, pp1_i the same with S1 and n1; pp1 = 0 everywhere when n1 = 0, pp2
//            when n = 0.
// Integrand  perc = (double) n1 / n.  If max(pp1_i, pp2_i) > 1e-6: accu = min(perc * pp1_i / pp2_i, 1.0), I_i = |x_i - accu|^order * pp2_i
//            (order 2: e * e, one multiplication).  Otherwise I_i = I_{i-1} for i >= 2 and 0 for i < 2 (the reference's carry-forward,
//            :431-440).  G >= 16 puts x_0 and x_1 below 0, so neither is ever set and the rule is "the last set index <= i, else 0".
// Trapezoids over the indices with 0.0 <= x_i <= 1.0, ascending, from 0.0:  a = a + (x_{i+1} - x_i) * (I_{i+1} + I_i) / 2.0,  b the same
//            with pp2;  ece_kde = a / b.
// Degenerate n = 0, or b == 0.0 (sd = 0 — no hit, one hit, all hit confidences equal —: the 1e-16 bandwidth reaches no grid point and the
//            reference returns NaN): ece_kde = 0.0 and degenerate[r] = 1.  No NaN reaches an output: bw_scale within [2^-100, 2^100] keeps
//            every quotient above finite.
// No floating-point atomics; every output is OVERWRITTEN; the same bits on every run, however the N images were cut into record calls.
//
//   reliability_kde_moments_kernel    one workgroup per row: two ordered sums (record_common.h's ordered_sum<1>) of the hit datum's d, then of
//                                     its squared deviation, +0.0 for every other record; n and n1 are integer counts (LDS integer atomics).
//   reliability_kde_density_kernel    grid (ceil(G / 256), R), one thread per grid point: walks the images in order from LDS tiles.  A centre
//                                     is skipped when the lowest x is at least h above it or the highest x at least h below it: x, the
//                                     difference and the quotient are monotone, so then |u| >= 1 at every point between and every term is
//                                     nothing.  Twice: for the workgroup's x range when a tile is staged — an order-keeping compaction
//                                     (ballots, a count per wave) leaves only the centres in its reach in LDS —, then for the wave's.
//   reliability_kde_integrate_kernel  one workgroup per row, tiles of RK_ITILE grid points, four consecutive ones per thread: pp1, pp2 (written
//                                     over S1, S2) and the integrand where set; the carry-forward as a max-scan of "the last set index", per
//                                     thread, per wave (__shfl_up), across the waves and the tiles; the two trapezoids added by ONE wave in
//                                     index order.
#include <cmath>
#include <cstdint>

#include "record_common.h"

#pragma clang fp contract(off)

#define RK_THREADS RECORD_THREADS
#define RK_ITILE (4 * RK_THREADS)

__device__ __forceinline__ double rk_grid(int i, double step) { return (double)i * step + (-0.6); }

__global__ __launch_bounds__(RK_THREADS) void reliability_kde_moments_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ hit,
                                                                             int N, size_t N_cap, double bw_scale, long long* __restrict__ n_data,
                                                                             long long* __restrict__ n_hit, double* __restrict__ sd_out,
                                                                             double* __restrict__ bw_out) {
    __shared__ double term[1][RL_TILE];     // per record what the ordered sum receives: +0.0 (the identity on these sums) from all but the hit data
    __shared__ int count[2];                // n, n1 (integers: counted by every thread, in no order)
    __shared__ double mean;
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint32_t* k = keys + (size_t)r * N_cap;
    const uint8_t* ht = hit + (size_t)r * N_cap;
    if (tid < 2) count[tid] = 0;
    int c0 = 0, c1 = 0;
    double s[1] = {0.0}, q[1] = {0.0};      // (wave 0's), both in image order
    __syncthreads();
    ordered_sum<1>(N, term, s, [&](int n, double (&t)[1]) {
        const uint32_t key = k[n];
        const bool datum = key != 0u, hit_datum = datum && ht[n];
        c0 += datum;
        c1 += hit_datum;
        t[0] = hit_datum ? (double)__uint_as_float(key) : 0.0;
    });
    if (c0) atomicAdd(&count[0], c0);
    if (c1) atomicAdd(&count[1], c1);
    __syncthreads();
    if (tid == 0) mean = count[1] ? s[0] / (double)count[1] : 0.0;
    __syncthreads();
    const double mu = mean;
    ordered_sum<1>(N, term, q, [&](int n, double (&t)[1]) {
        const uint32_t key = k[n];
        const double e = (double)__uint_as_float(key) - mu;
        t[0] = key != 0u && ht[n] ? e * e : 0.0;
    });
    if (tid == 0) {
        const int n1 = count[1];
        const double sd = n1 ? sqrt(q[0] / (double)n1) : 0.0;
        n_data[r] = count[0];
        n_hit[r] = n1;
        sd_out[r] = sd;
        bw_out[r] = (sd != 0.0 ? sd : 1e-16) * bw_scale;
    }
}

// density [R][2][G]: S1, S2 of the row's grid points
__global__ __launch_bounds__(RK_THREADS) void reliability_kde_density_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ hit,
                                                                             int N, size_t N_cap, int G, const double* __restrict__ bw,
                                                                             double* __restrict__ density) {
    __shared__ double centre[2 * RL_TILE];  // the tile's centres within the workgroup's reach, in image order, a datum's own before its mirror
    __shared__ uint8_t of_hit[2 * RL_TILE]; // ... whether the datum's hit bit is set
    __shared__ int wave_count[RK_THREADS / 64];
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * RK_THREADS + tid;             // (beyond G in the last workgroup: walks along, writes nothing)
    const uint32_t* k = keys + (size_t)r * N_cap;
    const uint8_t* ht = hit + (size_t)r * N_cap;
    const double step = 2.2 / (double)(G - 1);
    const double h = 3.0 * bw[r];
    const double x = rk_grid(i, step);
    const int first = __builtin_amdgcn_readfirstlane(i);     // the wave's lowest grid index: lane 0's
    const double x_lo = rk_grid(first, step), x_hi = rk_grid(first + 63, step);
    const double g_lo = rk_grid(blockIdx.x * RK_THREADS, step), g_hi = rk_grid(blockIdx.x * RK_THREADS + RK_THREADS - 1, step);   // the workgroup's
    const unsigned long long below = (1ull << lane) - 1ull;
    double S1 = 0.0, S2 = 0.0;
    for (int n0 = 0; n0 < N; n0 += RL_TILE) {
        const int len = min(RL_TILE, N - n0);
        int kept = 0;                       // (the same in every thread)
        for (int j0 = 0; j0 < len; j0 += RK_THREADS) {       // an order-keeping compaction, RK_THREADS records at a time
            const int j = j0 + tid;
            double d = 0.0, m = 0.0;
            bool keep_d = false, keep_m = false, hb = false;
            if (j < len) {
                const uint32_t key = k[n0 + j];
                if (key != 0u) {
                    d = (double)__uint_as_float(key);
                    m = d < 0.5 ? -d : 2.0 - d;
                    hb = ht[n0 + j] != 0;
                    keep_d = !(g_lo - d >= h || g_hi - d <= -h);
                    keep_m = !(g_lo - m >= h || g_hi - m <= -h);
                }
            }
            const unsigned long long b_d = __ballot(keep_d), b_m = __ballot(keep_m);
            if (lane == 0) wave_count[wave] = __popcll(b_d) + __popcll(b_m);
            __syncthreads();
            int at = kept + __popcll(b_d & below) + __popcll(b_m & below);
#pragma unroll
            for (int w = 0; w < RK_THREADS / 64; ++w) {
                const int c = wave_count[w];
                if (w < wave) at += c;
                kept += c;
            }
            if (keep_d) {
                centre[at] = d;
                of_hit[at] = hb;
                ++at;
            }
            if (keep_m) {
                centre[at] = m;
                of_hit[at] = hb;
            }
            __syncthreads();                // (wave_count is rewritten by the next step; after the last one the list is complete)
        }
#pragma unroll 2
        for (int e = 0; e < kept; ++e) {    // image order; the centre is the same in every lane
            const double c = centre[e];
            if (x_lo - c >= h || x_hi - c <= -h) continue;               // (wave-uniform) out of every lane's reach
            const double u = (x - c) / h;
            const double t = 1.0 - u * u;
            if (t > 0.0) {
                const double term = t * t * t;
                S2 = S2 + term;
                if (of_hit[e]) S1 = S1 + term;
            }
        }
        __syncthreads();
    }
    if (i < G) {
        density[((size_t)r * 2 + 0) * G + i] = S1;
        density[((size_t)r * 2 + 1) * G + i] = S2;
    }
}

__global__ __launch_bounds__(RK_THREADS) void reliability_kde_integrate_kernel(int G, int order, const long long* __restrict__ n_data,
                                                                               const long long* __restrict__ n_hit, const double* __restrict__ bw,
                                                                               double* __restrict__ density, double* __restrict__ ece,
                                                                               int* __restrict__ degenerate) {
    __shared__ double ti[RK_ITILE];         // the integrand of the tile's set points, then of all its points
    __shared__ double tp[RK_ITILE];         // pp2
    __shared__ int wave_last[RK_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = n_data[r], n1 = n_hit[r];
    const double h = 3.0 * bw[r];
    const double step = 2.2 / (double)(G - 1);
    const double perc = n ? (double)n1 / (double)n : 0.0;
    const double den1 = h * (double)(2 * n1), den2 = h * (double)(2 * n);
    double* p1 = density + (size_t)r * 2 * G;
    double* p2 = p1 + G;
    int carry_at = -1;                      // the last set index below the tile, and its integrand (the same in every thread)
    double carry = 0.0;
    double a = 0.0, b = 0.0, x_prev = 0.0, i_prev = 0.0, p_prev = 0.0;   // (wave 0's)
    bool in_prev = false;
    for (int base = 0; base < G; base += RK_ITILE) {
        const int len = min(RK_ITILE, G - base);
        int last = -1, src[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 4 * tid + q, i = base + j;
            if (j < len) {
                const double x = rk_grid(i, step);
                const bool inside = x > 0.0 && x < 1.0;
                const double v1 = inside && n1 ? p1[i] * (35.0 / 32.0) / den1 * 2.0 : 0.0;
                const double v2 = inside && n ? p2[i] * (35.0 / 32.0) / den2 * 2.0 : 0.0;
                p1[i] = v1;
                p2[i] = v2;
                tp[j] = v2;
                if ((v1 > v2 ? v1 : v2) > 1e-6) {
                    double accu = perc * v1 / v2;
                    if (accu > 1.0) accu = 1.0;
                    double e = __builtin_fabs(x - accu);
                    if (order == 2) e = e * e;
                    ti[j] = e * v2;
                    last = i;
                }
            }
            src[q] = last;
        }
        int incl = last;                    // the last set index up to this thread's points, within the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl = max(incl, up);
        }
        if (lane == 63) wave_last[wave] = incl;
        int before = __shfl_up(incl, 1);    // ... below this thread's points
        if (lane == 0) before = -1;
        __syncthreads();
        int tile_last = carry_at;
#pragma unroll
        for (int w = 0; w < RK_THREADS / 64; ++w) {
            if (w < wave) before = max(before, wave_last[w]);
            tile_last = max(tile_last, wave_last[w]);
        }
        before = max(before, carry_at);
        double val[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int at = max(src[q], before);
            val[q] = at < 0 ? 0.0 : (at >= base ? ti[at - base] : carry);
        }
        if (tile_last >= base) carry = ti[tile_last - base];
        carry_at = tile_last;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * tid + q < len) ti[4 * tid + q] = val[q];
        __syncthreads();
        // (wave-uniform) a tile wholly below 0 or above 1 adds nothing, and its neighbour's first point has no partner in it
        if (tid < 64 && !(rk_grid(base + len - 1, step) < 0.0) && !(rk_grid(base, step) > 1.0)) {
#pragma unroll 8
            for (int j = 0; j < len; ++j) { // index order; a pair outside [0, 1] adds +0.0: the identity on a sum of terms >= 0
                const double x = rk_grid(base + j, step);
                const bool in = x >= 0.0 && x <= 1.0;
                const double ci = ti[j], cp = tp[j];
                const bool pair = in && in_prev;
                const double dx = x - x_prev;
                a = a + (pair ? dx * (ci + i_prev) / 2.0 : 0.0);
                b = b + (pair ? dx * (cp + p_prev) / 2.0 : 0.0);
                x_prev = x;
                i_prev = ci;
                p_prev = cp;
                in_prev = in;
            }
        }
        __syncthreads();                    // (wave_last, ti and tp are rewritten by the next tile)
    }
    if (tid == 0) {
        const bool deg = n == 0 || b == 0.0;
        ece[r] = deg ? 0.0 : a / b;
        degenerate[r] = deg;
    }
}

bool reliability_kde_takes(int R, int N, int G, double bw_scale) {
    return R >= 1 && R <= 2 * BMI_ENS_MAX_EXITS && N >= 1 && N < BMI_REL_MAX_IMAGES && G >= BMI_KDE_MIN_GRID && G <= BMI_KDE_MAX_GRID &&
           bw_scale >= 0x1p-100 && bw_scale <= 0x1p100;
}

int launch_reliability_kde(const uint32_t* keys, const uint8_t* hit, int R, int N, int N_cap, int G, int order, double bw_scale, double* ece_kde,
                           double* bw, double* sd, long long* n_data, long long* n_hit, int* degenerate, double* density, hipStream_t s) {
    if (!reliability_kde_takes(R, N, G, bw_scale)) return BMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(reliability_kde_moments_kernel, dim3((unsigned)R), dim3(RK_THREADS), 0, s, keys, hit, N, (size_t)N_cap, bw_scale, n_data, n_hit,
                       sd, bw);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(reliability_kde_density_kernel, dim3((unsigned)((G + RK_THREADS - 1) / RK_THREADS), (unsigned)R), dim3(RK_THREADS), 0, s, keys,
                       hit, N, (size_t)N_cap, G, (const double*)bw, density);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(reliability_kde_integrate_kernel, dim3((unsigned)R), dim3(RK_THREADS), 0, s, G, order, (const long long*)n_data,
                       (const long long*)n_hit, (const double*)bw, density, ece_kde, degenerate);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
