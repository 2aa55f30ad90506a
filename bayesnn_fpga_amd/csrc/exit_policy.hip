// Exit-policy sweep (bmi_exit_stat_record / bmi_exit_policy_sweep): what accuracy and cost a multi-exit network reaches when every image
// leaves at the first exit whose decision statistic exceeds a threshold, for many thresholds at once, from per-image records that stay on
// the device — the read-out of the reference's get_confidence_exiting_values (SA/train/results_analyzer.py:543-566) without a host copy of
// the predictions, decided in the arithmetic of the staged engine's own rule.  THE CONTRACT (restated in numpy as
// train.exit_policy.exit_stat_numpy / exit_policy_numpy):
//
// Record   S1 float64 [E][B][C], the sum of t_count samples' probabilities -> stat float64 [2][E][N_cap] at columns n0 .. n0 + B - 1:
//          stat[ens][e][n0 + b] = exit_rule_stat(S1, B, C, b, e, (double) t_count, margin, ens, ens ? weights + e * E : null) of exit_rule.h,
//          the number exit_rule_decide_kernel compares with the threshold (weights null: the equal mean).  A NaN is stored as it is.
// Sweep    stat [E][N_cap] (ONE plane of the record), thresholds float64 [G] in any order, repeats allowed.  Per threshold g and image
//          n < N:  e* = the lowest e in [first_exit, E-2] with stat[e][n] > thresholds[g] (strict, float64: false for a NaN on either side),
//          E-1 if there is none.  exit_of[g][n] = e*.  keys[e*][n] == 0 (the outcome record of a bad label or a non-finite row):
//          invalid[g] += 1 and the selected record is all zeros.  Otherwise count[g][e*] += 1, hits[g][e*] += (hit[e*][n] != 0) and the
//          selected records sel_*[g][n] are copies of the four records at (e*, n).
// Outputs  count, hits int64 [G][E] and invalid int64 [G] are OVERWRITTEN; exit_of and sel_* in columns 0 .. N-1 only.
// Integer LDS atomics only; the workgroups' partial counts go to the scratch and are added up as integers: the same bits on every run and
// for every cut of the images into record calls.
//
//   exit_stat_record_kernel   grid (ceil(B / 256), E, 2): one thread per (image, exit, ens) calls exit_rule_stat.
//   exit_policy_sweep_kernel  grid (chunks, ceil(G / PS_TILE_G)).  A workgroup takes a tile of PS_TILE_G thresholds and every chunks-th tile
//                             of PS_TILE_N images; it stages the tile's tested statistics (exits first_exit .. E-2) in LDS, thread
//                             (image i, threshold lane l) keeps its image's valid and hit bits of all E exits as two 32-bit masks in
//                             registers (no array indexed by e), walks thresholds l, l + 2, ... and per threshold the exits with an
//                             early break, and adds into the LDS histogram [PS_TILE_G][2 E + 1], written to the scratch at the end
//                             (uint32 [chunks][G][2 E + 1]: count, hits, invalid).
//   exit_policy_finish_kernel one thread per (g, slot) adds the chunks' partials in chunk order.
#include <cstdint>

#include "exit_rule.h"
#include "kernels.h"

#define PS_THREADS 256
#define PS_TILE_N 128       // images of a tile: threads 0..127 and 128..255 share them, one half of the thresholds each
#define PS_TILE_G 64        // thresholds whose histogram a workgroup keeps in LDS
#define PS_MAX_CHUNKS 128   // workgroups along the images: bounds the scratch

static_assert(PS_THREADS == 2 * PS_TILE_N, "two threshold lanes per image");

__global__ __launch_bounds__(PS_THREADS) void exit_stat_record_kernel(const double* __restrict__ S1, int B, int C, double t, int margin,
                                                                       const double* __restrict__ weights, size_t n0, size_t N_cap,
                                                                       double* __restrict__ stat) {
    const int b = blockIdx.x * PS_THREADS + threadIdx.x, e = blockIdx.y, ens = blockIdx.z, E = gridDim.y;
    if (b >= B) return;
    const double* w = (ens && weights) ? weights + (size_t)e * E : (const double*)nullptr;
    stat[((size_t)ens * E + e) * N_cap + n0 + (size_t)b] = exit_rule_stat(S1, B, C, b, e, t, margin, ens, w);
}

__global__ __launch_bounds__(PS_THREADS) void exit_policy_sweep_kernel(
    const double* __restrict__ stat, int E, int N, size_t N_cap, int first_exit, const double* __restrict__ thresholds, int G,
    const uint32_t* __restrict__ keys, const uint8_t* __restrict__ hit, const double* __restrict__ nll, const double* __restrict__ brier,
    uint8_t* __restrict__ exit_of, uint32_t* __restrict__ sel_keys, uint8_t* __restrict__ sel_hit, double* __restrict__ sel_nll,
    double* __restrict__ sel_brier, uint32_t* __restrict__ part) {
    __shared__ double sstat[(BMI_ENS_MAX_EXITS - 1) * PS_TILE_N];      // [tested exit][image of the tile]
    __shared__ double sthr[PS_TILE_G];
    __shared__ unsigned int hist[PS_TILE_G * (2 * BMI_ENS_MAX_EXITS + 1)];       // [threshold of the tile][count e | hits e | invalid]
    const int tid = threadIdx.x, img = tid & (PS_TILE_N - 1), lane_g = tid / PS_TILE_N;
    const int g0 = blockIdx.y * PS_TILE_G, glen = min(PS_TILE_G, G - g0);
    const int slots = 2 * E + 1, last = E - 1;
    const int tested = max(0, last - first_exit);            // exits first_exit .. E-2
    for (int i = tid; i < glen * slots; i += PS_THREADS) hist[i] = 0u;
    if (tid < glen) sthr[tid] = thresholds[g0 + tid];
    for (int n_base = blockIdx.x * PS_TILE_N; n_base < N; n_base += gridDim.x * PS_TILE_N) {
        __syncthreads();                    // (the tile before this one has been read; hist and sthr are set before the first use)
        for (int i = tid; i < tested * PS_TILE_N; i += PS_THREADS) {
            const int k = i / PS_TILE_N, j = i - k * PS_TILE_N, n = n_base + j;
            sstat[i] = n < N ? stat[(size_t)(first_exit + k) * N_cap + n] : 0.0;
        }
        __syncthreads();
        const int n = n_base + img;
        if (n < N) {
            uint32_t valid = 0u, hits = 0u;     // bit e: the outcome record at (e, n) is valid / a hit
            for (int e = 0; e < E; ++e) {
                const size_t at = (size_t)e * N_cap + n;
                valid |= (uint32_t)(keys[at] != 0u) << e;
                hits |= (uint32_t)(hit[at] != 0) << e;
            }
            for (int gl = lane_g; gl < glen; gl += 2) {
                const double thr = sthr[gl];
                int k = 0;
                while (k < tested && !(sstat[k * PS_TILE_N + img] > thr)) ++k;
                const int e = k < tested ? first_exit + k : last;
                const bool ok = (valid >> e) & 1u;
                unsigned int* h = hist + gl * slots;
                if (ok) {
                    atomicAdd(h + e, 1u);
                    if ((hits >> e) & 1u) atomicAdd(h + E + e, 1u);
                } else {
                    atomicAdd(h + 2 * E, 1u);
                }
                const size_t to = (size_t)(g0 + gl) * N_cap + n;
                if (exit_of) exit_of[to] = (uint8_t)e;
                if (sel_keys) {
                    const size_t from = (size_t)e * N_cap + n;
                    sel_keys[to] = ok ? keys[from] : 0u;
                    sel_hit[to] = ok ? hit[from] : (uint8_t)0;
                    sel_nll[to] = ok ? nll[from] : 0.0;
                    sel_brier[to] = ok ? brier[from] : 0.0;
                }
            }
        }
    }
    __syncthreads();
    uint32_t* p = part + ((size_t)blockIdx.x * G + g0) * slots;
    for (int i = tid; i < glen * slots; i += PS_THREADS) p[i] = hist[i];
}

__global__ __launch_bounds__(PS_THREADS) void exit_policy_finish_kernel(const uint32_t* __restrict__ part, int chunks, int E, int G,
                                                                         long long* __restrict__ count, long long* __restrict__ hits,
                                                                         long long* __restrict__ invalid) {
    const int slots = 2 * E + 1;
    const int i = blockIdx.x * PS_THREADS + threadIdx.x;
    if (i >= G * slots) return;
    long long sum = 0;
    for (int c = 0; c < chunks; ++c) sum += (long long)part[(size_t)c * G * slots + i];
    const int g = i / slots, s = i - g * slots;
    if (s < E) count[(size_t)g * E + s] = sum;
    else if (s < 2 * E) hits[(size_t)g * E + s - E] = sum;
    else invalid[g] = sum;
}

bool exit_stat_record_takes(int E, int B, int C) {
    return E >= 1 && B >= 1 && C >= 1 && E <= BMI_ENS_MAX_EXITS && C <= BMI_ENS_MAX_CLASSES;
}

bool exit_policy_takes(int E, int N, int G, bool select) {
    return E >= 1 && N >= 1 && G >= 1 && E <= BMI_ENS_MAX_EXITS && G <= BMI_POLICY_MAX_THRESHOLDS && N < BMI_REL_MAX_IMAGES &&
           (!select || G <= BMI_POLICY_MAX_RECORD_ROWS);
}

static int policy_chunks(int N) { return min((N + PS_TILE_N - 1) / PS_TILE_N, PS_MAX_CHUNKS); }

size_t exit_policy_scratch_bytes(int E, int N, int G) {
    if (!exit_policy_takes(E, N, G, false)) return 0;
    return (size_t)policy_chunks(N) * (size_t)G * (size_t)(2 * E + 1) * sizeof(uint32_t);
}

int launch_exit_stat_record(const double* S1, int E, int B, int C, int t_count, int margin, const double* weights, int n0, int N_cap, double* stat,
                            hipStream_t s) {
    if (!exit_stat_record_takes(E, B, C)) return BMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(exit_stat_record_kernel, dim3((unsigned)((B + PS_THREADS - 1) / PS_THREADS), (unsigned)E, 2u), dim3(PS_THREADS), 0, s, S1, B,
                       C, (double)t_count, margin, weights, (size_t)n0, (size_t)N_cap, stat);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_exit_policy_sweep(const double* stat, int E, int N, int N_cap, int first_exit, const double* thresholds, int G, const uint32_t* keys,
                             const uint8_t* hit, const double* nll, const double* brier, long long* count, long long* hits, long long* invalid,
                             uint8_t* exit_of, uint32_t* sel_keys, uint8_t* sel_hit, double* sel_nll, double* sel_brier, void* scratch,
                             hipStream_t s) {
    if (!exit_policy_takes(E, N, G, sel_keys != nullptr)) return BMI_ERR_UNSUPPORTED;
    const int chunks = policy_chunks(N), gtiles = (G + PS_TILE_G - 1) / PS_TILE_G, cells = G * (2 * E + 1);
    hipLaunchKernelGGL(exit_policy_sweep_kernel, dim3((unsigned)chunks, (unsigned)gtiles), dim3(PS_THREADS), 0, s, stat, E, N, (size_t)N_cap,
                       first_exit, thresholds, G, keys, hit, nll, brier, exit_of, sel_keys, sel_hit, sel_nll, sel_brier, (uint32_t*)scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(exit_policy_finish_kernel, dim3((unsigned)((cells + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, s,
                       (const uint32_t*)scratch, chunks, E, G, count, hits, invalid);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
