// Rank quality of the per-image uncertainty scores (bmi_score_record / bmi_rank_quality): per row the stable ascending order of the images by
// a 32-bit score key, the number of positive images (wrong predictions, or noise images) in every prefix of that order — the risk-coverage
// curve of selective prediction — and the Mann-Whitney count behind the AUROC, without a host copy of the scores and without a sort.  THE
// ARITHMETIC CONTRACT (restated in numpy as train.ranking.score_keys_numpy / rank_quality_numpy):
//
// Keys     score float64 [R][B] -> ukeys uint32 [R][N_cap] at columns n0 .. n0 + B - 1.  f = (float) score (round to nearest).  Where
//          valid_keys is given and valid_keys[r][n] == 0: ukey = INVALID = 0xFFFFFFFF, not counted.  Otherwise f NaN, infinite or below zero:
//          ukey = INVALID and *counter += 1.  Otherwise b = the bit pattern of f + 0.0f (-0.0 becomes +0.0; b <= 0x7F7FFFFF) and
//          ukey = b (direction +1, an uncertainty) or 0x7F7FFFFF - b (direction -1, a confidence): ascending unsigned key order is "most
//          certain first".
// Order    per row r over columns 0 .. N-1: the valid images (ukey != INVALID, m of them) in the STABLE ascending order, by ukey, ties by
//          image index (np.argsort(kind="stable")).  (A ukey above 0x7F7FFFFF, which no record call writes, is read as INVALID.)
// Outputs  every one OVERWRITTEN in columns 0 .. N-1, columns >= N untouched:
//          rank int32 [R][N_cap]         the image's position 0 .. m-1, -1 for an invalid image
//          sorted_keys uint32 [R][N_cap] position k: the ukey of the image ranked k; positions m .. N-1: 0xFFFFFFFF
//          curve int32 [R][N_cap]        position k: the positive images at positions 0 .. k; positions m .. N-1: n_pos
//          counts int64 [R][3]           m, n_pos (valid and positive), U2 = the sum over the pairs (positive i, negative j), both valid, of
//                                        2 [ukey_j < ukey_i] + [ukey_j == ukey_i]: AUROC = U2 / (2 n_pos n_neg), ties counted half
//          aurc_sum float64 [R]          ((0.0 + curve[0] / 1) + curve[1] / 2) + ... + curve[m-1] / m: ascending k from 0.0, each quotient
//                                        the correctly rounded float64 division of the two integers converted exactly, no fused
//                                        multiply-add; 0.0 when m = 0 (AURC = aurc_sum / m is formed on the host)
// No floating-point atomics; integer atomics only (the record call's counter, LDS counts in the rank call): the same bits on every run
// and for every cut of the images into record calls.  No NaN reaches an output.
//
// Ranking by counting.  For image i of key u, over every j of the row:  less = #{u_j < u},  eq_bef = #{j < i, u_j == u},  the same two
// among the positives (less_pos, eq_pos_bef), and eq_neg = #{u_j == u, j negative}.  Then rank = less + eq_bef, the image's curve value is
// less_pos + eq_pos_bef + its own bit, and a positive image adds 2 (less - less_pos) + eq_neg to U2.  Each valid image writes its key and
// its curve value at its rank — a permutation: no two writers share a cell.
//
//   score_record_kernel   grid (ceil(B / 256), R), one thread per (row, image); the counter receives one integer atomicAdd per wave that
//                         saw a bad score (ballot + popcount).
//   rank_count_kernel     the hot path, O(N^2) per row: grid (ceil(N / RANK_TILE_I), R).  A thread keeps RK_IPT images' keys in
//                         registers; the row's keys stream through LDS in tiles of RANK_TILE_J as two packed words per image j:
//                         p = (ukey << 1) | positive (the key's free low bit: ukey <= 0x7F7FFFFF) and q = p for a positive image, all ones
//                         for a negative one; an invalid image or a column >= N is all ones in both, above every a + 2 below.  With
//                         a = ukey_i << 1:  #{p < a} = less,  #{p < a + 1} = less + eq_neg,  #{q < a} = less_pos,  and over the tiles wholly
//                         below the workgroup's images also #{p < a + 2} and #{q < a + 2} (less + eq, among all and among the positives).
//                         Every lane reads the same LDS words in the same step (a broadcast: no bank conflict), four images j per
//                         ds_read_b128; per pair three to five compare-and-add steps on registers.  The one tile that holds the
//                         workgroup's own images compares the indices as well; the tiles above it skip the two equal counts.  The
//                         workgroup's m, n_pos and U2 partial go to the scratch (int64 [R][tiles][3]).
//   rank_finish_kernel    one workgroup per row: the partials added up (integers, order-free), the tails m .. N-1 of sorted_keys and curve
//                         filled, and aurc_sum added in position order by record_common.h's ordered_sum<1> over the quotients.
#include <cstdint>

#include "record_common.h"

#pragma clang fp contract(off)

#define RK_THREADS RECORD_THREADS
#define RK_IPT (BMI_RANK_TILE_I / RK_THREADS)
#define RK_INVALID 0xFFFFFFFFu
#define RK_MAX_KEY 0x7F7FFFFFu

static_assert(BMI_RANK_TILE_I % RK_THREADS == 0 && BMI_RANK_TILE_J % BMI_RANK_TILE_I == 0 && BMI_RANK_TILE_J % (4 * RK_THREADS) == 0,
              "an image tile lies inside one key tile; the staging and the b128 reads take whole steps");

__global__ __launch_bounds__(RK_THREADS) void score_record_kernel(const double* __restrict__ score, int B, int direction,
                                                                   const uint32_t* __restrict__ valid_keys, size_t n0, size_t N_cap,
                                                                   uint32_t* __restrict__ ukeys, int* counter) {
    const int b = blockIdx.x * RK_THREADS + threadIdx.x, r = blockIdx.y;
    bool bad = false;
    if (b < B) {
        const size_t at = (size_t)r * N_cap + n0 + (size_t)b;
        const float f = (float)score[(size_t)r * B + b];
        uint32_t key = RK_INVALID;
        if (valid_keys && valid_keys[at] == 0u) {
            // (silenced by the reliability record: counted there)
        } else if (!__builtin_isfinite(f) || f < 0.0f) {
            bad = true;
        } else {
            const uint32_t bits = __float_as_uint(f) & 0x7FFFFFFFu;      // f + 0.0f: only -0.0 changes, to +0.0
            key = direction > 0 ? bits : RK_MAX_KEY - bits;
        }
        ukeys[at] = key;
    }
    const unsigned long long bad_lanes = __ballot(bad);
    if (counter && bad_lanes && (threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(bad_lanes));
}

// MODE 0: every image j of the tile lies below every image of the workgroup; 1: the tile holds the workgroup's images; 2: it lies above them
template <int MODE>
__device__ __forceinline__ void rank_count_tile(const uint32_t* sp, const uint32_t* sq, const uint32_t (&a)[RK_IPT], const int (&local)[RK_IPT],
                                                int (&lt)[RK_IPT], int (&le_neg)[RK_IPT], int (&lt_pos)[RK_IPT], int (&eq_bef)[RK_IPT],
                                                int (&eq_pos_bef)[RK_IPT]) {
#pragma unroll 2
    for (int j = 0; j < BMI_RANK_TILE_J; j += 4) {
        const uint4 pv = *reinterpret_cast<const uint4*>(sp + j);       // the same address in every lane: a broadcast
        const uint4 qv = *reinterpret_cast<const uint4*>(sq + j);
        const uint32_t p[4] = {pv.x, pv.y, pv.z, pv.w}, q[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int k = 0; k < RK_IPT; ++k) {
                lt[k] += p[s] < a[k];
                le_neg[k] += p[s] < a[k] + 1u;
                lt_pos[k] += q[s] < a[k];
                if (MODE == 0) {            // (here the two hold less + eq; the caller takes the differences)
                    eq_bef[k] += p[s] < a[k] + 2u;
                    eq_pos_bef[k] += q[s] < a[k] + 2u;
                } else if (MODE == 1) {
                    const bool before = j + s < local[k];
                    eq_bef[k] += before && (p[s] | 1u) == (a[k] | 1u);
                    eq_pos_bef[k] += before && q[s] == (a[k] | 1u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(const uint32_t* __restrict__ ukeys, const uint8_t* __restrict__ positive, int N,
                                                                 size_t N_cap, int* __restrict__ rank, uint32_t* __restrict__ sorted_keys,
                                                                 int* __restrict__ curve, long long* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) uint32_t sp[BMI_RANK_TILE_J];
    __shared__ __attribute__((aligned(16))) uint32_t sq[BMI_RANK_TILE_J];
    __shared__ unsigned long long total[3];                  // m, n_pos, U2 of the workgroup's images
    const int tid = threadIdx.x, r = blockIdx.y;
    const int i0 = blockIdx.x * BMI_RANK_TILE_I;
    const uint32_t* keys = ukeys + (size_t)r * N_cap;
    const uint8_t* pos = positive + (size_t)r * N_cap;
    uint32_t u[RK_IPT], a[RK_IPT];
    bool is_pos[RK_IPT];
    int local[RK_IPT], lt[RK_IPT], le_neg[RK_IPT], lt_pos[RK_IPT], eq_bef[RK_IPT], eq_pos_bef[RK_IPT];
    const int own = i0 / BMI_RANK_TILE_J * BMI_RANK_TILE_J;  // the first image of the key tile that holds the workgroup's
    if (tid < 3) total[tid] = 0ull;
#pragma unroll
    for (int k = 0; k < RK_IPT; ++k) {
        const int i = i0 + k * RK_THREADS + tid;
        u[k] = i < N ? keys[i] : RK_INVALID;
        if (u[k] > RK_MAX_KEY) u[k] = RK_INVALID;            // (no record call writes such a key: read as INVALID, which keeps every a + 2 from wrapping)
        is_pos[k] = i < N && pos[i] != 0;
        a[k] = u[k] << 1;                   // (an invalid image: its counts are formed and dropped)
        local[k] = i - own;
        lt[k] = le_neg[k] = lt_pos[k] = eq_bef[k] = eq_pos_bef[k] = 0;
    }
    for (int j0 = 0; j0 < N; j0 += BMI_RANK_TILE_J) {
        __syncthreads();                    // (the tile before this one has been read by every wave; `total` is zero before its first use)
#pragma unroll
        for (int s = 0; s < BMI_RANK_TILE_J / RK_THREADS; ++s) {
            const int jj = s * RK_THREADS + tid, j = j0 + jj;
            const uint32_t key = j < N ? keys[j] : RK_INVALID;
            const bool bit = j < N && pos[j] != 0;
            const uint32_t p = key > RK_MAX_KEY ? RK_INVALID : (key << 1) | (uint32_t)bit;
            sp[jj] = p;
            sq[jj] = p & 1u ? p : RK_INVALID;
        }
        __syncthreads();
        if (j0 < own) {                     // (uniform over the workgroup)
            rank_count_tile<0>(sp, sq, a, local, lt, le_neg, lt_pos, eq_bef, eq_pos_bef);
            if (j0 + BMI_RANK_TILE_J == own) {
#pragma unroll
                for (int k = 0; k < RK_IPT; ++k) {           // the tiles below are done: less + eq becomes eq
                    eq_bef[k] -= lt[k];
                    eq_pos_bef[k] -= lt_pos[k];
                }
            }
        } else if (j0 == own) {
            rank_count_tile<1>(sp, sq, a, local, lt, le_neg, lt_pos, eq_bef, eq_pos_bef);
        } else {
            rank_count_tile<2>(sp, sq, a, local, lt, le_neg, lt_pos, eq_bef, eq_pos_bef);
        }
    }
    int m = 0, n_pos = 0;
    long long u2 = 0;
#pragma unroll
    for (int k = 0; k < RK_IPT; ++k) {
        const int i = i0 + k * RK_THREADS + tid;
        if (i >= N) continue;
        const size_t row = (size_t)r * N_cap;
        if (u[k] == RK_INVALID) {
            rank[row + i] = -1;
            continue;
        }
        const int at = lt[k] + eq_bef[k];                    // < m <= N: a permutation of 0 .. m-1 over the row's valid images
        rank[row + i] = at;
        sorted_keys[row + at] = u[k];
        curve[row + at] = lt_pos[k] + eq_pos_bef[k] + (int)is_pos[k];
        ++m;
        if (is_pos[k]) {
            ++n_pos;
            u2 += 2ll * (lt[k] - lt_pos[k]) + (le_neg[k] - lt[k]);
        }
    }
    if (m) atomicAdd(&total[0], (unsigned long long)m);      // (LDS, integers: order-free)
    if (n_pos) {
        atomicAdd(&total[1], (unsigned long long)n_pos);
        atomicAdd(&total[2], (unsigned long long)u2);
    }
    __syncthreads();
    if (tid < 3) partial[((size_t)r * gridDim.x + blockIdx.x) * 3 + tid] = (long long)total[tid];
}

__global__ __launch_bounds__(RK_THREADS) void rank_finish_kernel(int N, size_t N_cap, int tiles, const long long* __restrict__ partial,
                                                                  uint32_t* __restrict__ sorted_keys, int* __restrict__ curve,
                                                                  long long* __restrict__ counts, double* __restrict__ aurc_sum) {
    __shared__ double term[1][RL_TILE];
    __shared__ unsigned long long total[3];
    const int r = blockIdx.x, tid = threadIdx.x;
    uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    int* cv = curve + (size_t)r * N_cap;
    if (tid < 3) total[tid] = 0ull;
    __syncthreads();
    for (int t = tid; t < tiles; t += RK_THREADS)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long v = partial[((size_t)r * tiles + t) * 3 + c];
            if (v) atomicAdd(&total[c], (unsigned long long)v);
        }
    __syncthreads();
    const int m = (int)total[0], n_pos = (int)total[1];
    for (int k = m + tid; k < N; k += RK_THREADS) {
        sk[k] = RK_INVALID;
        cv[k] = n_pos;
    }
    double acc[1] = {0.0};                  // position order
    ordered_sum<1>(m, term, acc, [&](int k, double (&t)[1]) { t[0] = (double)cv[k] / (double)(k + 1); });
    if (tid < 3) counts[(size_t)r * 3 + tid] = (long long)total[tid];
    if (tid == 0) aurc_sum[r] = acc[0];
}

bool score_record_takes(int R, int B) { return R >= 1 && R <= BMI_RANK_MAX_ROWS && B >= 1 && B <= BMI_RANK_MAX_IMAGES; }

bool rank_quality_takes(int R, int N) { return R >= 1 && R <= BMI_RANK_MAX_ROWS && N >= 1 && N <= BMI_RANK_MAX_IMAGES; }

size_t rank_scratch_bytes(int R, int N) {
    if (!rank_quality_takes(R, N)) return 0;
    return (size_t)R * (size_t)((N + BMI_RANK_TILE_I - 1) / BMI_RANK_TILE_I) * 3 * sizeof(long long);
}

int launch_score_record(const double* score, int R, int B, int direction, const uint32_t* valid_keys, int n0, int N_cap, uint32_t* ukeys,
                        int* counter, hipStream_t s) {
    if (!score_record_takes(R, B)) return BMI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(score_record_kernel, dim3((unsigned)((B + RK_THREADS - 1) / RK_THREADS), (unsigned)R), dim3(RK_THREADS), 0, s, score, B,
                       direction, valid_keys, (size_t)n0, (size_t)N_cap, ukeys, counter);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_rank_quality(const uint32_t* ukeys, const uint8_t* positive, int R, int N, int N_cap, int* rank, uint32_t* sorted_keys, int* curve,
                        long long* counts, double* aurc_sum, void* scratch, hipStream_t s) {
    if (!rank_quality_takes(R, N)) return BMI_ERR_UNSUPPORTED;
    const int tiles = (N + BMI_RANK_TILE_I - 1) / BMI_RANK_TILE_I;
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)tiles, (unsigned)R), dim3(RK_THREADS), 0, s, ukeys, positive, N, (size_t)N_cap, rank,
                       sorted_keys, curve, (long long*)scratch);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)R), dim3(RK_THREADS), 0, s, N, (size_t)N_cap, tiles, (const long long*)scratch,
                       sorted_keys, curve, counts, aurc_sum);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
