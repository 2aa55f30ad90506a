// Conformal prediction sets (bmi_conformal_scores / bmi_conformal_quantile / bmi_conformal_sets): split conformal prediction — LAC (Sadinle et
// al. 2019), APS (Romano et al. 2020, the deterministic form) and RAPS (Angelopoulos et al. 2021) — per exit and per exit ensemble, from the
// classwise records (reliability_classwise.hip: the float32 confidence of EVERY class of every image, on the device), without a host copy of
// them.  THE ARITHMETIC CONTRACT (restated in numpy, loop by loop, as train.conformal.conformal_numpy) — integers only:
//
// Input    pkeys uint32 [R][C][N_cap], the image index fastest, and labels_rec int32 [N_cap]: bmi_classwise_record's (a key is at most
//          0x3F800000, the bits of 1.0f, or INVALID = 0xFFFFFFFF); rows r = kind * E + e.  Columns 0 .. N-1 are read.
// Valid    a (row, image) none of whose C keys is INVALID and whose label record is in [0, C).
// Per class of a valid pair, conf_c the float32 behind key_c:
//     u_c      = (uint64) ((double) conf_c * 2^30), truncating.  conf_c is zero or a normal float32 at most 1, so the product by 2^30 is exact
//                in float32 as well, which is how the kernel forms it; u_c <= 2^30
//     order    class j PRECEDES class c when key_j > key_c, or key_j == key_c and j < c: total and stable, ties by class index
//     rank_c   = the classes that precede c;   above_c = the sum of u_j over them (below 2^37)
//     score_c  (uint64) = LAC: 2^30 - u_c;   APS: above_c + u_c;   RAPS: above_c + u_c + lam_fix * max(0, rank_c + 1 - k_reg), lam_fix <= 2^30
//     skey_c   = (uint32) min(score_c, 0xFFFFFFFE): saturating.  An invalid pair has the one key INVALID, which sorts last
// Scores   score_keys uint32 [R][N_cap]: the skey of the LABEL's class; INVALID for an invalid pair; columns >= N are not touched.
// Quantile per row n = the keys that are not INVALID, per level k = (int64) ceil((double) (n + 1) * coverage_l) (one rounded product, one ceil);
//          qhat = 0xFFFFFFFE when n == 0 or k > n, else the order statistic of rank k - 1 of the row's N keys in unsigned order
//          (record_common.h's radix_select_u32: exact under duplicates, no sort).
// Sets     class c is in the set of (r, l, n) iff skey_c <= qhat[r][l].  set_size uint8 [R][L][N_cap] (255: an invalid pair), members uint32
//          [R][L][ceil(C / 32)][N_cap] (bit c % 32 of word c / 32; 0 beyond C and for an invalid pair; may be null), and over the valid
//          images int64 valid [R], covered / size_sum [R][L], size_hist / cov_hist [R][L][C + 1], class_n [R][C], class_cov [R][L][C].
// Integer atomics only; every output is OVERWRITTEN; the same bits on every run, however the N images were cut into record calls.
//
//   conformal_kernel<NI, SETS>   the shared body of the scores (SETS = false) and the sets.  The records are image-fastest, so ONE IMAGE TO A
//       LANE: a workgroup of four waves takes a tile of 64 consecutive images of one row.  Thread (wave w, lane l) owns image l and the
//       classes c = w + 4 i, i < NI (NI = 8, 16, 32 for C <= 32, 64, 128): it loads their keys — a coalesced row load per class —, keeps them
//       in registers and stages them in LDS (C x 64 keys, 32 KB at C = 128; the column of an image is conflict-free).  ONE walk over j = 0 ..
//       C-1 reads each LDS key of the lane's image once and updates the rank and the `above` sum of all NI owned classes in registers: C
//       reads and C NI compare-adds per thread.  LAC needs neither and walks for the validity alone.  Scores: the wave that owns the label's
//       class stores its key.  Sets: per level the owned scores are compared with qhat into membership words whose bits the four waves
//       hold interleaved (class c = bit w + 4 (i % 8) of word i / 8); they are joined through the LDS the keys have left, thread (w, l)
//       then finishes the levels l' = w, w + 4 of its image: the words, the popcount, the label's bit.  The tile's tables are int32 in LDS
//       (integer atomics) and added to the int64 outputs once per tile (integer global atomics: order-free), which conformal_clear_kernel
//       zeroed.  Tails by predication: a column >= N is never read and is INVALID in LDS, a class >= C owns no bit.
//   conformal_quantile_kernel    one workgroup per row: the count of valid keys, then one radix select per level.
// Matrix instructions have no place here: the work is compares and integer adds.
#include <cstdint>

#include "record_common.h"

#define CF_THREADS RECORD_THREADS
#define CF_TILE 64                          // images of a tile: one to a lane
#define CF_INVALID 0xFFFFFFFFu
#define CF_MAX_KEY 0xFFFFFFFEu
#define CF_ONE 0x3F800000u                  // the key of confidence 1
#define CF_UNIT 1073741824u                 // 2^30

struct ConformalLevels { double v[BMI_CONFORMAL_MAX_LEVELS]; };

// a row's tables in one index space, in this order: size_hist, cov_hist [L][C + 1], class_cov [L][C], class_n [C], covered, size_sum [L], valid
__host__ __device__ constexpr int table_len(int L, int C) { return 2 * L * (C + 1) + L * C + C + 2 * L + 1; }
#define CF_TAB_MAX table_len(BMI_CONFORMAL_MAX_LEVELS, BMI_ENS_MAX_CLASSES)

// entry i of row r's tables
__device__ __forceinline__ long long* table_slot(const ConformalTables& t, int L, int C, int r, int i) {
    const int h = L * (C + 1), cc = L * C;
    if (i < h) return t.size_hist + (size_t)r * h + i;
    i -= h;
    if (i < h) return t.cov_hist + (size_t)r * h + i;
    i -= h;
    if (i < cc) return t.class_cov + (size_t)r * cc + i;
    i -= cc;
    if (i < C) return t.class_n + (size_t)r * C + i;
    i -= C;
    if (i < L) return t.covered + (size_t)r * L + i;
    i -= L;
    if (i < L) return t.size_sum + (size_t)r * L + i;
    return t.valid + r;
}

// u = (uint64) ((double) conf * 2^30) of a record key: exact in float32 (a power-of-two scale of zero or a normal number, at most 2^30)
__device__ __forceinline__ uint32_t conf_fix30(uint32_t key) { return key <= CF_ONE ? (uint32_t)(__uint_as_float(key) * 1073741824.0f) : 0u; }

// grid (ceil(table_len / CF_THREADS), R)
__global__ __launch_bounds__(CF_THREADS) void conformal_clear_kernel(ConformalTables t, int L, int C) {
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < table_len(L, C)) *table_slot(t, L, C, blockIdx.y, i) = 0ll;
}

// grid (ceil(N / CF_TILE), R)
template <int NI, bool SETS>
__global__ __launch_bounds__(CF_THREADS) void conformal_kernel(const uint32_t* __restrict__ pkeys, const int* __restrict__ labels_rec, int C, int N,
                                                               size_t N_cap, int method, int k_reg, uint32_t lam_fix,
                                                               uint32_t* __restrict__ score_keys, const uint32_t* __restrict__ qhat, int L,
                                                               uint8_t* __restrict__ set_size, uint32_t* __restrict__ members, ConformalTables t) {
    __shared__ uint32_t stage[4 * NI * CF_TILE];        // the tile's keys [class][lane]; then the membership words [level][word][wave][lane]
    __shared__ int tab[SETS ? CF_TAB_MAX : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = blockIdx.y;
    const size_t n = (size_t)blockIdx.x * CF_TILE + lane;
    const bool present = n < (size_t)N;
    const int len = table_len(L, C);
    if (SETS)
        for (int i = tid; i < len; i += CF_THREADS) tab[i] = 0;

    const uint32_t* row = pkeys + (size_t)r * C * N_cap + n;
    uint32_t key[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = w + 4 * i;
        key[i] = 0u;
        if (c < C) {                        // (wave-uniform)
            key[i] = present ? row[(size_t)c * N_cap] : CF_INVALID;
            stage[c * CF_TILE + lane] = key[i];
        }
    }
    __syncthreads();

    uint32_t rank[NI];
    unsigned long long above[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        rank[i] = 0u;
        above[i] = 0ull;
    }
    bool invalid = false;
    if (method == BMI_CONFORMAL_LAC) {
        for (int j = 0; j < C; ++j) invalid |= stage[j * CF_TILE + lane] == CF_INVALID;
    } else {
        for (int j = 0; j < C; ++j) {
            const uint32_t kj = stage[j * CF_TILE + lane];
            const unsigned long long uj = conf_fix30(kj);
            invalid |= kj == CF_INVALID;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const bool precedes = kj > key[i] || (kj == key[i] && j < w + 4 * i);
                rank[i] += precedes ? 1u : 0u;
                above[i] += precedes ? uj : 0ull;
            }
        }
    }
    const int y = present ? labels_rec[n] : -1;
    const bool valid = present && !invalid && (unsigned)y < (unsigned)C;

    uint32_t skey[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const unsigned long long u = conf_fix30(key[i]);
        unsigned long long score = CF_UNIT - u;
        if (method != BMI_CONFORMAL_LAC) {
            const int over = (int)rank[i] + 1 - k_reg;
            score = above[i] + u;
            if (method == BMI_CONFORMAL_RAPS && over > 0) score += (unsigned long long)lam_fix * (unsigned long long)over;
        }
        skey[i] = score > CF_MAX_KEY ? CF_MAX_KEY : (uint32_t)score;
    }

    if (!SETS) {                            // the label's key, from the wave that owns its class; wave 0 marks an invalid pair
        uint32_t mine = CF_INVALID;
        bool own = !valid && w == 0;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (valid && w + 4 * i == y) {
                mine = skey[i];
                own = true;
            }
        if (present && own) score_keys[(size_t)r * N_cap + n] = mine;
        return;
    }

    const int W = (C + 31) >> 5;
    __syncthreads();                        // every walk is over: the keys' LDS is free
    for (int l = 0; l < L; ++l) {
        const uint32_t q = qhat[r * L + l];
        uint32_t part[NI / 8];
#pragma unroll
        for (int k = 0; k < NI / 8; ++k) part[k] = 0u;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (w + 4 * i < C && skey[i] <= q) part[i >> 3] |= 1u << (w + 4 * (i & 7));
#pragma unroll
        for (int k = 0; k < NI / 8; ++k)
            if (k < W) stage[((l * W + k) * 4 + w) * CF_TILE + lane] = part[k];
    }
    __syncthreads();
    if (present) {
        for (int l = w; l < L; l += 4) {    // thread (w, lane) finishes the levels w, w + 4 of its image
            int size = 0;
            bool hit = false;
            for (int k = 0; k < W; ++k) {
                const uint32_t* p = stage + (l * W + k) * 4 * CF_TILE + lane;
                const uint32_t m = valid ? (p[0] | p[CF_TILE] | p[2 * CF_TILE] | p[3 * CF_TILE]) : 0u;
                size += __popc(m);
                if (valid && k == (y >> 5)) hit = (m >> (y & 31)) & 1u;
                if (members) members[(((size_t)r * L + l) * W + k) * N_cap + n] = m;
            }
            set_size[((size_t)r * L + l) * N_cap + n] = valid ? (uint8_t)size : (uint8_t)255;
            if (valid) {
                const int h = L * (C + 1);
                atomicAdd(&tab[l * (C + 1) + size], 1);
                atomicAdd(&tab[2 * h + L * C + C + L + l], size);
                if (hit) {
                    atomicAdd(&tab[h + l * (C + 1) + size], 1);
                    atomicAdd(&tab[2 * h + l * C + y], 1);
                    atomicAdd(&tab[2 * h + L * C + C + l], 1);
                }
            }
        }
        if (w == 0 && valid) {
            atomicAdd(&tab[2 * L * (C + 1) + L * C + y], 1);
            atomicAdd(&tab[len - 1], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < len; i += CF_THREADS) {
        const int v = tab[i];
        if (v) atomicAdd((unsigned long long*)table_slot(t, L, C, r, i), (unsigned long long)v);
    }
}

// grid (R)
__global__ __launch_bounds__(CF_THREADS) void conformal_quantile_kernel(const uint32_t* __restrict__ score_keys, int N, size_t N_cap,
                                                                        ConformalLevels coverage, int L, uint32_t* __restrict__ qhat,
                                                                        long long* __restrict__ n_valid) {
#pragma clang fp contract(off)
    __shared__ int hist[256];
    __shared__ int chosen[2];
    __shared__ int count;
    const int tid = threadIdx.x, r = blockIdx.x;
    const uint32_t* line = score_keys + (size_t)r * N_cap;
    if (tid == 0) count = 0;
    __syncthreads();
    int seen = 0;
    for (int i = tid; i < N; i += CF_THREADS) seen += line[i] != CF_INVALID ? 1 : 0;
    if (seen) atomicAdd(&count, seen);
    __syncthreads();
    const int n = count;
    for (int l = 0; l < L; ++l) {
        const long long k = (long long)ceil((double)(n + 1) * coverage.v[l]);
        uint32_t q = CF_MAX_KEY;
        if (n > 0 && k <= (long long)n) q = radix_select_u32(line, N, (int)(k - 1), hist, chosen);      // (workgroup-uniform)
        if (tid == 0) qhat[r * L + l] = q;
    }
    if (tid == 0) n_valid[r] = (long long)n;
}

bool conformal_takes(int R, int C, int N) {
    return R >= 1 && C >= 1 && N >= 1 && R <= 2 * BMI_ENS_MAX_EXITS && C <= BMI_ENS_MAX_CLASSES && N < BMI_REL_MAX_IMAGES;
}

template <bool SETS>
static void launch_body(const uint32_t* pkeys, const int* labels_rec, int R, int C, int N, int N_cap, int method, int k_reg, uint32_t lam_fix,
                        uint32_t* score_keys, const uint32_t* qhat, int L, uint8_t* set_size, uint32_t* members, ConformalTables t, hipStream_t s) {
    const dim3 grid((unsigned)((N + CF_TILE - 1) / CF_TILE), (unsigned)R);
    auto kernel = C <= 32 ? conformal_kernel<8, SETS> : C <= 64 ? conformal_kernel<16, SETS> : conformal_kernel<32, SETS>;
    hipLaunchKernelGGL(kernel, grid, dim3(CF_THREADS), 0, s, pkeys, labels_rec, C, N, (size_t)N_cap, method, k_reg, lam_fix, score_keys, qhat, L,
                       set_size, members, t);
}

int launch_conformal_scores(const uint32_t* pkeys, const int* labels_rec, int R, int C, int N, int N_cap, int method, int k_reg, uint32_t lam_fix,
                            uint32_t* score_keys, hipStream_t s) {
    launch_body<false>(pkeys, labels_rec, R, C, N, N_cap, method, k_reg, lam_fix, score_keys, nullptr, 0, nullptr, nullptr, ConformalTables{}, s);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_conformal_quantile(const uint32_t* score_keys, int R, int N, int N_cap, const double* coverage, int L, uint32_t* qhat,
                              long long* n_valid, hipStream_t s) {
    ConformalLevels lv = {};
    for (int l = 0; l < L; ++l) lv.v[l] = coverage[l];
    hipLaunchKernelGGL(conformal_quantile_kernel, dim3((unsigned)R), dim3(CF_THREADS), 0, s, score_keys, N, (size_t)N_cap, lv, L, qhat, n_valid);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_conformal_sets(const uint32_t* pkeys, const int* labels_rec, int R, int C, int N, int N_cap, int method, int k_reg, uint32_t lam_fix,
                          const uint32_t* qhat, int L, uint8_t* set_size, uint32_t* members, ConformalTables t, hipStream_t s) {
    const int len = table_len(L, C);
    hipLaunchKernelGGL(conformal_clear_kernel, dim3((unsigned)((len + CF_THREADS - 1) / CF_THREADS), (unsigned)R), dim3(CF_THREADS), 0, s, t, L, C);
    BMI_CHECK_LAUNCH();
    launch_body<true>(pkeys, labels_rec, R, C, N, N_cap, method, k_reg, lam_fix, nullptr, qhat, L, set_size, members, t, s);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
