// The sorted form of the rank call (bmi_rank_quality_sorted) and the detection read-out (bmi_rank_detection).
//
// bmi_rank_quality_sorted takes the inputs of ranking.hip's rank call and gives its five outputs — rank, sorted_keys, curve, counts =
// (m, n_pos, U2), aurc_sum — under THE ARITHMETIC CONTRACT at the top of ranking.hip, bit for bit, for rows of 1 <= N < 2^22 images: a
// stable multi-row LSD radix sort for wave64 in place of the O(N^2) counting.  train.ranking.rank_quality_numpy restates both calls.
//
// Sort word and payload.  The sort word of an image is its ukey, a ukey above 0x7F7FFFFF read as 0xFFFFFFFF: the invalid images land
// behind the m valid ones, so the sorted words ARE sorted_keys, tail included.  The payload is the image index (< 2^22) with the positive
// bit in bit 31.
//
// Passes.  Four passes of 8 bits, least significant digit first, over ping-pong buffers in the caller's scratch (pass 0 reads ukeys /
// positive, pass 3 writes its words into sorted_keys).  A pass is three launches over all R rows at once (grid.y = row); a tile is
// BMI_RANK_SORT_TILE consecutive positions of one row:
//   (a) sort_hist_kernel     grid (tiles, R).  A thread owns RS_KPT consecutive positions; the workgroup builds a 256-bin LDS histogram
//                            with integer atomics, a run of equal digits in one thread with ONE atomic, and writes hist[row][digit][tile].
//   (b) row_scan_kernel      grid (R).  One workgroup per row: the exclusive scan of the row's hist in (digit, tile) order, in place.
//   (c) sort_scatter_kernel  grid (tiles, R).  The tile again, wave w taking its positions w * 64 * RS_KPT + i * 64 + lane in steps i: the
//                            wave's elements in position order.  Per step eight __ballots of the digit's bits are ANDed to the mask of
//                            the lanes that hold the same digit; an element's place among the wave's keys of its digit is the wave's
//                            count so far (LDS [waves][256]) plus the popcount of the mask below the lane, and the highest lane of the
//                            mask adds the mask's popcount to the count.  After the last step the counts are scanned across the waves
//                            once, on top of the tile's scanned hist entry, and every element goes to base + place: stable, no
//                            comparison, no per-key global atomic.  The last pass also scatters rank[image] = position (-1: invalid).
// The launch sequence depends on (R, N) only; the launches are the only ordering — no workgroup waits on another.
//
// Read-out, position order (positive bit of position k: payload bit 31 where the word is valid):
//   curve_sum_kernel   grid (tiles, R): the tile's positives -> tsum[row][tile];  row_scan_kernel over tsum;
//   curve_apply_kernel grid (tiles, R): curve[k] = the inclusive scan (ballots per wave, the waves' sums through LDS); the tail is n_pos.
//   rank_u2_kernel     grid (tiles, R): every position that starts a tie group (k == 0 or key[k-1] != key[k]) finds the group's end by an
//                      upper-bound binary search in sorted_keys and adds pos_in_group * (2 neg_before + neg_in_group); the workgroup's
//                      int64 partial goes to the scratch.
//   sort_finish_kernel grid (R): the partials joined as rank_finish_kernel joins them, m = the first position of 0xFFFFFFFF, n_pos =
//                      curve[N-1], aurc_sum by ordered_sum<1> over curve[k] / (k + 1): ranking.hip's expression in ranking.hip's order.
// Integers only apart from aurc_sum; no floating-point atomics: the same bits on every run and for every cut into record calls.
//
// bmi_rank_detection reads the sorted_keys, curve and counts of either rank call.  A threshold sits at a tie-group boundary: "flag every
// image whose key is at least the key of the group starting at position s" has TP(s) = n_pos - curve[s-1] (curve[-1] = 0) and FP(s) =
// (m - s) - TP(s).  rank_detection_kernel, grid (R), restated by train.ranking.rank_detection_numpy:
//   ap_sum float64 [R][2]   ordered_sum<2> over i = 0 .. m-1, every quotient the correctly rounded division of two integers converted
//                           exactly (the product formed in int64), a position that is no boundary adding +0.0; 0.0 where m = 0:
//                           [0] position s = m-1-i (DESCENDING): a group start adds pos_in_group * TP(s) / (m - s);
//                           [1] end e = i+1 (exclusive, ASCENDING): a group end adds neg_in_group * (e - curve[e-1]) / e.
//   det int64 [R][L][2]     thread l < L: need = min(max((long) ceil(q_l * (double) n_pos), 1), n_pos); the largest position p whose
//                           curve[p-1] <= n_pos - need (binary search on curve), snapped down to the start s of p's group:
//                           (TP(s), FP(s)); (0, 0) where n_pos = 0.
#include <cstdint>

#include "record_common.h"

#pragma clang fp contract(off)

#define RS_THREADS RECORD_THREADS
#define RS_WAVES (RS_THREADS / 64)
#define RS_TILE BMI_RANK_SORT_TILE
#define RS_KPT (RS_TILE / RS_THREADS)     // positions of a tile per thread
#define RS_SCAN 8                         // consecutive entries per thread and step of row_scan_kernel
#define RS_INVALID 0xFFFFFFFFu
#define RS_MAX_KEY 0x7F7FFFFFu
#define RS_INDEX 0x003FFFFFu              // the payload's image index
#define RS_DET_MAX BMI_RANK_DET_MAX_LEVELS

static_assert(RS_TILE % RS_THREADS == 0 && RS_KPT >= 1 && RS_THREADS == 256, "whole steps per wave; one thread per digit");
static_assert(BMI_RANK_SORT_MAX_IMAGES <= (int)RS_INDEX, "the image index fits the payload");

struct TprLevels { double q[RS_DET_MAX]; };

// the sort word at position k of a row: the caller's ukey in pass 0 (clamped), the ping-pong buffer's word afterwards
template <bool FIRST>
__device__ __forceinline__ uint32_t sort_word(const uint32_t* __restrict__ keys, int k) {
    const uint32_t u = keys[k];
    return FIRST && u > RS_MAX_KEY ? RS_INVALID : u;
}

// the first position of [lo, hi) whose word is above `key` (UPPER) / not below it (lower bound); hi when there is none
template <bool UPPER>
__device__ __forceinline__ int key_bound(const uint32_t* __restrict__ sk, uint32_t key, int lo, int hi) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const uint32_t v = sk[mid];
        if (UPPER ? v <= key : v < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool FIRST>
__global__ __launch_bounds__(RS_THREADS) void sort_hist_kernel(const uint32_t* __restrict__ key_in, size_t stride_in, int N, int shift, int tiles,
                                                                int* __restrict__ hist) {
    __shared__ int h[256];
    const int tid = threadIdx.x, tile = blockIdx.x, r = blockIdx.y;
    const uint32_t* keys = key_in + (size_t)r * stride_in;
    h[tid] = 0;
    __syncthreads();
    const int k0 = tile * RS_TILE + tid * RS_KPT;            // the thread's run of consecutive positions
    int cur = -1, run = 0;                  // its run of equal digits, added at once
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) {
        if (k0 + i >= N) break;
        const int d = (int)((sort_word<FIRST>(keys, k0 + i) >> shift) & 255u);
        if (d != cur) {
            if (run) atomicAdd(&h[cur], run);
            cur = d;
            run = 0;
        }
        ++run;
    }
    if (run) atomicAdd(&h[cur], run);
    __syncthreads();
    hist[((size_t)r * 256 + tid) * tiles + tile] = h[tid];
}

// the exclusive scan of n entries per row, in place, by one workgroup: RS_SCAN consecutive entries per thread and step, the threads' sums
// scanned by shuffles inside a wave and through LDS across the waves, a running carry from step to step
__global__ __launch_bounds__(RS_THREADS) void row_scan_kernel(int* __restrict__ data, int n) {
    __shared__ int wave_sum[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* d = data + (size_t)blockIdx.x * n;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += RS_THREADS * RS_SCAN) {
        const int base = i0 + tid * RS_SCAN;
        int v[RS_SCAN], sum = 0;
#pragma unroll
        for (int j = 0; j < RS_SCAN; ++j) {
            v[j] = base + j < n ? d[base + j] : 0;
            sum += v[j];
        }
        int incl = sum;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int up = __shfl_up(incl, s);
            if (lane >= s) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int below = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
            const int ws = wave_sum[w];
            below += w < wave ? ws : 0;
            total += ws;
        }
        int at = carry + below + incl - sum;
#pragma unroll
        for (int j = 0; j < RS_SCAN; ++j) {
            if (base + j < n) d[base + j] = at;
            at += v[j];
        }
        carry += total;
        __syncthreads();                    // (wave_sum is rewritten by the next step)
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(RS_THREADS) void sort_scatter_kernel(const uint32_t* __restrict__ key_in, size_t stride_in,
                                                                   const uint32_t* __restrict__ pay_in, const uint8_t* __restrict__ positive,
                                                                   int N, int shift, int tiles, const int* __restrict__ hist,
                                                                   uint32_t* __restrict__ key_out, size_t stride_out,
                                                                   uint32_t* __restrict__ pay_out, int* __restrict__ rank) {
    __shared__ int cnt[RS_WAVES][256];      // per wave and digit: the keys seen so far, then the first destination
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, r = blockIdx.y;
    const uint32_t* keys = key_in + (size_t)r * stride_in;
    const uint32_t* pays = FIRST ? nullptr : pay_in + (size_t)r * N;
    const uint8_t* pos = FIRST ? positive + (size_t)r * stride_in : nullptr;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const int k0 = tile * RS_TILE + wave * (64 * RS_KPT) + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t key[RS_KPT], pay[RS_KPT];
    int place[RS_KPT];
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) {
        const int k = k0 + i * 64;
        const bool in = k < N;
        key[i] = in ? sort_word<FIRST>(keys, k) : 0u;
        pay[i] = !in ? 0u : FIRST ? (uint32_t)k | (pos[k] != 0 ? 0x80000000u : 0u) : pays[k];
        const int d = (int)((key[i] >> shift) & 255u);
        unsigned long long same = __ballot(in);              // the lanes of this step that hold the lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long set = __ballot(bit);
            same &= bit ? set : ~set;
        }
        const int seen = cnt[wave][d];
        place[i] = seen + __popcll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (in && (same >> lane) == 1ull) cnt[wave][d] = seen + __popcll(same);      // the highest lane of the digit: one writer per counter
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    int at = hist[((size_t)r * 256 + tid) * tiles + tile];   // digit tid: the tile's first destination, then wave by wave
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
        const int c = cnt[w][tid];
        cnt[w][tid] = at;
        at += c;
    }
    __syncthreads();
    uint32_t* ko = key_out + (size_t)r * stride_out;
    uint32_t* po = pay_out + (size_t)r * N;
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) {
        if (k0 + i * 64 >= N) continue;
        const int dest = cnt[wave][(key[i] >> shift) & 255u] + place[i];
        if ((unsigned)dest >= (unsigned)N) continue;         // (a permutation of 0 .. N-1: never taken)
        ko[dest] = key[i];
        po[dest] = pay[i];
        const uint32_t image = pay[i] & RS_INDEX;            // (below N likewise)
        if (LAST && image < (uint32_t)N) rank[(size_t)r * stride_out + image] = key[i] == RS_INVALID ? -1 : dest;
    }
}

// the positive bit of position k: the payload's bit 31 where the sorted word is valid
__device__ __forceinline__ bool position_bit(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ pay, int k, int N) {
    return k < N && (pay[k] >> 31) != 0u && sk[k] != RS_INVALID;
}

__global__ __launch_bounds__(RS_THREADS) void curve_sum_kernel(const uint32_t* __restrict__ sorted_keys, size_t N_cap,
                                                                const uint32_t* __restrict__ pay_in, int N, int tiles, int* __restrict__ tsum) {
    __shared__ int total;
    const int tid = threadIdx.x, tile = blockIdx.x, r = blockIdx.y;
    const uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    const uint32_t* pay = pay_in + (size_t)r * N;
    if (tid == 0) total = 0;
    __syncthreads();
    int c = 0;                              // (wave-uniform)
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) c += __popcll(__ballot(position_bit(sk, pay, tile * RS_TILE + i * RS_THREADS + tid, N)));
    if ((tid & 63) == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (tid == 0) tsum[(size_t)r * tiles + tile] = total;
}

__global__ __launch_bounds__(RS_THREADS) void curve_apply_kernel(const uint32_t* __restrict__ sorted_keys, size_t N_cap,
                                                                  const uint32_t* __restrict__ pay_in, int N, int tiles,
                                                                  const int* __restrict__ tsum, int* __restrict__ curve) {
    __shared__ int wave_sum[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, r = blockIdx.y;
    const uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    const uint32_t* pay = pay_in + (size_t)r * N;
    int* cv = curve + (size_t)r * N_cap;
    const int k0 = tile * RS_TILE + wave * (64 * RS_KPT) + lane;
    const unsigned long long upto = ~0ull >> (63 - lane);    // the lanes at and below this one
    unsigned long long bits[RS_KPT];        // (wave-uniform)
    int c = 0;
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) {
        bits[i] = __ballot(position_bit(sk, pay, k0 + i * 64, N));
        c += __popcll(bits[i]);
    }
    if (lane == 0) wave_sum[wave] = c;
    __syncthreads();
    int run = tsum[(size_t)r * tiles + tile];                // the positives below the tile, then below the wave, then below the step
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) run += w < wave ? wave_sum[w] : 0;
#pragma unroll
    for (int i = 0; i < RS_KPT; ++i) {
        const int k = k0 + i * 64;
        if (k < N) cv[k] = run + __popcll(bits[i] & upto);
        run += __popcll(bits[i]);
    }
}

__global__ __launch_bounds__(RS_THREADS) void rank_u2_kernel(const uint32_t* __restrict__ sorted_keys, const int* __restrict__ curve, int N,
                                                              size_t N_cap, int tiles, long long* __restrict__ partial) {
    __shared__ unsigned long long total;
    const int tid = threadIdx.x, tile = blockIdx.x, r = blockIdx.y;
    const uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    const int* cv = curve + (size_t)r * N_cap;
    if (tid == 0) total = 0ull;
    __syncthreads();
    long long u2 = 0;
#pragma unroll 1
    for (int i = 0; i < RS_KPT; ++i) {
        const int k = tile * RS_TILE + i * RS_THREADS + tid;
        if (k >= N) break;
        const uint32_t key = sk[k];
        if (key == RS_INVALID || (k && sk[k - 1] == key)) continue;
        const int e = key_bound<true>(sk, key, k + 1, N);    // one past the group's last position (the invalid tail lies above every key)
        const int pos_before = k ? cv[k - 1] : 0;
        const int pos_in = cv[e - 1] - pos_before, neg_before = k - pos_before, neg_in = (e - k) - pos_in;
        u2 += (long long)pos_in * (2ll * neg_before + neg_in);
    }
    if (u2) atomicAdd(&total, (unsigned long long)u2);       // (LDS, integers: order-free)
    __syncthreads();
    if (tid == 0) partial[(size_t)r * tiles + tile] = (long long)total;
}

__global__ __launch_bounds__(RS_THREADS) void sort_finish_kernel(int N, size_t N_cap, int tiles, const long long* __restrict__ partial,
                                                                  const uint32_t* __restrict__ sorted_keys, const int* __restrict__ curve,
                                                                  long long* __restrict__ counts, double* __restrict__ aurc_sum) {
    __shared__ double term[1][RL_TILE];
    __shared__ unsigned long long total;
    __shared__ int valid;
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    const int* cv = curve + (size_t)r * N_cap;
    if (tid == 0) {
        total = 0ull;
        valid = key_bound<false>(sk, RS_INVALID, 0, N);
    }
    __syncthreads();
    for (int t = tid; t < tiles; t += RS_THREADS) {
        const long long v = partial[(size_t)r * tiles + t];
        if (v) atomicAdd(&total, (unsigned long long)v);
    }
    __syncthreads();
    const int m = valid;
    double acc[1] = {0.0};                  // position order
    ordered_sum<1>(m, term, acc, [&](int k, double (&t)[1]) { t[0] = (double)cv[k] / (double)(k + 1); });
    if (tid == 0) {
        counts[(size_t)r * 3] = m;
        counts[(size_t)r * 3 + 1] = cv[N - 1];
        counts[(size_t)r * 3 + 2] = (long long)total;
        aurc_sum[r] = acc[0];
    }
}

__global__ __launch_bounds__(RS_THREADS) void rank_detection_kernel(const uint32_t* __restrict__ sorted_keys, const int* __restrict__ curve,
                                                                     const long long* __restrict__ counts, int N, size_t N_cap, TprLevels tpr,
                                                                     int L, double* __restrict__ ap_sum, long long* __restrict__ det) {
    __shared__ double term[2][RL_TILE];
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint32_t* sk = sorted_keys + (size_t)r * N_cap;
    const int* cv = curve + (size_t)r * N_cap;
    const int m = (int)min(max(counts[(size_t)r * 3], 0ll), (long long)N);           // (a rank call's counts: 0 <= n_pos <= m <= N)
    const int n_pos = (int)min(max(counts[(size_t)r * 3 + 1], 0ll), (long long)m);
    double acc[2] = {0.0, 0.0};
    ordered_sum<2>(m, term, acc, [&](int i, double (&t)[2]) {
        t[0] = t[1] = 0.0;
        const int s = m - 1 - i;            // descending: does a group start here?
        const uint32_t ks = sk[s];
        if (s == 0 || sk[s - 1] != ks) {
            const int end = key_bound<true>(sk, ks, s + 1, m);
            const int before = s ? cv[s - 1] : 0;
            t[0] = (double)((long long)(cv[end - 1] - before) * (long long)(n_pos - before)) / (double)(m - s);
        }
        const int e = i + 1;                // ascending: does a group end (exclusive) here?
        const uint32_t ke = sk[e - 1];
        if (e == m || sk[e] != ke) {
            const int start = key_bound<false>(sk, ke, 0, e - 1);
            const int before = start ? cv[start - 1] : 0;
            const long long neg_in = (long long)(e - start) - (long long)(cv[e - 1] - before);
            t[1] = (double)(neg_in * (long long)(e - cv[e - 1])) / (double)e;
        }
    });
    if (tid == 0) {
        ap_sum[(size_t)r * 2] = acc[0];
        ap_sum[(size_t)r * 2 + 1] = acc[1];
    }
    if (tid < L) {
        long long tp = 0, fp = 0;
        if (n_pos > 0) {
            const long long up = (long long)ceil(tpr.q[tid] * (double)n_pos);
            const int room = n_pos - (int)min(max(up, 1ll), (long long)n_pos);       // curve[s-1] may be at most this
            int lo = 0, hi = m - 1;         // the largest position p with curve[p-1] <= room (p = 0 always holds)
            while (lo < hi) {
                const int mid = lo + ((hi - lo + 1) >> 1);
                if (cv[mid - 1] <= room) lo = mid; else hi = mid - 1;
            }
            const int s = key_bound<false>(sk, sk[lo], 0, lo);
            tp = n_pos - (s ? cv[s - 1] : 0);
            fp = (long long)(m - s) - tp;
        }
        det[((size_t)r * L + tid) * 2] = tp;
        det[((size_t)r * L + tid) * 2 + 1] = fp;
    }
}

bool rank_sort_takes(int R, int N) { return R >= 1 && R <= BMI_RANK_MAX_ROWS && N >= 1 && N <= BMI_RANK_SORT_MAX_IMAGES; }

static int sort_tiles(int N) { return (N + RS_TILE - 1) / RS_TILE; }

// int32 hist [R][256][tiles] (after the passes: int64 partial [R][tiles], then int32 tsum [R][tiles]), then the four uint32 [R][N]
// ping-pong buffers key A, payload A, key B, payload B
size_t rank_sort_scratch_bytes(int R, int N) {
    if (!rank_sort_takes(R, N)) return 0;
    return ((size_t)R * 256 * (size_t)sort_tiles(N) + 4 * (size_t)R * (size_t)N) * sizeof(uint32_t);
}

int launch_rank_quality_sorted(const uint32_t* ukeys, const uint8_t* positive, int R, int N, int N_cap, int* rank, uint32_t* sorted_keys,
                               int* curve, long long* counts, double* aurc_sum, void* scratch, hipStream_t s) {
    if (!rank_sort_takes(R, N)) return BMI_ERR_UNSUPPORTED;
    const int tiles = sort_tiles(N);
    const size_t cells = (size_t)R * (size_t)N;
    int* hist = (int*)scratch;
    uint32_t* key_a = (uint32_t*)scratch + (size_t)R * 256 * (size_t)tiles;
    uint32_t *pay_a = key_a + cells, *key_b = pay_a + cells, *pay_b = key_b + cells;
    long long* partial = (long long*)scratch;
    int* tsum = hist + 2 * (size_t)R * (size_t)tiles;
    const dim3 grid((unsigned)tiles, (unsigned)R), rows((unsigned)R), block(RS_THREADS);
    const size_t n = (size_t)N, cap = (size_t)N_cap;
#define RS_PASS(FIRST, LAST, shift, kin, sin, pin, kout, sout, pout)                                                                       \
    hipLaunchKernelGGL((sort_hist_kernel<FIRST>), grid, block, 0, s, kin, sin, N, shift, tiles, hist);                                     \
    BMI_CHECK_LAUNCH();                                                                                                                    \
    hipLaunchKernelGGL(row_scan_kernel, rows, block, 0, s, hist, 256 * tiles);                                                             \
    BMI_CHECK_LAUNCH();                                                                                                                    \
    hipLaunchKernelGGL((sort_scatter_kernel<FIRST, LAST>), grid, block, 0, s, kin, sin, pin, positive, N, shift, tiles, (const int*)hist,  \
                       kout, sout, pout, rank);                                                                                            \
    BMI_CHECK_LAUNCH()
    RS_PASS(true, false, 0, ukeys, cap, (const uint32_t*)nullptr, key_a, n, pay_a);
    RS_PASS(false, false, 8, (const uint32_t*)key_a, n, (const uint32_t*)pay_a, key_b, n, pay_b);
    RS_PASS(false, false, 16, (const uint32_t*)key_b, n, (const uint32_t*)pay_b, key_a, n, pay_a);
    RS_PASS(false, true, 24, (const uint32_t*)key_a, n, (const uint32_t*)pay_a, sorted_keys, cap, pay_b);
#undef RS_PASS
    hipLaunchKernelGGL(curve_sum_kernel, grid, block, 0, s, (const uint32_t*)sorted_keys, cap, (const uint32_t*)pay_b, N, tiles, tsum);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(row_scan_kernel, rows, block, 0, s, tsum, tiles);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(curve_apply_kernel, grid, block, 0, s, (const uint32_t*)sorted_keys, cap, (const uint32_t*)pay_b, N, tiles,
                       (const int*)tsum, curve);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(rank_u2_kernel, grid, block, 0, s, (const uint32_t*)sorted_keys, (const int*)curve, N, cap, tiles, partial);
    BMI_CHECK_LAUNCH();
    hipLaunchKernelGGL(sort_finish_kernel, rows, block, 0, s, N, cap, tiles, (const long long*)partial, (const uint32_t*)sorted_keys,
                       (const int*)curve, counts, aurc_sum);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

bool rank_detection_takes(int R, int N, int L) { return rank_sort_takes(R, N) && L >= 1 && L <= RS_DET_MAX; }

int launch_rank_detection(const uint32_t* sorted_keys, const int* curve, const long long* counts, int R, int N, int N_cap, const double* tpr,
                          int L, double* ap_sum, long long* det, hipStream_t s) {
    if (!rank_detection_takes(R, N, L)) return BMI_ERR_UNSUPPORTED;
    TprLevels levels = {};
    for (int l = 0; l < L; ++l) levels.q[l] = tpr[l];
    hipLaunchKernelGGL(rank_detection_kernel, dim3((unsigned)R), dim3(RS_THREADS), 0, s, sorted_keys, curve, counts, N, (size_t)N_cap, levels, L,
                       ap_sum, det);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
