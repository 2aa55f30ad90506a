// Votes under adaptive sampling and staged early exit (bmi_vote_counts_rows, bmi_vote_decide, bmi_forward_mcd_adaptive_votes,
// bmi_forward_mcd_exit_staged_votes): the image-list form of votes.hip's count kernel, and the stop rule that retires an image once the
// passes still to come can no longer overturn its majority vote.
//
//   vote_counts_rows_kernel  vote_counts_kernel (votes.hip; the exit walk is the one body of vote_walk.h: the same numbers, the same integer
//                            atomics into V int32 [2][E][B][C]) over the images of a list: one wave per (t, i), i < Bc, b = list[i] (list null:
//                            b = i, Bc = B), and of image b only the exits e < n_e[b] (n_e null: all E) — the running exit sum is cut there, so
//                            every count that is added is the one vote_counts_kernel adds for that row.  logits and V keep the full batch
//                            stride B and the ORIGINAL image row (where the heads leave the logits under a row table); rows of images not in
//                            the list and of exits >= n_e[b] are neither read nor written: stale or NaN logits there count for nothing.
//   vote_decide_kernel       the decided-vote rule on one [B][C] row block of V (one kind, one exit), integer arithmetic throughout:
//                                c1   = the lowest class with the largest count
//                                lead = min_{c != c1} (V[c1] - V[c] - (c < c1 ? 1 : 0))        INT_MAX when C == 1
//                                r    = max(0, t_max - t - slack)                               the passes that can still change the outcome
//                                decided  <=>  lead >= r
//                            A class c below c1 overtakes the leader already on a TIE (the lowest index wins), hence the 1.  With lead >= r
//                            no class can reach the leader in r more passes even if every one of them votes for it and none for c1: the
//                            majority vote of the t passes is the majority vote of all t_max passes (slack = 0).
//                            DECIDE: launch_adaptive_decide's list discipline — every image of the active list `in` (null: 0 .. bc-1) gets
//                            t_used[b] = t; the decided ones retire, the others go to `out` in their order, their number to *count.  One
//                            workgroup, one wave per image, VDEC_WAVES images at a time: the survivors of a round take their places behind
//                            those of the rounds before (every thread keeps the running count: the flags are the same for all).
//                            FINAL: converged[b] = the rule at t_used[b], one wave per image of the batch.
#include <climits>
#include <cstdint>

#include "kernels.h"
#include "vote_walk.h"

template <int MAP, bool WEIGHTED>
__global__ __launch_bounds__(VOTE_THREADS) void vote_counts_rows_kernel(const float* __restrict__ logits, int T, int E, int B, int C, int Bc,
                                                                        VoteTau tau, const float* __restrict__ ma, const float* __restrict__ mb,
                                                                        const double* __restrict__ W, int* __restrict__ V, int* nonfinite,
                                                                        const int* __restrict__ list, const int* __restrict__ n_e) {
    extern __shared__ double vote_rows_p[];               // WEIGHTED: [wave][exit][2][64] — p of this lane's two classes
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + wv;       // (t, i), wave-uniform
    if (w >= (long long)T * Bc) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(w / Bc), i = (int)(w - (long long)t * Bc);
    const int b = __builtin_amdgcn_readfirstlane(list ? list[i] : i);
    if ((unsigned)b >= (unsigned)B) return;               // (the whole wave: an index that is no image of the batch touches nothing)
    const int En = __builtin_amdgcn_readfirstlane(n_e ? min(n_e[b], E) : E);
    vote_walk<MAP, WEIGHTED>(logits, t, b, lane, E, En, B, C, tau, ma, mb, W, V, nonfinite, vote_rows_p + (size_t)wv * E * 128 + lane);
}

#define VDEC_WAVES 16

// lead of one row of counts (every lane gets it): see the top of the file
__device__ __forceinline__ int vote_lead(const int* __restrict__ v, int C, int lane) {
    int m = INT_MIN;
    for (int c = lane; c < C; c += 64) m = max(m, v[c]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = max(m, __shfl_xor(m, k));
    int c1 = INT_MAX;
    for (int c = lane; c < C; c += 64)
        if (v[c] == m) c1 = min(c1, c);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) c1 = min(c1, __shfl_xor(c1, k));
    int lead = INT_MAX;
    for (int c = lane; c < C; c += 64)
        if (c != c1) lead = min(lead, m - v[c] - (c < c1 ? 1 : 0));
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) lead = min(lead, __shfl_xor(lead, k));
    return lead;
}

template <bool FINAL>
__global__ __launch_bounds__(VDEC_WAVES * 64) void vote_decide_kernel(const int* __restrict__ Vr, int B, int C, int t, int t_max, int slack,
                                                                      const int* __restrict__ in, int bc, int* __restrict__ out,
                                                                      int* __restrict__ count, int* __restrict__ t_used,
                                                                      uint8_t* __restrict__ converged) {
    __shared__ int keep_s[VDEC_WAVES];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (FINAL) {
        const int b = (int)blockIdx.x * VDEC_WAVES + wv;
        if (b >= bc) return;                              // (wave-uniform)
        const int r = max(0, t_max - t_used[b] - slack);
        const int lead = vote_lead(Vr + (size_t)b * C, C, lane);
        if (lane == 0) converged[b] = lead >= r ? 1 : 0;
        return;
    }
    const int r = max(0, t_max - t - slack);
    int n_out = 0;                                        // the survivors of the rounds so far: the same number in every thread
    for (int base = 0; base < bc; base += VDEC_WAVES) {
        const int i = base + wv;
        int keep = 0, b = -1;
        if (i < bc) {                                     // (wave-uniform)
            b = in ? in[i] : i;
            if ((unsigned)b < (unsigned)B) {              // (an entry that is no image of the batch touches nothing and goes nowhere)
                if (lane == 0) t_used[b] = t;
                keep = vote_lead(Vr + (size_t)b * C, C, lane) >= r ? 0 : 1;
            }
        }
        if (lane == 0) keep_s[wv] = keep;
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < VDEC_WAVES; ++k) {
            const int f = keep_s[k];
            before += k < wv ? f : 0;
            all += f;
        }
        if (keep && lane == 0) out[n_out + before] = b;
        n_out += all;
        __syncthreads();                                  // (the flags are read: the next round may write them)
    }
    if (threadIdx.x == 0) *count = n_out;
}

template <int MAP, bool WEIGHTED>
static void launch_votes_rows(const VoteLaunch& l, hipStream_t s, const float* logits, int T, int E, int B, int C, int Bc, const double* W, int* V,
                              int* nonfinite, const EnsRows& rows) {
    hipLaunchKernelGGL((vote_counts_rows_kernel<MAP, WEIGHTED>), dim3(l.grid), dim3(l.threads), l.lds, s, logits, T, E, B, C, Bc, l.tau, l.ma, l.mb, W,
                       V, nonfinite, rows.list, rows.n_e);
}

int launch_vote_counts_rows(const float* logits, int T, int E, int B, int C, const Calibration& cal, const EnsRows& rows, int* V, int* nonfinite,
                            hipStream_t s) {
    if (rows.list && (rows.Bc < 1 || rows.Bc > B)) return BMI_ERR_INVALID;
    if (cal.check() != BMI_OK) return BMI_ERR_INVALID;
    if (!vote_counts_takes(T, E, B, C)) return BMI_ERR_UNSUPPORTED;      // (Bc <= B: the grid of the list form is no larger)
    const int Bc = rows.list ? rows.Bc : B;
    const VoteLaunch l = vote_launch_plan(cal, E, (int64_t)T * Bc);
#define VOTE_ROWS_CASE(M)                                                                                              \
    case M:                                                                                                            \
        if (l.weighted) launch_votes_rows<M, true>(l, s, logits, T, E, B, C, Bc, cal.ens_w, V, nonfinite, rows);       \
        else launch_votes_rows<M, false>(l, s, logits, T, E, B, C, Bc, cal.ens_w, V, nonfinite, rows);                 \
        break;
    switch (l.map) {
        VOTE_ROWS_CASE(VOTE_MAP_NONE)
        VOTE_ROWS_CASE(VOTE_MAP_TEMP)
        VOTE_ROWS_CASE(VOTE_MAP_VEC)
        VOTE_ROWS_CASE(VOTE_MAP_MAT)
    }
#undef VOTE_ROWS_CASE
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_vote_decide(const int* Vr, int B, int C, int t, int t_max, int slack, const int* in, int bc, int* out, int* count, int* t_used,
                       hipStream_t s) {
    if (!Vr || !out || !count || !t_used || bc <= 0 || bc > B || C <= 0 || t <= 0 || t_max < t || slack < 0 || in == out) return BMI_ERR_INVALID;
    hipLaunchKernelGGL((vote_decide_kernel<false>), dim3(1), dim3(VDEC_WAVES * 64), 0, s, Vr, B, C, t, t_max, slack, in, bc, out, count, t_used,
                       (uint8_t*)nullptr);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

int launch_vote_converged(const int* Vr, int C, int t_max, int slack, int batch, const int* t_used, uint8_t* converged, hipStream_t s) {
    if (!Vr || !t_used || !converged || batch <= 0 || C <= 0 || t_max <= 0 || slack < 0) return BMI_ERR_INVALID;
    hipLaunchKernelGGL((vote_decide_kernel<true>), dim3((unsigned)((batch + VDEC_WAVES - 1) / VDEC_WAVES)), dim3(VDEC_WAVES * 64), 0, s, Vr, batch, C, 0,
                       t_max, slack, (const int*)nullptr, batch, (int*)nullptr, (int*)nullptr, (int*)t_used, converged);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}
