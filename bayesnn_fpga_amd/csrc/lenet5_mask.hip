// Masksembles LeNet-5 (the network of lenet5.hip with sites A, B, C of kind BMI_SITE_MASKSEMBLE) as ONE kernel.  A Masksembles mask is the same
// for every image, depends on the channel / unit alone, repeats with period M and carries no rescale and no random draw, so this kernel has
// another shape than lenet5_kernel (per-image Philox bits, a masked copy of the map, five to six barriers per sample).  Replaces T forwards
// of the Keras LeNet with `dropout_type == "mask"` (Hardware_Artifact/bayes_hw/models/model_utils.py:43-52, models.py:34-73) plus the softmax /
// averaging of FullAnalysis._get_output (SA/train/results_analyzer.py:236-248).
//
// Work split   grid.x = image, grid.y = chunk of PASSES, 256 threads = 4 waves.  A call's samples t0 .. t0+tc-1 use the masks (t0 + i) mod M:
//              only D = min(tc, M) passes differ, so the workgroup runs pass d = 0 .. D-1 with mask (t0 + d) mod M and weighs it by the
//              n_d = (tc - d + M - 1) / M samples it stands for: S1 += n_d p, S2 += n_d p p, SL += n_d z in float64 registers, d ascending
//              (the products are exact in float64); `logits` receives pass d's row at every i = d (mod M).  Small batches split the D
//              passes over grid.y by lenet5_chunks(B, D); lenet5_mask_join_kernel adds the chunks' partials onto S in chunk order.
// Prefix       as lenet5_kernel: the haloed fp32 image, conv1 + bias + ReLU + 2x2 max in fp32 -> P1, fp16 [18][18][24] in LDS.  The image
//              and conv1's weights live in the room of fc2's weights, which are copied in behind conv1.  Everything in front of the
//              first site that is on runs once.  The mask rows (fp32 [M][C] in global memory, any nonzero = keep) become a bit table in
//              LDS, eight words per mask: word 0 site A (20 bits), 1..3 site B (80), 4..7 site C (100).
// Site A       no masked copy of P1.  A lane's MFMA weight fragment is eight consecutive k of ONE K-group kg = the channels 8 (kg % 3) ..
//              + 7 of one tap, so the mask is ANDed onto the weight fragment in registers (0xFFFF per kept channel): a zeroed fp16 weight
//              gives the exact zero product a zeroed activation gives.  kg = 4 ks + lg, so kg % 3 = (ks + lg) % 3: the lane builds its
//              three 128-bit patterns once per pass in the order it meets them and the K-loop is unrolled by three (19 = 6 * 3 + 1).
// conv2        lenet5_kernel's: the same 19 K-steps in the same order on v_mfma_f32_16x16x32_f16, wave q = pooling window q, bias + ReLU +
//              7x7 max in registers and four xor-shuffles.  fc1 (threads 0..99, 80 weights in registers), fc2 + softmax: the same chains.
// Pipeline     site A on: conv2(d) on all four waves -> the 80 features, masked by site B's bits as they are written | barrier | fc1(d) on
//              waves 0 and 1 -> the 100 hidden units (masked by site C's bits) BESIDE fc2 + softmax + sums of pass d-1 on wave 3 | barrier.
//              The hidden units are double-buffered for that; two barriers per pass, and the longer of fc1 and fc2 instead of their sum
//              on the critical path.  Site A off, B on: conv2 once; per pass wave 2 masks the next pass's features beside fc1(d) and
//              fc2(d-1): both buffers double, one barrier per pass.  Site C alone: fc1 once, wave 3 masks the hidden units as it reads
//              them: no barrier in the loop.
// LDS          P1 15 552 + conv2 fragments 24 320 + fc2 12 800 + offsets 304 + bit table 1 024 + features 960 + hidden units 1 200 =
//              56 160 bytes: two workgroups per CU.
#include <algorithm>

#include "kernels.h"

namespace {

typedef _Float16 lm_half8 __attribute__((ext_vector_type(8)));
typedef float lm_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lm_u32x4 __attribute__((ext_vector_type(4)));

constexpr int LM_THREADS = 256;
constexpr int LM_P1_W = 18, LM_P1_C = 24, LM_P1_HALVES = LM_P1_W * LM_P1_W * LM_P1_C;     // 7776
constexpr int LM_KG = 76;                       // K-groups of 8 (75 live), 19 K-steps of 32
constexpr int LM_EA = 3920, LM_EB = 80, LM_EC = 100;      // elements per image of the three sites
constexpr int LM_MAX_MASKS = 32, LM_WORDS = 8;  // bit table: word 0 site A, 1..3 site B, 4..7 site C
constexpr int LM_WB = 1, LM_WC = 4;

__device__ __forceinline__ bool lm_bit(const uint32_t* w, int j) { return (w[j >> 5] >> (j & 31)) & 1u; }

// eight channels' keep bits -> 0xFFFF per kept fp16 lane of a weight fragment
__device__ __forceinline__ lm_u32x4 lm_pattern(uint32_t bits) {
    lm_u32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = ((bits >> (2 * r)) & 1u ? 0xFFFFu : 0u) | ((bits >> (2 * r + 1)) & 1u ? 0xFFFF0000u : 0u);
    return p;
}

// one K-step of conv2: K-group kg, its weight fragments ANDed with `pat`
__device__ __forceinline__ void lm_kstep(const _Float16* s_p1, const _Float16* s_w2, const int* s_koff, const int pbase[4], int kg, int ln, lm_u32x4 pat,
                                         lm_f32x4 acc[4][2]) {
    union { lm_u32x4 u; lm_half8 h; } w0, w1;
    const int koff = s_koff[kg];
    w0.u = *(const lm_u32x4*)(s_w2 + (kg * 20 + ln) * 8) & pat;
    w1.u = lm_u32x4{0u, 0u, 0u, 0u};
    if (ln < 4) w1.u = *(const lm_u32x4*)(s_w2 + (kg * 20 + 16 + ln) * 8) & pat;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const lm_half8 px = *(const lm_half8*)(s_p1 + pbase[mt] + koff);
        acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0.h, px, acc[mt][0], 0, 0, 0);
        acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1.h, px, acc[mt][1], 0, 0, 0);
    }
}

// conv2 + bias + ReLU + 7x7 max of the wave's pooling window under the channel mask in pat[] (pat[j]: the pattern of channel group
// (lg + j) % 3, the group of the lane's K-step ks = j mod 3); the lanes with (lane & 15) == 0 return their channels' maxima in v[]:
// v[r] = channel 4 * (lane >> 4) + r, v[4 + r] = channel 16 + r (lanes 0..15 only)
__device__ __forceinline__ void lm_conv2(const _Float16* s_p1, const _Float16* s_w2, const int* s_koff, const int pbase[4], int lane, const lm_u32x4 pat[3],
                                         const float bias[8], float v[8]) {
    const int lg = lane >> 4, ln = lane & 15;
    lm_f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = lm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k3 = 0; k3 < 18; k3 += 3) {
#pragma unroll
        for (int j = 0; j < 3; ++j) lm_kstep(s_p1, s_w2, s_koff, pbase, (k3 + j) * 4 + lg, ln, pat[j], acc);
    }
    lm_kstep(s_p1, s_w2, s_koff, pbase, 72 + lg, ln, pat[0], acc);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = fmaxf(fmaxf(acc[0][nt][r], acc[1][nt][r]), fmaxf(acc[2][nt][r], acc[3][nt][r]));
            m = fmaxf(fmaf(m, 1.f, bias[nt * 4 + r]), 0.f);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
            v[nt * 4 + r] = m;
        }
}

// the wave's 20 features of window `wave` -> dst in torch's flatten order (channel * 4 + window); bbits: site B's keep bits or null
__device__ __forceinline__ void lm_store_features(float* dst, const float v[8], int lane, int wave, const uint32_t* bbits) {
    const int lg = lane >> 4;
    if ((lane & 15) != 0) return;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (r >= 4 && lg != 0) break;
        const int j = (r < 4 ? lg * 4 + r : 12 + r) * 4 + wave;
        dst[j] = (!bbits || lm_bit(bbits, j)) ? v[r] : 0.f;
    }
}

__device__ __forceinline__ float lm_fc1(const float* f, const float w[LM_EB], float bias) {
    float h = bias;
#pragma unroll
    for (int k = 0; k < LM_EB; ++k) h = fmaf(f[k], w[k], h);
    return fmaxf(h, 0.f);
}

struct LmSums {
    double s1, s2, sl;
};

// fc2, softmax and the weighted moment sums of pass d on one wave, lane = class; cbits: site C's keep bits when h is not masked yet, else null
__device__ __forceinline__ void lm_fc2(const float* h, const uint32_t* cbits, const float* s_fc2, float b_fc2, int lane, int C, int d, int M,
                                       const Lenet5Args& a, int b, LmSums& s) {
    float z = b_fc2;
    if (cbits) {
#pragma unroll 4
        for (int k = 0; k < LM_EC; ++k) z = fmaf(lm_bit(cbits, k) ? h[k] : 0.f, s_fc2[k * 32 + (lane & 31)], z);
    } else {
#pragma unroll 4
        for (int k = 0; k < LM_EC; ++k) z = fmaf(h[k], s_fc2[k * 32 + (lane & 31)], z);
    }
    float m = lane < C ? z : -INFINITY;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    const float e = lane < C ? expf(z - m) : 0.f;
    float sum = e;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane < C) {
        const double p = (double)(e / sum), n = (double)((a.tc - d + M - 1) / M);      // the samples i = d (mod M) of the call
        s.s1 += n * p;
        s.s2 += n * (p * p);
        s.sl += n * (double)z;
        if (a.logits)
            for (int i = d; i < a.tc; i += M) a.logits[((size_t)i * a.B + b) * C + lane] = z;
    }
}

__global__ __launch_bounds__(LM_THREADS, 2) void lenet5_mask_kernel(Lenet5Args a) {
    __shared__ __attribute__((aligned(16))) _Float16 s_p1[LM_P1_HALVES];
    __shared__ __attribute__((aligned(16))) _Float16 s_w2[LM_KG * 20 * 8];
    __shared__ __attribute__((aligned(16))) float s_fc2[LM_EC * 32];            // prefix: the haloed image and conv1's weights
    __shared__ int s_koff[LM_KG];
    __shared__ uint32_t s_bits[LM_MAX_MASKS][LM_WORDS];
    __shared__ float s_feat[LM_EB], s_fM[2][LM_EB], s_hpre[LM_EC], s_hM[2][LM_EC];
    float* const s_img = s_fc2;               // [32][32]
    float* const s_w1 = s_img + 1024;         // [20][25] then the 20 biases

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C;
    const SiteArgs& sA = a.site[0];
    const SiteArgs& sB = a.site[1];
    const SiteArgs& sC = a.site[2];
    const bool onA = sA.kind != BMI_SITE_NONE, onB = sB.kind != BMI_SITE_NONE, onC = sC.kind != BMI_SITE_NONE;
    const int M = onA ? sA.num_masks : (onB ? sB.num_masks : sC.num_masks);
    const int d0 = (int)blockIdx.y * a.per_chunk;                  // the chunk's passes d0 .. d0 + n_p - 1 of the call's min(tc, M)
    const int n_p = min(a.per_chunk, min(a.tc, M) - d0);
    const int m0 = a.t0 % M;

    // ---- prefix: staging ----------------------------------------------------------------------------------------------------------
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += LM_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? img[r * 28 + c] : 0.f;
    }
    for (int i = tid; i < 520; i += LM_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < LM_P1_HALVES / 8; i += LM_THREADS) ((uint4*)s_p1)[i] = uint4{0u, 0u, 0u, 0u};
    for (int i = tid; i < LM_KG * 20; i += LM_THREADS) ((uint4*)s_w2)[i] = ((const uint4*)a.w2f)[i];
    if (tid < LM_KG) {      // K-group -> offset of its tap and channel group inside the haloed map (group 75: zero weights, any valid offset)
        const int kg = min(tid, LM_KG - 2), tap = kg / 3;
        s_koff[tid] = ((tap / 5) * LM_P1_W + tap % 5) * LM_P1_C + (kg % 3) * 8;
    }
    if (tid < M * LM_WORDS) {      // one word of the bit table per thread
        const int m = tid / LM_WORDS, w = tid % LM_WORDS;
        const int st = w < LM_WB ? 0 : (w < LM_WC ? 1 : 2);
        const int n = st == 0 ? 20 : (st == 1 ? LM_EB : LM_EC), j0 = (w - (st == 0 ? 0 : (st == 1 ? LM_WB : LM_WC))) * 32;
        const float* mk = st == 0 ? sA.masks : (st == 1 ? sB.masks : sC.masks);
        const bool on = st == 0 ? onA : (st == 1 ? onB : onC);
        uint32_t word = 0u;
        if (on)
            for (int i = 0; i < 32 && j0 + i < n; ++i) word |= (mk[m * n + j0 + i] != 0.f ? 1u : 0u) << i;
        s_bits[m][w] = word;
    }
    __syncthreads();

    // ---- prefix: conv1 + bias + ReLU + 2x2 max -> P1 -------------------------------------------------------------------------------
    for (int i = tid; i < LM_EA; i += LM_THREADS) {
        const int c = i % 20, pos = i / 20, y = pos / 14, x = pos % 14;
        float p[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q) p[r][q] = s_img[(2 * y + r) * 32 + 2 * x + q];
        const float bias = s_w1[500 + c];
        float o00 = bias, o01 = bias, o10 = bias, o11 = bias;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const float w = s_w1[c * 25 + ky * 5 + kx];
                o00 = fmaf(w, p[ky][kx], o00);
                o01 = fmaf(w, p[ky][kx + 1], o01);
                o10 = fmaf(w, p[ky + 1][kx], o10);
                o11 = fmaf(w, p[ky + 1][kx + 1], o11);
            }
        s_p1[((y + 2) * LM_P1_W + x + 2) * LM_P1_C + c] = (_Float16)fmaxf(fmaxf(fmaxf(o00, o01), fmaxf(o10, o11)), 0.f);
    }
    __syncthreads();
    // the image is no longer needed: its room takes fc2's weights (read first behind the barriers of conv2 and fc1)
    for (int i = tid; i < LM_EC * 32; i += LM_THREADS) s_fc2[i] = (i & 31) < C ? a.fc2t[(i >> 5) * C + (i & 31)] : 0.f;

    // ---- what a thread keeps across the pass loop -----------------------------------------------------------------------------------
    const int lg = lane >> 4, ln = lane & 15;
    int pbase[4];      // wave = pooling window: position tile mt, column ln
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int s = min(mt * 16 + ln, 48);
        pbase[mt] = (((wave >> 1) * 7 + s / 7) * LM_P1_W + (wave & 1) * 7 + s % 7) * LM_P1_C;
    }
    float bias2[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bias2[r] = a.b2[lg * 4 + r];
        bias2[4 + r] = lg == 0 ? a.b2[16 + r] : 0.f;
    }
    const int j1 = min(tid, LM_EC - 1);
    float w_fc1[LM_EB];
#pragma unroll
    for (int k = 0; k < LM_EB; ++k) w_fc1[k] = a.fc1t[k * LM_EC + j1];
    const float b_fc1 = a.fb1[j1];
    const float b_fc2 = a.fb2[min(lane, C - 1)];
    LmSums sums = {0.0, 0.0, 0.0};      // wave 3's

    if (onA) {
        // ---- conv2(d) | barrier | fc1(d) beside fc2(d - 1) | barrier ----------------------------------------------------------------
        for (int i = 0; i < n_p; ++i) {
            const int d = d0 + i, p = i & 1;
            const uint32_t* bits = s_bits[(m0 + d) % M];
            lm_u32x4 pat[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) pat[j] = lm_pattern((bits[0] >> (8 * ((lg + j) % 3))) & 0xFFu);
            float v[8];
            lm_conv2(s_p1, s_w2, s_koff, pbase, lane, pat, bias2, v);
            lm_store_features(s_fM[p], v, lane, wave, onB ? bits + LM_WB : nullptr);
            __syncthreads();
            if (tid < LM_EC) {
                const float h = lm_fc1(s_fM[p], w_fc1, b_fc1);
                s_hM[p][tid] = (!onC || lm_bit(bits + LM_WC, tid)) ? h : 0.f;
            } else if (wave == 3 && i > 0) {
                lm_fc2(s_hM[p ^ 1], nullptr, s_fc2, b_fc2, lane, C, d - 1, M, a, b, sums);
            }
            __syncthreads();
        }
        if (wave == 3 && n_p > 0) lm_fc2(s_hM[(n_p - 1) & 1], nullptr, s_fc2, b_fc2, lane, C, d0 + n_p - 1, M, a, b, sums);
    } else {
        // ---- conv2 once -----------------------------------------------------------------------------------------------------------
        const lm_u32x4 ones = {~0u, ~0u, ~0u, ~0u};
        const lm_u32x4 pat[3] = {ones, ones, ones};
        float v[8];
        lm_conv2(s_p1, s_w2, s_koff, pbase, lane, pat, bias2, v);
        lm_store_features(s_feat, v, lane, wave, nullptr);
        __syncthreads();
        if (onB) {
            // ---- fc1(d) beside the masked features of pass d + 1 (wave 2) and fc2(d - 1) (wave 3) | barrier --------------------------
            if (wave == 2 && n_p > 0) {
                const uint32_t* bits = s_bits[(m0 + d0) % M] + LM_WB;
                for (int j = lane; j < LM_EB; j += 64) s_fM[0][j] = lm_bit(bits, j) ? s_feat[j] : 0.f;
            }
            __syncthreads();
            for (int i = 0; i < n_p; ++i) {
                const int d = d0 + i, p = i & 1;
                if (tid < LM_EC) {
                    const float h = lm_fc1(s_fM[p], w_fc1, b_fc1);
                    s_hM[p][tid] = (!onC || lm_bit(s_bits[(m0 + d) % M] + LM_WC, tid)) ? h : 0.f;
                } else if (wave == 2) {
                    if (i + 1 < n_p) {
                        const uint32_t* bits = s_bits[(m0 + d + 1) % M] + LM_WB;
                        for (int j = lane; j < LM_EB; j += 64) s_fM[p ^ 1][j] = lm_bit(bits, j) ? s_feat[j] : 0.f;
                    }
                } else if (wave == 3 && i > 0) {
                    lm_fc2(s_hM[p ^ 1], nullptr, s_fc2, b_fc2, lane, C, d - 1, M, a, b, sums);
                }
                __syncthreads();
            }
            if (wave == 3 && n_p > 0) lm_fc2(s_hM[(n_p - 1) & 1], nullptr, s_fc2, b_fc2, lane, C, d0 + n_p - 1, M, a, b, sums);
        } else {
            // ---- site C alone: fc1 once, wave 3 masks the hidden units as it reads them ---------------------------------------------
            if (tid < LM_EC) s_hpre[tid] = lm_fc1(s_feat, w_fc1, b_fc1);
            __syncthreads();
            if (wave == 3)
                for (int i = 0; i < n_p; ++i)
                    lm_fc2(s_hpre, s_bits[(m0 + d0 + i) % M] + LM_WC, s_fc2, b_fc2, lane, C, d0 + i, M, a, b, sums);
        }
    }
    if (wave == 3 && lane < C && a.S1 && n_p > 0) {
        const size_t n = (size_t)a.B * C, i = (size_t)b * C + lane;
        if (a.n_chunks == 1) {
            a.S1[i] += sums.s1;
            a.S2[i] += sums.s2;
            a.SL[i] += sums.sl;
        } else {
            double* part = a.part + (size_t)blockIdx.y * 3 * n;
            part[i] = sums.s1;
            part[n + i] = sums.s2;
            part[2 * n + i] = sums.sl;
        }
    }
}

// S += the chunks' partials, in chunk order: [n_chunks][3][n]
__global__ __launch_bounds__(LM_THREADS) void lenet5_mask_join_kernel(const double* __restrict__ part, int n_chunks, size_t n, double* S1, double* S2,
                                                                      double* SL) {
    const size_t i = (size_t)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= 3 * n) return;
    const size_t m = i / n, r = i % n;
    double* S = m == 0 ? S1 : (m == 1 ? S2 : SL);
    double s = S[r];
    for (int ch = 0; ch < n_chunks; ++ch) s += part[((size_t)ch * 3 + m) * n + r];
    S[r] = s;
}

}  // namespace

// a.site[]: every site that is on is BMI_SITE_MASKSEMBLE with the same num_masks in [1, 32] and device masks (bmi_lenet5_create checks);
// at least one is on.  The chunks are those of lenet5_chunks(B, min(tc, M)).
int launch_lenet5_mask(Lenet5Args a, hipStream_t s) {
    if (a.B < 1 || a.tc < 1 || a.t0 < 0 || a.C < 2 || a.C > 32) return BMI_ERR_INVALID;
    int M = 0;
    for (const SiteArgs& st : a.site) {
        if (st.kind == BMI_SITE_NONE) continue;
        if (st.kind != BMI_SITE_MASKSEMBLE || !st.masks || st.num_masks < 1 || st.num_masks > LM_MAX_MASKS || (M && st.num_masks != M)) return BMI_ERR_INVALID;
        M = st.num_masks;
    }
    if (!M) return BMI_ERR_INVALID;
    a.n_chunks = lenet5_chunks(a.B, std::min(a.tc, M), &a.per_chunk);
    if (a.S1 && a.n_chunks > 1 && !a.part) return BMI_ERR_NOMEM;
    hipLaunchKernelGGL(lenet5_mask_kernel, dim3((unsigned)a.B, (unsigned)a.n_chunks), dim3(LM_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    if (a.S1 && a.n_chunks > 1) {
        const size_t n = (size_t)a.B * a.C;
        hipLaunchKernelGGL(lenet5_mask_join_kernel, dim3((unsigned)((3 * n + LM_THREADS - 1) / LM_THREADS)), dim3(LM_THREADS), 0, s, a.part, a.n_chunks, n,
                           a.S1, a.S2, a.SL);
        BMI_CHECK_LAUNCH();
    }
    return BMI_OK;
}
