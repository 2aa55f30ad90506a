// MC-dropout LeNet-5 (BASELINE config 1: 28x28x1 -> conv5x5x20 + ReLU + pool 2 -> conv5x5x20 + ReLU + pool 7 -> 80 -> 100 -> C) as ONE
// kernel: the network is 2.4 M MAC per image, so five launches with the activations in HBM would be launch- and latency-bound.  One
// workgroup owns one image: it computes the deterministic part once into LDS and loops over its Monte-Carlo samples inside the kernel,
// with the float64 moment sums in registers in sample order.  Replaces T forwards of the Keras model
// Hardware_Artifact/bayes_hw/models/models.py:34-73 (restated in oracle/extra_models.py:LeNet5MC) plus the softmax / averaging of
// FullAnalysis._get_output (SA/train/results_analyzer.py:236-248).
//
// Work split   grid.x = image, grid.y = sample chunk (lenet5_chunks: a pure function of (batch, t_count)), 256 threads = 4 waves.  No
//              workgroup waits on another; with more than one chunk the float64 partials go to the caller's scratch and
//              lenet5_join_kernel adds them onto S in chunk order (no floating-point atomics anywhere).
// Sites        A (on the pooled conv1 map, element ((b*14 + y)*14 + x)*20 + c), B (on the 80 features, b*80 + j), C (on the 100 hidden
//              units, b*100 + j): elementwise MC dropout under the convention of philox.h.  Everything in front of the first site that
//              is on runs once per workgroup; the rest runs per sample.
// Prefix       the fp32 image with a 2-pixel zero halo in LDS (32 x 32); conv1 + bias + ReLU + 2x2 max on the VALU in fp32 (one item =
//              one pooled position x channel, its 6 x 6 input patch in registers) -> P1, fp16 [18][18][24] in LDS: a 2-position zero
//              halo and 20 -> 24 channels (zero), so that eight consecutive K values never straddle a tap.
// Keep bits    per sample ONE Philox phase for all three sites, one call per item: a call of site A covers 64 elements at 2 bits per
//              element (16-bit p: 8) and may straddle the image's first / last element — the item writes only the 8-element groups
//              that lie inside the image (3920 = 8 * 490: a group never straddles); keep bytes land in LDS.
// Site A       P1m = the kept elements of P1, bit-exact (the 1/(1-p) is applied to conv2's fp32 accumulators instead: one rounding
//              less); P1 itself survives for the next sample.
// conv2        implicit GEMM on v_mfma_f32_16x16x32_f16, fp32 accumulate: K = 25 taps x 24 channels = 600 -> 19 K-steps (the last
//              quarter of the last step is zero weights); channels are the MFMA rows (20 -> 2 tiles of 16), positions the columns.  A
//              position tile is 16 of the 49 positions of ONE 7x7 pooling window (4 tiles, the last one repeats position 48: a
//              duplicate cannot change a maximum), and wave q owns window q: 16 tiles where a row-major walk would need 13, but the
//              longest wave has 4 tiles either way, and bias + ReLU + the 7x7 max stay inside the wave — registers over its four
//              tiles, then four xor-shuffles over the 16 positions of a tile.  Dead share of the MFMA work: 1 - 196*20*500 /
//              (16*16 * 32 * 608) = 60.6 % (13 row tiles: 51.6 %; 32-channel padding, one tap per K-step: 25 K-steps, 70.0 %).
//              Operand fragments are single 16-byte LDS reads: pixels gathered from the haloed map ((y + ky)*18 + x + kx)*24 + 8 cg,
//              weights from the host's [76 K-groups][20 channels][8] fp16 layout.  No im2col buffer.
// fc1          fp32, one FMA chain per output in ascending k starting from the bias, thread j = output j; its 80 weights stay in
//              registers for the whole sample loop (32 KB of LDS would leave one workgroup per CU).
// fc2 + softmax  wave 0, lane c = class c: fp32 chain over the 100 hidden units (weights [100][32] in LDS), max-subtracted softmax by
//              wave shuffles, S1 += p, S2 += p * p, SL += logit in float64 registers; the other waves already draw the next sample.
// LDS          P1 15 552 + P1m 15 552 (the image and conv1's weights live there during the prefix) + conv2 weights 24 320 + fc2
//              12 800 + keep bytes, features, hidden units, offsets 2 272 = 70 496 bytes: two workgroups per CU.
#include <algorithm>
#include <new>

#include "kernels.h"

namespace {

typedef _Float16 ln_half8 __attribute__((ext_vector_type(8)));
typedef float ln_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LN_THREADS = 256;
constexpr int LN_P1_W = 18, LN_P1_C = 24, LN_P1_HALVES = LN_P1_W * LN_P1_W * LN_P1_C;     // 7776
constexpr int LN_KG = 76, LN_KSTEPS = 19;       // K-groups of 8 (75 live), K-steps of 32
constexpr int LN_EA = 3920, LN_EB = 80, LN_EC = 100;      // elements per image of the three sites

// keep flag of element `bit` (counted from the first keep byte) of a site's keep bytes
__device__ __forceinline__ bool ln_kept(const uint8_t* keep, int bit) { return (keep[bit >> 3] >> (bit & 7)) & 1; }

// conv2 + bias + ReLU + 7x7 max of pooling window `wave` from the haloed map `src`; the lanes with (lane & 15) == 0 return their channels'
// maxima in v[]: v[r] = channel 4 * (lane >> 4) + r, v[4 + r] = channel 16 + r (lanes 0..15 only)
__device__ __forceinline__ void ln_conv2(const _Float16* src, const _Float16* s_w2, const int* s_koff, const int pbase[4], int lane, float scale,
                                         const float bias[8], float v[8]) {
    const int lg = lane >> 4, ln = lane & 15;
    ln_f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = ln_f32x4{0.f, 0.f, 0.f, 0.f};
    const ln_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < LN_KSTEPS; ++ks) {
        const int kg = ks * 4 + lg;
        const int koff = s_koff[kg];
        const ln_half8 w0 = *(const ln_half8*)(s_w2 + (kg * 20 + ln) * 8);
        const ln_half8 w1 = ln < 4 ? *(const ln_half8*)(s_w2 + (kg * 20 + 16 + ln) * 8) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const ln_half8 px = *(const ln_half8*)(src + pbase[mt] + koff);
            acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, px, acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, px, acc[mt][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = fmaxf(fmaxf(acc[0][nt][r], acc[1][nt][r]), fmaxf(acc[2][nt][r], acc[3][nt][r]));
            m = fmaxf(fmaf(m, scale, bias[nt * 4 + r]), 0.f);      // scale > 0: the maximum commutes with scale, bias and ReLU
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
            v[nt * 4 + r] = m;
        }
}

__global__ __launch_bounds__(LN_THREADS, 2) void lenet5_kernel(Lenet5Args a) {
    __shared__ __attribute__((aligned(16))) _Float16 s_p1[LN_P1_HALVES];
    __shared__ __attribute__((aligned(16))) _Float16 s_p1m[LN_P1_HALVES];      // prefix: the haloed image and conv1's weights
    __shared__ __attribute__((aligned(16))) _Float16 s_w2[LN_KG * 20 * 8];
    __shared__ float s_fc2[LN_EC * 32];
    __shared__ int s_koff[LN_KG];
    __shared__ float s_feat[LN_EB], s_featM[LN_EB], s_hpre[LN_EC], s_hM[LN_EC];
    __shared__ uint8_t s_keepA[LN_EA / 8 + 6], s_keepB[16], s_keepC[16];
    float* const s_img = (float*)s_p1m;       // [32][32]
    float* const s_w1 = s_img + 1024;         // [20][25] then the 20 biases

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C;
    const int it0 = (int)blockIdx.y * a.per_chunk;
    const int n_t = min(a.per_chunk, a.tc - it0);
    const SiteArgs& sA = a.site[0];
    const SiteArgs& sB = a.site[1];
    const SiteArgs& sC = a.site[2];
    const bool onA = sA.kind != BMI_SITE_NONE, onB = sB.kind != BMI_SITE_NONE, onC = sC.kind != BMI_SITE_NONE;

    // ---- prefix: staging ----------------------------------------------------------------------------------------------------------
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += LN_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? img[r * 28 + c] : 0.f;
    }
    for (int i = tid; i < 520; i += LN_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < LN_P1_HALVES / 8; i += LN_THREADS) ((uint4*)s_p1)[i] = uint4{0u, 0u, 0u, 0u};
    for (int i = tid; i < LN_KG * 20; i += LN_THREADS) ((uint4*)s_w2)[i] = ((const uint4*)a.w2f)[i];
    for (int i = tid; i < LN_EC * 32; i += LN_THREADS) s_fc2[i] = (i & 31) < C ? a.fc2t[(i >> 5) * C + (i & 31)] : 0.f;
    if (tid < LN_KG) {      // K-group -> offset of its tap and channel group inside the haloed map (group 75: zero weights, any valid offset)
        const int kg = min(tid, LN_KG - 2), tap = kg / 3;
        s_koff[tid] = ((tap / 5) * LN_P1_W + tap % 5) * LN_P1_C + (kg % 3) * 8;
    }
    __syncthreads();

    // ---- prefix: conv1 + bias + ReLU + 2x2 max -> P1 -------------------------------------------------------------------------------
    for (int i = tid; i < LN_EA; i += LN_THREADS) {
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
        s_p1[((y + 2) * LN_P1_W + x + 2) * LN_P1_C + c] = (_Float16)fmaxf(fmaxf(fmaxf(o00, o01), fmaxf(o10, o11)), 0.f);
    }
    __syncthreads();
    if (onA) {      // the image is no longer needed: its room becomes P1m, whose halo and padding channels stay zero
        for (int i = tid; i < LN_P1_HALVES / 8; i += LN_THREADS) ((uint4*)s_p1m)[i] = uint4{0u, 0u, 0u, 0u};
        __syncthreads();
    }

    // ---- what a thread keeps across the sample loop ---------------------------------------------------------------------------------
    const int lg = lane >> 4, ln = lane & 15;
    int pbase[4];      // wave = pooling window: position tile mt, column ln
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int s = min(mt * 16 + ln, 48);
        pbase[mt] = (((wave >> 1) * 7 + s / 7) * LN_P1_W + (wave & 1) * 7 + s % 7) * LN_P1_C;
    }
    float bias2[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bias2[r] = a.b2[lg * 4 + r];
        bias2[4 + r] = lg == 0 ? a.b2[16 + r] : 0.f;
    }
    const int j1 = min(tid, LN_EC - 1);
    float w_fc1[LN_EB];
#pragma unroll
    for (int k = 0; k < LN_EB; ++k) w_fc1[k] = a.fc1t[k * LN_EC + j1];
    const float b_fc1 = a.fb1[j1];
    const float b_fc2 = a.fb2[min(lane, C - 1)];
    const uint64_t eA0 = (uint64_t)(a.b0 + b) * LN_EA, eB0 = (uint64_t)(a.b0 + b) * LN_EB, eC = (uint64_t)(a.b0 + b) * LN_EC;
    const uint64_t eC0 = eC & ~7ull;          // 100 is a multiple of 4 only: the image's first keep byte starts up to 4 elements early
    const int offC = (int)(eC - eC0);
    const int shA = 7 - sA.log2_bits;         // log2 of the elements per Philox call
    const uint64_t cA0 = eA0 >> shA;
    const int nA = onA ? (int)(((eA0 + LN_EA - 1) >> shA) - cA0) + 1 : 0, nB = onB ? LN_EB / 8 : 0, nC = onC ? (offC + LN_EC + 7) / 8 : 0;
    double s1 = 0.0, s2 = 0.0, sl = 0.0;

    for (int it = 0; it < n_t; ++it) {
        const uint32_t t = (uint32_t)(a.t0 + it0 + it);
        const bool first = it == 0;
        // ---- the sample's keep bits, all sites, one Philox call per item ------------------------------------------------------------
        if (nA + nB + nC) {
            for (int i = tid; i < nA + nB + nC; i += LN_THREADS) {
                if (i < nA) {
                    const uint64_t e_call = (cA0 + (uint64_t)i) << shA;
                    const philox4 r = philox_site_call(sA, e_call, t);
                    for (int g = 0; g < (1 << (shA - 3)); ++g) {
                        const uint64_t e0 = e_call + 8u * g;
                        if (e0 >= eA0 && e0 < eA0 + LN_EA) s_keepA[(int)(e0 - eA0) >> 3] = sA.drop_all ? (uint8_t)0 : (uint8_t)philox_keep8(r, (uint32_t)e0, sA.log2_bits, sA.thresh);
                    }
                } else if (i < nA + nB) {
                    s_keepB[i - nA] = (uint8_t)site_keep8(sB, eB0 + 8u * (i - nA), t);
                } else {
                    s_keepC[i - nA - nB] = (uint8_t)site_keep8(sC, eC0 + 8u * (i - nA - nB), t);
                }
            }
            __syncthreads();
        }
        // ---- site A, conv2, pool 7 -> the 80 features (once when site A is off) -----------------------------------------------------
        if (first || onA) {
            const _Float16* src = s_p1;
            if (onA) {
                for (int i = tid; i < 196 * 5; i += LN_THREADS) {      // four channels of one position: one nibble of a keep byte
                    const int pos = i / 5, qd = i % 5, e = pos * 20 + qd * 4;
                    const uint32_t nib = (uint32_t)s_keepA[e >> 3] >> (e & 4);
                    const int off = ((pos / 14 + 2) * LN_P1_W + pos % 14 + 2) * LN_P1_C + qd * 4;
                    uint2 v = *(const uint2*)(s_p1 + off);
                    v.x &= ((nib & 1u) ? 0xFFFFu : 0u) | ((nib & 2u) ? 0xFFFF0000u : 0u);
                    v.y &= ((nib & 4u) ? 0xFFFFu : 0u) | ((nib & 8u) ? 0xFFFF0000u : 0u);
                    *(uint2*)(s_p1m + off) = v;
                }
                __syncthreads();
                src = s_p1m;
            }
            float v[8];
            ln_conv2(src, s_w2, s_koff, pbase, lane, sA.scale, bias2, v);
            if (ln == 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r >= 4 && lg != 0) break;
                    const int j = (r < 4 ? lg * 4 + r : 12 + r) * 4 + wave;      // torch's flatten: channel * 4 + window
                    s_feat[j] = v[r];
                    if (onB) s_featM[j] = ln_kept(s_keepB, j) ? v[r] * sB.scale : 0.f;
                }
            }
            __syncthreads();
        } else if (onB) {
            if (tid < LN_EB) s_featM[tid] = ln_kept(s_keepB, tid) ? s_feat[tid] * sB.scale : 0.f;
            __syncthreads();
        }
        // ---- site B's features -> fc1 + ReLU -> site C (once when sites A and B are off) ---------------------------------------------
        if (first || onA || onB) {
            if (wave < 2 && tid < LN_EC) {
                const float* f = onB ? s_featM : s_feat;
                float h = b_fc1;
#pragma unroll
                for (int k = 0; k < LN_EB; ++k) h = fmaf(f[k], w_fc1[k], h);
                h = fmaxf(h, 0.f);
                s_hpre[tid] = h;
                if (onC) s_hM[tid] = ln_kept(s_keepC, offC + tid) ? h * sC.scale : 0.f;
            }
            __syncthreads();
        } else if (onC) {
            if (tid < LN_EC) s_hM[tid] = ln_kept(s_keepC, offC + tid) ? s_hpre[tid] * sC.scale : 0.f;
            __syncthreads();
        }
        // ---- fc2, softmax, moment sums: wave 0, lane = class (the next barrier this wave meets is behind its reads of the hidden units) --
        if (wave == 0) {
            const float* h = onC ? s_hM : s_hpre;
            float z = b_fc2;
#pragma unroll 4
            for (int k = 0; k < LN_EC; ++k) z = fmaf(h[k], s_fc2[k * 32 + (lane & 31)], z);
            float m = lane < C ? z : -INFINITY;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            const float e = lane < C ? expf(z - m) : 0.f;
            float sum = e;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
            if (lane < C) {
                const double p = (double)(e / sum);
                s1 += p;
                s2 += p * p;
                sl += (double)z;
                if (a.logits) a.logits[((size_t)(it0 + it) * a.B + b) * C + lane] = z;
            }
        }
    }
    if (wave == 0 && lane < C && a.S1 && n_t > 0) {
        const size_t n = (size_t)a.B * C, i = (size_t)b * C + lane;
        if (a.n_chunks == 1) {
            a.S1[i] += s1;
            a.S2[i] += s2;
            a.SL[i] += sl;
        } else {
            double* part = a.part + (size_t)blockIdx.y * 3 * n;
            part[i] = s1;
            part[n + i] = s2;
            part[2 * n + i] = sl;
        }
    }
}

// S += the chunks' partials, in chunk order: [n_chunks][3][n]
__global__ __launch_bounds__(LN_THREADS) void lenet5_join_kernel(const double* __restrict__ part, int n_chunks, size_t n, double* S1, double* S2,
                                                                 double* SL) {
    const size_t i = (size_t)blockIdx.x * LN_THREADS + threadIdx.x;
    if (i >= 3 * n) return;
    const size_t m = i / n, r = i % n;
    double* S = m == 0 ? S1 : (m == 1 ? S2 : SL);
    double s = S[r];
    for (int ch = 0; ch < n_chunks; ++ch) s += part[((size_t)ch * 3 + m) * n + r];
    S[r] = s;
}

}  // namespace

// Sample chunks of a call: enough workgroups for two per CU of a 256-CU device at small batches, never more than the samples; a pure
// function of (batch, t_count).  want = min(t_count, max(1, 512 / batch)) is an upper bound: the samples per chunk are rounded up and the
// count follows from them (t_count = 10, want = 4: chunks of 3, 3, 3, 1; want = 6: five chunks of 2).  *per_chunk = samples per chunk.
int lenet5_chunks(int batch, int t_count, int* per_chunk) {
    const int want = std::min(t_count, std::max(1, 512 / batch));
    const int per = (t_count + want - 1) / want;
    if (per_chunk) *per_chunk = per;
    return (t_count + per - 1) / per;
}

int launch_lenet5(Lenet5Args a, hipStream_t s) {
    if (a.B < 1 || a.tc < 1 || a.C < 2 || a.C > 32) return BMI_ERR_INVALID;
    a.n_chunks = lenet5_chunks(a.B, a.tc, &a.per_chunk);
    if (a.S1 && a.n_chunks > 1 && !a.part) return BMI_ERR_NOMEM;
    hipLaunchKernelGGL(lenet5_kernel, dim3((unsigned)a.B, (unsigned)a.n_chunks), dim3(LN_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    if (a.S1 && a.n_chunks > 1) {
        const size_t n = (size_t)a.B * a.C;
        hipLaunchKernelGGL(lenet5_join_kernel, dim3((unsigned)((3 * n + LN_THREADS - 1) / LN_THREADS)), dim3(LN_THREADS), 0, s, a.part, a.n_chunks, n,
                           a.S1, a.S2, a.SL);
        BMI_CHECK_LAUNCH();
    }
    return BMI_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
struct bmi_lenet5_s {
    Lenet5Args args;
    bmi_site sites[3];
    size_t partials_bytes;
    int num_masks;      // > 0: the sites that are on are Masksembles sites of this many masks (lenet5_mask.hip)
};

extern "C" {

int bmi_lenet5_create(const bmi_lenet5_desc* d, bmi_lenet5_handle* out) {
    if (!d || !out) return BMI_ERR_INVALID;
    if (!d->conv1_w || !d->conv1_b || !d->conv2_w_frag || !d->conv2_b || !d->fc1_wt || !d->fc1_b || !d->fc2_wt || !d->fc2_b) return BMI_ERR_INVALID;
    if (d->out_dim < 2 || d->out_dim > 32) return BMI_ERR_UNSUPPORTED;
    int n_mc = 0, num_masks = 0;
    for (const bmi_site& st : d->sites) {
        if (st.kind == BMI_SITE_NONE) continue;
        if (st.kind == BMI_SITE_MASKSEMBLE) {      // (host-only: `masks` is never read here)
            if (!st.masks || st.num_masks < 1) return BMI_ERR_INVALID;
            if (st.num_masks > 32 || (num_masks && st.num_masks != num_masks)) return BMI_ERR_UNSUPPORTED;
            num_masks = st.num_masks;
            continue;
        }
        if (st.kind != BMI_SITE_ELEMENTWISE) return st.kind == BMI_SITE_CHANNEL ? BMI_ERR_UNSUPPORTED : BMI_ERR_INVALID;
        if (!(st.p >= 0.f && st.p < 1.f) || st.site_id < 0) return BMI_ERR_INVALID;      // (a NaN fails the comparison)
        ++n_mc;
    }
    if (n_mc && num_masks) return BMI_ERR_UNSUPPORTED;      // all MC dropout or all Masksembles, as the reference's global dropout_type
    if (d->partials_bytes && !d->partials) return BMI_ERR_INVALID;
    bmi_lenet5_s* h = new (std::nothrow) bmi_lenet5_s();
    if (!h) return BMI_ERR_NOMEM;
    Lenet5Args& a = h->args;
    a.w1 = d->conv1_w; a.b1 = d->conv1_b; a.w2f = (const _Float16*)d->conv2_w_frag; a.b2 = d->conv2_b;
    a.fc1t = d->fc1_wt; a.fb1 = d->fc1_b; a.fc2t = d->fc2_wt; a.fb2 = d->fc2_b;
    a.C = d->out_dim;
    a.part = (double*)d->partials;
    for (int i = 0; i < 3; ++i) h->sites[i] = d->sites[i];
    h->partials_bytes = d->partials_bytes;
    h->num_masks = num_masks;
    *out = h;
    return BMI_OK;
}

int bmi_lenet5_destroy(bmi_lenet5_handle h) {
    delete h;
    return BMI_OK;
}

int bmi_lenet5_forward_mcd(bmi_lenet5_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed, double* S1,
                           double* S2, double* SL, float* logits, bmi_stream stream) {
    if (!h || !x_nchw || batch < 1 || t_count < 1 || t_begin < 0) return BMI_ERR_INVALID;
    const bool sums = S1 || S2 || SL;
    if ((sums && !(S1 && S2 && SL)) || (!sums && !logits)) return BMI_ERR_INVALID;
    Lenet5Args a = h->args;
    const int chunks = lenet5_chunks(batch, h->num_masks ? std::min(t_count, h->num_masks) : t_count, nullptr);      // Masksembles: one pass per distinct mask
    if (sums && chunks > 1 && (size_t)chunks * 3 * batch * a.C * sizeof(double) > h->partials_bytes) return BMI_ERR_NOMEM;
    a.x = x_nchw; a.B = batch; a.b0 = 0; a.t0 = t_begin; a.tc = t_count;
    a.S1 = S1; a.S2 = S2; a.SL = SL; a.logits = logits;
    for (int i = 0; i < 3; ++i) a.site[i] = resolve_site(h->sites[i].kind == BMI_SITE_NONE ? nullptr : &h->sites[i], seed, 0);
    return h->num_masks ? launch_lenet5_mask(a, (hipStream_t)stream) : launch_lenet5(a, (hipStream_t)stream);
}

}  // extern "C"
