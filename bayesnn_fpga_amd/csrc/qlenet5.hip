// The QUANTISED MC-dropout LeNet-5 of the reference's hardware flow as ONE kernel: T_Qlenet_bayes
// (Hardware_Artifact/bayes_hw/models/t_qmodels_bayes.py:38-96 with qmodels.py:60 and s_qmodels_bayes.py:36), the network of lenet5.hip with
// every kernel and bias through quantized_bits(W, I, alpha = 1) and every activation through quantized_relu(W) (train_qkeras.py:204-205:
// W = 6, I = 0).  Operands of at most 8 bits and power-of-two scales: every multiply-accumulate is an exact integer, conv2 runs on
// v_mfma_i32_16x16x64_i8, the dense layers on v_dot4_i32_i8, and a plain integer loop on the host reproduces the fp32 logits bit for bit.
//
// Arithmetic   (the contract; W = quant_tbit in [2, 8], I = quant_ibit in [0, W-1], F = W-1-I, rne = round half to even)
//              weight / bias code q = clip(rne(w * 2^F), -2^(W-1), 2^(W-1) - 1), value q * 2^-F: quantised by the HOST, the kernel reads codes;
//              activation code a = clip(rne(v * 2^W), 0, 2^W - 1), value a * 2^-W; input x8 = clip(rne(x * 2^8), 0, 255), value x8 * 2^-8.
//              conv1: acc = sum x8 * q1 over the 25 taps, pre = acc + (b1 << 8), a1 = clip(rne(pre / 2^(7-I)), 0, 2^W - 1) on integers, then
//              the 2x2 max on codes.  conv2, fc1, fc2: acc = sum keep * a * q in int32 (a dropped element adds 0; at most 500 * 255 * 128
//              < 2^24, so float(acc) is exact), y = fadd_rn(fmul_rn(float(acc) * 2^-(W+F), d), b * 2^-F): two rounded operations, never one
//              FMA (this file is compiled with fp contraction off); d = fl32(1 / fl32(1 - p)) of the site in front of the layer, 1 where it is
//              off.  conv2 and fc1 end in a = clip(rintf(y * 2^W), 0, 2^W - 1), conv2 then in the 7x7 max on codes; fc2's y is the logit.
//              Every step from acc to a is non-decreasing, so both maxima are taken on the raw integers and one position is finished.
// Signed operands  the MFMA and the dot instruction take SIGNED bytes and at W = 8 a code reaches 255.  Every activation byte, from P1 to the
//              hidden units, is stored as a - 128 (a ^ 0x80); the halo and a dropped element are -128, i.e. code 0.  sum (a - 128) * q misses
//              128 * sum q over the layer's whole K, a constant per output that each thread adds to its integer sum (computed once per
//              workgroup from the weights it holds).  Exact in int32 (|.| <= 500 * 128 * 128), one path for every W, and dropping stays a
//              byte select.  Splitting a into two 7-bit halves would double conv2's MFMA work for the one W that needs it.
// Work split   lenet5.hip's: grid.x = image, grid.y = sample chunk (lenet5_chunks), 256 threads = 4 waves, wave q = pooling window q, a
//              restated join launch for the chunks' float64 partials.  Sites A, B, C, their element numbering, the one Philox phase per
//              sample and everything in front of the first active site running once per workgroup are lenet5.hip's as well.
// Prefix       x8 as int with a 2-pixel zero halo (32 x 32) and conv1's codes in LDS; conv1 on the VALU in int32 (one item = one pooled
//              position x channel) -> P1, i8 [18][18][32] in LDS: a 2-position halo of -128, 32 bytes per position (20 live channels) so that
//              16-byte fragment reads stay aligned.  10 368 bytes where the fp16 map takes 15 552.
// conv2        implicit GEMM, K = 500 split 16 + 4 channels.  Main part: 25 taps x channels 0..15, a 16-byte fragment = 16 channels of one
//              tap, lane group g of K-step s reads tap 4 s + g: 7 K-steps (taps 25..27: zero weights).  Tail: channels 16..19, a fragment =
//              4 taps x 4 channels gathered by four 4-byte reads at byte 16 of a position: 2 K-steps (32 tap slots, 25 live).  9 K-steps of 64
//              against 13 with the channels padded to 32; 72 MFMAs per wave and sample where lenet5_kernel issues 152.  Rows = output
//              channels (20 -> 2 tiles of 16), columns = 16 of the 49 positions of the wave's window (4 tiles, the last repeats position 48).
//              Dead share of the MFMA multiply-adds: 1 - 196*20*500 / (16*16 * 32 * 576) = 58.5 % (32-channel padding: 13 K-steps, 71.2 %;
//              flat 500 -> 512 with byte gathers: 8 K-steps, 53.3 %, but every fragment would be sixteen 1-byte reads).
// fc1          thread j = output j, its 80 weight bytes in 20 registers for the whole sample loop, 20 v_dot4_i32_i8 over the feature bytes.
// fc2 + softmax  wave 0, lane c = class c: 25 v_dot4_i32_i8 (weights [25][32] dwords in LDS), then lenet5_kernel's softmax and float64 sums.
// LDS          P1 10 368 + P1m 10 368 (the image and conv1's codes live there during the prefix) + conv2 fragments 11 520 + fc2 3 200 +
//              offsets, corrections, features, hidden units, keep bytes 1 232 = 36 688 bytes; 146 VGPRs: three workgroups per CU.
#include <algorithm>
#include <new>

#include "kernels.h"

#pragma clang fp contract(off)

struct QLenet5Args {
    const float* x;          // fp32 [B][1][28][28]
    const int8_t* w1;        // conv1 codes [20][25]
    const int8_t* b1;
    const int8_t* w2f;       // conv2 codes [36 groups][20 channels][16] (include/bayesnn_fpga_amd.h: conv2_q_frag)
    const int8_t* b2;
    const int8_t* fc1;       // fc1 codes [100][80]
    const int8_t* fb1;
    const int8_t* fc2;       // fc2 codes [C][100]
    const int8_t* fb2;
    int W, I;                // quant_tbit, quant_ibit
    int B, C, b0;            // images of the call, classes, index of image 0 in the sites' element spaces
    int t0, tc;              // first sample, samples
    int n_chunks, per_chunk; // filled by launch_qlenet5 from lenet5_chunks(B, tc)
    SiteArgs site[3];        // A, B, C (kind BMI_SITE_NONE: off)
    double* S1;              // float64 [B][C] sums, ADDED to; all three null: logits only
    double* S2;
    double* SL;
    double* part;            // float64 [n_chunks][3][B][C] scratch, read only when n_chunks > 1
    float* logits;           // fp32 [tc][B][C] or null
};

namespace {

typedef int ql_i32x4 __attribute__((ext_vector_type(4)));

constexpr int QL_THREADS = 256;
constexpr int QL_P1_W = 18, QL_P1_C = 32, QL_P1_BYTES = QL_P1_W * QL_P1_W * QL_P1_C;      // 10368
constexpr int QL_KG_MAIN = 28, QL_KG = 36, QL_KS_MAIN = 7, QL_KS = 9;      // 16-byte K-groups (25 + 7 live), K-steps of 64
constexpr int QL_EA = 3920, QL_EB = 80, QL_EC = 100;      // elements per image of the three sites
constexpr uint32_t QL_OFF = 0x80808080u;                  // four activation bytes of code 0

__device__ __forceinline__ bool ql_kept(const uint8_t* keep, int bit) { return (keep[bit >> 3] >> (bit & 7)) & 1; }

// rne(v / 2^sh) on integers, sh in [0, 7]
__device__ __forceinline__ int ql_rne_shift(int v, int sh) {
    const int q = v >> sh, rem = v & ((1 << sh) - 1), half = (1 << sh) >> 1;
    return q + ((rem > half || (sh > 0 && rem == half && (q & 1))) ? 1 : 0);
}

// y = fadd_rn(fmul_rn(float(acc) * 2^-(W+F), d), bias): the power-of-two product is exact, the other two operations round (contraction is off)
__device__ __forceinline__ float ql_affine(int acc, float s_acc, float d, float bias) {
    const float prod = ((float)acc * s_acc) * d;
    return prod + bias;
}

// the stored byte (code ^ 0x80) of a = clip(rintf(y * 2^W), 0, 2^W - 1)
__device__ __forceinline__ uint8_t ql_act_byte(float y, float s_w, float a_max) { return (uint8_t)((int)fminf(fmaxf(rintf(y * s_w), 0.f), a_max) ^ 0x80); }

// raw conv2 sums, maximum over pooling window `wave`, from the haloed map `src`; the lanes with (lane & 15) == 0 return their channels' maxima
// in v[]: v[r] = channel 4 * (lane >> 4) + r, v[4 + r] = channel 16 + r (lanes 0..15 only).  The sums are over a - 128: the caller adds 128 * sum q.
__device__ __forceinline__ void ql_conv2(const int8_t* src, const int8_t* s_w2, const int* s_koff, const int pbase[4], int lane, int v[8]) {
    const int lg = lane >> 4, ln = lane & 15;
    ql_i32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = ql_i32x4{0, 0, 0, 0};
    const ql_i32x4 zero = {0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < QL_KS_MAIN; ++ks) {      // channels 0..15: one 16-byte read per fragment
        const int kg = ks * 4 + lg;
        const int koff = s_koff[kg];
        const ql_i32x4 w0 = *(const ql_i32x4*)(s_w2 + (kg * 20 + ln) * 16);
        const ql_i32x4 w1 = ln < 4 ? *(const ql_i32x4*)(s_w2 + (kg * 20 + 16 + ln) * 16) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const ql_i32x4 px = *(const ql_i32x4*)(src + pbase[mt] + koff);
            acc[mt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, px, acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, px, acc[mt][1], 0, 0, 0);
        }
    }
#pragma unroll 1
    for (int ks = QL_KS_MAIN; ks < QL_KS; ++ks) {      // channels 16..19: four taps per fragment, four 4-byte reads
        const int kg = ks * 4 + lg;
        const ql_i32x4 koff = *(const ql_i32x4*)(s_koff + QL_KG_MAIN + (kg - QL_KG_MAIN) * 4);
        const ql_i32x4 w0 = *(const ql_i32x4*)(s_w2 + (kg * 20 + ln) * 16);
        const ql_i32x4 w1 = ln < 4 ? *(const ql_i32x4*)(s_w2 + (kg * 20 + 16 + ln) * 16) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int8_t* p = src + pbase[mt];
            const ql_i32x4 px = {*(const int*)(p + koff[0]), *(const int*)(p + koff[1]), *(const int*)(p + koff[2]), *(const int*)(p + koff[3])};
            acc[mt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, px, acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, px, acc[mt][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int m = max(max(acc[0][nt][r], acc[1][nt][r]), max(acc[2][nt][r], acc[3][nt][r]));
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) m = max(m, __shfl_xor(m, off));
            v[nt * 4 + r] = m;
        }
}

// (three waves per SIMD: at four the allocator spills 12 VGPRs to scratch)
__global__ __launch_bounds__(QL_THREADS, 3) void qlenet5_kernel(QLenet5Args a) {
    __shared__ __attribute__((aligned(16))) int8_t s_p1[QL_P1_BYTES];
    __shared__ __attribute__((aligned(16))) int8_t s_p1m[QL_P1_BYTES];      // prefix: the haloed image and conv1's codes
    __shared__ __attribute__((aligned(16))) int8_t s_w2[QL_KG * 20 * 16];
    __shared__ uint32_t s_fc2[25 * 32];                                     // [k / 4][class]: four codes of one class
    __shared__ __attribute__((aligned(16))) int s_koff[QL_KG_MAIN + 32];
    __shared__ int s_corr2[20];
    __shared__ uint32_t s_feat[QL_EB / 4], s_featM[QL_EB / 4], s_hpre[QL_EC / 4], s_hM[QL_EC / 4];
    __shared__ uint8_t s_keepA[QL_EA / 8 + 6], s_keepB[16], s_keepC[16];
    int* const s_img = (int*)s_p1m;           // [32][32]
    int* const s_w1 = s_img + 1024;           // [20][25] then the 20 biases

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C;
    const int it0 = (int)blockIdx.y * a.per_chunk;
    const int n_t = min(a.per_chunk, a.tc - it0);
    const SiteArgs& sA = a.site[0];
    const SiteArgs& sB = a.site[1];
    const SiteArgs& sC = a.site[2];
    const bool onA = sA.kind != BMI_SITE_NONE, onB = sB.kind != BMI_SITE_NONE, onC = sC.kind != BMI_SITE_NONE;
    const int F = a.W - 1 - a.I;
    const float s_acc = ldexpf(1.f, -(a.W + F)), s_bias = ldexpf(1.f, -F), s_w = (float)(1 << a.W), a_max = (float)((1 << a.W) - 1);

    // ---- prefix: staging ----------------------------------------------------------------------------------------------------------
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += QL_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? (int)fminf(fmaxf(rintf(img[r * 28 + c] * 256.f), 0.f), 255.f) : 0;
    }
    for (int i = tid; i < 520; i += QL_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < QL_P1_BYTES / 16; i += QL_THREADS) ((uint4*)s_p1)[i] = uint4{QL_OFF, QL_OFF, QL_OFF, QL_OFF};
    for (int i = tid; i < QL_KG * 20; i += QL_THREADS) ((uint4*)s_w2)[i] = ((const uint4*)a.w2f)[i];
    for (int i = tid; i < 25 * 32; i += QL_THREADS) s_fc2[i] = (i & 31) < C ? *(const uint32_t*)(a.fc2 + (i & 31) * QL_EC + (i >> 5) * 4) : 0u;
    if (tid < QL_KG_MAIN + 32) {      // K-group -> byte offset of its tap inside the haloed map (taps >= 25: zero weights, any valid offset)
        const int tap = min(tid < QL_KG_MAIN ? tid : tid - QL_KG_MAIN, 24);
        s_koff[tid] = ((tap / 5) * QL_P1_W + tap % 5) * QL_P1_C + (tid < QL_KG_MAIN ? 0 : 16);
    }
    __syncthreads();

    // ---- prefix: 128 * sum q of conv2's channels; conv1 + bias + 2x2 max + quantised ReLU -> P1 ---------------------------------------
    if (tid < 20) {
        int s = 0;
        for (int g = 0; g < QL_KG * 4; ++g) s = __builtin_amdgcn_sdot4(*(const int*)(s_w2 + ((g >> 2) * 20 + tid) * 16 + (g & 3) * 4), 0x01010101, s, false);
        s_corr2[tid] = 128 * s;
    }
    const int sh1 = 7 - a.I, i_max = (1 << a.W) - 1;
    for (int i = tid; i < QL_EA; i += QL_THREADS) {
        const int c = i % 20, pos = i / 20, y = pos / 14, x = pos % 14;
        int p[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q) p[r][q] = s_img[(2 * y + r) * 32 + 2 * x + q];
        int o00 = 0, o01 = 0, o10 = 0, o11 = 0;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int w = s_w1[c * 25 + ky * 5 + kx];
                o00 += w * p[ky][kx];
                o01 += w * p[ky][kx + 1];
                o10 += w * p[ky + 1][kx];
                o11 += w * p[ky + 1][kx + 1];
            }
        const int pre = max(max(o00, o01), max(o10, o11)) + s_w1[500 + c] * 256;
        s_p1[((y + 2) * QL_P1_W + x + 2) * QL_P1_C + c] = (int8_t)(min(max(ql_rne_shift(pre, sh1), 0), i_max) - 128);
    }
    __syncthreads();
    if (onA) {      // the image is no longer needed: its room becomes P1m, whose halo stays at code 0
        for (int i = tid; i < QL_P1_BYTES / 16; i += QL_THREADS) ((uint4*)s_p1m)[i] = uint4{QL_OFF, QL_OFF, QL_OFF, QL_OFF};
        __syncthreads();
    }

    // ---- what a thread keeps across the sample loop ---------------------------------------------------------------------------------
    const int lg = lane >> 4, ln = lane & 15;
    int pbase[4];      // wave = pooling window: position tile mt, column ln
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int s = min(mt * 16 + ln, 48);
        pbase[mt] = (((wave >> 1) * 7 + s / 7) * QL_P1_W + (wave & 1) * 7 + s % 7) * QL_P1_C;
    }
    float bias2[8];
    int corr2[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bias2[r] = (float)a.b2[lg * 4 + r] * s_bias;
        corr2[r] = s_corr2[lg * 4 + r];
        bias2[4 + r] = lg == 0 ? (float)a.b2[16 + r] * s_bias : 0.f;
        corr2[4 + r] = lg == 0 ? s_corr2[16 + r] : 0;
    }
    const int j1 = min(tid, QL_EC - 1);
    int w_fc1[QL_EB / 4], corr_fc1 = 0, corr_fc2 = 0;
#pragma unroll
    for (int k = 0; k < QL_EB / 16; ++k) {
        const ql_i32x4 w = ((const ql_i32x4*)(a.fc1 + j1 * QL_EB))[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w_fc1[k * 4 + i] = w[i];
            corr_fc1 = __builtin_amdgcn_sdot4(w[i], 0x01010101, corr_fc1, false);
        }
    }
    for (int k = 0; k < 25; ++k) corr_fc2 = __builtin_amdgcn_sdot4((int)s_fc2[k * 32 + (lane & 31)], 0x01010101, corr_fc2, false);
    corr_fc1 *= 128;
    corr_fc2 *= 128;
    const float b_fc1 = (float)a.fb1[j1] * s_bias;
    const float b_fc2 = (float)a.fb2[min(lane, C - 1)] * s_bias;
    const uint64_t eA0 = (uint64_t)(a.b0 + b) * QL_EA, eB0 = (uint64_t)(a.b0 + b) * QL_EB, eC = (uint64_t)(a.b0 + b) * QL_EC;
    const uint64_t eC0 = eC & ~7ull;          // 100 is a multiple of 4 only: the image's first keep byte starts up to 4 elements early
    const int offC = (int)(eC - eC0);
    const int shA = 7 - sA.log2_bits;         // log2 of the elements per Philox call
    const uint64_t cA0 = eA0 >> shA;
    const int nA = onA ? (int)(((eA0 + QL_EA - 1) >> shA) - cA0) + 1 : 0, nB = onB ? QL_EB / 8 : 0, nC = onC ? (offC + QL_EC + 7) / 8 : 0;
    uint8_t* const feat = (uint8_t*)s_feat;
    uint8_t* const featM = (uint8_t*)s_featM;
    uint8_t* const hpre = (uint8_t*)s_hpre;
    uint8_t* const hM = (uint8_t*)s_hM;
    double s1 = 0.0, s2 = 0.0, sl = 0.0;

    for (int it = 0; it < n_t; ++it) {
        const uint32_t t = (uint32_t)(a.t0 + it0 + it);
        const bool first = it == 0;
        // ---- the sample's keep bits, all sites, one Philox call per item ------------------------------------------------------------
        if (nA + nB + nC) {
            for (int i = tid; i < nA + nB + nC; i += QL_THREADS) {
                if (i < nA) {
                    const uint64_t e_call = (cA0 + (uint64_t)i) << shA;
                    const philox4 r = philox_site_call(sA, e_call, t);
                    for (int g = 0; g < (1 << (shA - 3)); ++g) {
                        const uint64_t e0 = e_call + 8u * g;
                        if (e0 >= eA0 && e0 < eA0 + QL_EA) s_keepA[(int)(e0 - eA0) >> 3] = sA.drop_all ? (uint8_t)0 : (uint8_t)philox_keep8(r, (uint32_t)e0, sA.log2_bits, sA.thresh);
                    }
                } else if (i < nA + nB) {
                    s_keepB[i - nA] = (uint8_t)site_keep8(sB, eB0 + 8u * (i - nA), t);
                } else {
                    s_keepC[i - nA - nB] = (uint8_t)site_keep8(sC, eC0 + 8u * (i - nA - nB), t);
                }
            }
            __syncthreads();
        }
        // ---- site A, conv2, pool 7, quantised ReLU -> the 80 feature bytes (once when site A is off) ---------------------------------
        if (first || onA) {
            const int8_t* src = s_p1;
            if (onA) {
                for (int i = tid; i < 196 * 5; i += QL_THREADS) {      // four channels of one position: one dword, one nibble of a keep byte
                    const int pos = i / 5, qd = i % 5, e = pos * 20 + qd * 4;
                    const uint32_t nib = (uint32_t)s_keepA[e >> 3] >> (e & 4);
                    const int off = ((pos / 14 + 2) * QL_P1_W + pos % 14 + 2) * QL_P1_C + qd * 4;
                    const uint32_t m = ((nib & 1u) ? 0xFFu : 0u) | ((nib & 2u) ? 0xFF00u : 0u) | ((nib & 4u) ? 0xFF0000u : 0u) | ((nib & 8u) ? 0xFF000000u : 0u);
                    *(uint32_t*)(s_p1m + off) = (*(const uint32_t*)(s_p1 + off) & m) | (QL_OFF & ~m);
                }
                __syncthreads();
                src = s_p1m;
            }
            int v[8];
            ql_conv2(src, s_w2, s_koff, pbase, lane, v);
            if (ln == 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r >= 4 && lg != 0) break;
                    const int j = (r < 4 ? lg * 4 + r : 12 + r) * 4 + wave;      // torch's flatten: channel * 4 + window
                    const uint8_t f = ql_act_byte(ql_affine(v[r] + corr2[r], s_acc, sA.scale, bias2[r]), s_w, a_max);
                    feat[j] = f;
                    if (onB) featM[j] = ql_kept(s_keepB, j) ? f : (uint8_t)0x80;
                }
            }
            __syncthreads();
        } else if (onB) {
            if (tid < QL_EB) featM[tid] = ql_kept(s_keepB, tid) ? feat[tid] : (uint8_t)0x80;
            __syncthreads();
        }
        // ---- site B's features -> fc1 + quantised ReLU -> site C (once when sites A and B are off) ------------------------------------
        if (first || onA || onB) {
            if (wave < 2 && tid < QL_EC) {
                const uint32_t* f = onB ? s_featM : s_feat;
                int acc = corr_fc1;
#pragma unroll
                for (int k = 0; k < QL_EB / 4; ++k) acc = __builtin_amdgcn_sdot4((int)f[k], w_fc1[k], acc, false);
                const uint8_t h = ql_act_byte(ql_affine(acc, s_acc, sB.scale, b_fc1), s_w, a_max);
                hpre[tid] = h;
                if (onC) hM[tid] = ql_kept(s_keepC, offC + tid) ? h : (uint8_t)0x80;
            }
            __syncthreads();
        } else if (onC) {
            if (tid < QL_EC) hM[tid] = ql_kept(s_keepC, offC + tid) ? hpre[tid] : (uint8_t)0x80;
            __syncthreads();
        }
        // ---- fc2, softmax, moment sums: wave 0, lane = class (the next barrier this wave meets is behind its reads of the hidden units) --
        if (wave == 0) {
            const uint32_t* h = onC ? s_hM : s_hpre;
            int acc = corr_fc2;
#pragma unroll 5
            for (int k = 0; k < QL_EC / 4; ++k) acc = __builtin_amdgcn_sdot4((int)h[k], (int)s_fc2[k * 32 + (lane & 31)], acc, false);
            const float z = ql_affine(acc, s_acc, sC.scale, b_fc2);
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
__global__ __launch_bounds__(QL_THREADS) void qlenet5_join_kernel(const double* __restrict__ part, int n_chunks, size_t n, double* S1, double* S2,
                                                                  double* SL) {
    const size_t i = (size_t)blockIdx.x * QL_THREADS + threadIdx.x;
    if (i >= 3 * n) return;
    const size_t m = i / n, r = i % n;
    double* S = m == 0 ? S1 : (m == 1 ? S2 : SL);
    double s = S[r];
    for (int ch = 0; ch < n_chunks; ++ch) s += part[((size_t)ch * 3 + m) * n + r];
    S[r] = s;
}

int launch_qlenet5(QLenet5Args a, hipStream_t s) {
    if (a.B < 1 || a.tc < 1 || a.C < 2 || a.C > 32 || a.W < 2 || a.W > 8 || a.I < 0 || a.I >= a.W) return BMI_ERR_INVALID;
    a.n_chunks = lenet5_chunks(a.B, a.tc, &a.per_chunk);
    if (a.S1 && a.n_chunks > 1 && !a.part) return BMI_ERR_NOMEM;
    hipLaunchKernelGGL(qlenet5_kernel, dim3((unsigned)a.B, (unsigned)a.n_chunks), dim3(QL_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    if (a.S1 && a.n_chunks > 1) {
        const size_t n = (size_t)a.B * a.C;
        hipLaunchKernelGGL(qlenet5_join_kernel, dim3((unsigned)((3 * n + QL_THREADS - 1) / QL_THREADS)), dim3(QL_THREADS), 0, s, a.part, a.n_chunks, n,
                           a.S1, a.S2, a.SL);
        BMI_CHECK_LAUNCH();
    }
    return BMI_OK;
}

}  // namespace

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
struct bmi_qlenet5_s {
    QLenet5Args args;
    bmi_site sites[3];
    size_t partials_bytes;
};

extern "C" {

int bmi_qlenet5_create(const bmi_qlenet5_desc* d, bmi_qlenet5_handle* out) {
    if (!d || !out) return BMI_ERR_INVALID;
    if (!d->conv1_q || !d->conv1_bq || !d->conv2_q_frag || !d->conv2_bq || !d->fc1_q || !d->fc1_bq || !d->fc2_q || !d->fc2_bq) return BMI_ERR_INVALID;
    if (d->quant_tbit < 2 || d->quant_tbit > 8 || d->quant_ibit < 0 || d->quant_ibit >= d->quant_tbit) return BMI_ERR_UNSUPPORTED;
    if (d->out_dim < 2 || d->out_dim > 32) return BMI_ERR_UNSUPPORTED;
    for (const bmi_site& st : d->sites) {
        if (st.kind == BMI_SITE_NONE) continue;
        if (st.kind == BMI_SITE_MASKSEMBLE || st.kind == BMI_SITE_CHANNEL) return BMI_ERR_UNSUPPORTED;
        if (st.kind != BMI_SITE_ELEMENTWISE) return BMI_ERR_INVALID;
        if (!(st.p >= 0.f && st.p < 1.f) || st.site_id < 0) return BMI_ERR_INVALID;      // (a NaN fails the comparison)
    }
    if (d->partials_bytes && !d->partials) return BMI_ERR_INVALID;
    bmi_qlenet5_s* h = new (std::nothrow) bmi_qlenet5_s();
    if (!h) return BMI_ERR_NOMEM;
    QLenet5Args& a = h->args;
    a.w1 = d->conv1_q; a.b1 = d->conv1_bq; a.w2f = d->conv2_q_frag; a.b2 = d->conv2_bq;
    a.fc1 = d->fc1_q; a.fb1 = d->fc1_bq; a.fc2 = d->fc2_q; a.fb2 = d->fc2_bq;
    a.C = d->out_dim; a.W = d->quant_tbit; a.I = d->quant_ibit;
    a.part = (double*)d->partials;
    for (int i = 0; i < 3; ++i) h->sites[i] = d->sites[i];
    h->partials_bytes = d->partials_bytes;
    *out = h;
    return BMI_OK;
}

int bmi_qlenet5_destroy(bmi_qlenet5_handle h) {
    delete h;
    return BMI_OK;
}

int bmi_qlenet5_forward_mcd(bmi_qlenet5_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed, double* S1,
                            double* S2, double* SL, float* logits, bmi_stream stream) {
    if (!h || !x_nchw || batch < 1 || t_count < 1 || t_begin < 0) return BMI_ERR_INVALID;
    const bool sums = S1 || S2 || SL;
    if ((sums && !(S1 && S2 && SL)) || (!sums && !logits)) return BMI_ERR_INVALID;
    QLenet5Args a = h->args;
    const int chunks = lenet5_chunks(batch, t_count, nullptr);
    if (sums && chunks > 1 && (size_t)chunks * 3 * batch * a.C * sizeof(double) > h->partials_bytes) return BMI_ERR_NOMEM;
    a.x = x_nchw; a.B = batch; a.b0 = 0; a.t0 = t_begin; a.tc = t_count;
    a.S1 = S1; a.S2 = S2; a.SL = SL; a.logits = logits;
    for (int i = 0; i < 3; ++i) a.site[i] = resolve_site(h->sites[i].kind == BMI_SITE_NONE ? nullptr : &h->sites[i], seed, 0);
    return launch_qlenet5(a, (hipStream_t)stream);
}

}  // extern "C"
