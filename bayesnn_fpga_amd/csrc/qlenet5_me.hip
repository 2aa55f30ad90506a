// The QUANTISED multi-exit MC-dropout LeNet-5 of the reference's hardware flow as ONE kernel: T_Qlenet_bayes_me
// (Hardware_Artifact/bayes_hw/models/t_qmodels_bayes_me.py:41-147), the network of lenet5_me.hip with every kernel and bias through
// quantized_bits(W, I, alpha = 1) and every activation through quantized_relu(W): the model train_qkeras_mcme.py trains.  The arithmetic is
// qlenet5.hip's fixed point, the shape of the work lenet5_me.hip's: a heavy deterministic prefix, once per image, then a sample loop in
// which the waves never meet.  A plain integer loop on the host reproduces the fp32 logits of both exits bit for bit.
//
// Arithmetic   (the contract, bmi_qlenet5_desc's layer for layer; W = quant_tbit in [2, 8], I = quant_ibit in [0, W-1], F = W-1-I, rne =
//              round half to even)  weight / bias code q = clip(rne(w * 2^F), -2^(W-1), 2^(W-1) - 1), value q * 2^-F: quantised by the
//              HOST; activation code a = clip(rne(v * 2^W), 0, 2^W - 1), value a * 2^-W; input x8 = clip(rne(x * 2^8), 0, 255).
//              conv1: acc = sum x8 * q1 over the 25 taps, pre = acc + (b1 << 8), a1 = clip(rne(pre / 2^(7-I)), 0, 2^W - 1) on integers, then
//              the 2x2 max on codes.  conv2, fc1, fc2, ex1conv1, ex1fc1, ex1linear: acc = sum keep * a * q in int32 (at most 500 * 255 * 128
//              < 2^24, so float(acc) is exact), y = fadd_rn(fmul_rn(float(acc) * 2^-(W+F), d), b * 2^-F): two rounded operations, never one
//              FMA (this file is compiled with fp contraction off); d = fl32(1 / fl32(1 - p)) for the two classifiers when their site is
//              on, 1 everywhere else.  The hidden layers end in a = clip(rintf(y * 2^W), 0, 2^W - 1), conv2 then in the 7x7 max on codes
//              (taken on the raw integers: every step from acc to a is non-decreasing); the classifiers' y is the logit.
// Signed operands  as qlenet5.hip: every activation byte is stored as a - 128 (a ^ 0x80), the halo and a dropped unit are -128 = code 0, and
//              every output adds 128 * sum q over its layer's whole K to its integer sum.  Dropping is a byte select.
// Work split   grid.x = image, 256 threads = 4 waves, all t_count samples of the call: no sample chunks, no partials, no join launch.
// Prefix       qlenet5.hip's (its device functions are restated here: sharing them through a header changed the sibling's register
//              allocation, and that kernel stays as it is): x8 with a 2-pixel halo and conv1's codes in LDS, conv1 on the VALU in int32 ->
//              P1, i8 [18][18][32].  No site touches the map, so there is no masked copy; the image and conv1's codes are staged in the room
//              of conv2's fragments, which wait in 3 x 4 registers per thread until conv1 is done (the load's latency lies under conv1).
// conv2        qlenet5.hip's implicit GEMM: K = 500 split 16 + 4 channels, 9 K-steps of 64 on v_mfma_i32_16x16x64_i8, wave q = pooling
//              window q, four position tiles x two output-channel tiles, + 128 * sum q per output channel.
// ex1conv1     one more position tile of the same K walk over the same map: tap (ky, kx) of output (oy, ox) at byte ((7 oy + ky + 2) * 18
//              + 7 ox + kx + 2) * 32, four live columns of 16, fragments [36][20][16] straight from global memory (used once per image).
//              SPLIT-K over the waves: wave w runs K-steps 2 w, 2 w + 1 (wave 3: 6, 7, 8 — the two gathered tail steps), the int32 partials
//              are added through LDS by 80 threads, exact in any order.  One barrier more than a fifth tile on wave 3 would take; the two
//              forms were timed against each other and do not differ measurably (profiles/lenet5.md), the split was kept.
// Hidden layers  side by side, threads 0..99 fc1 and 128..227 ex1fc1: the weight row as five 16-byte loads from global memory, 20
//              v_dot4_i32_i8 over the branch's 80 feature bytes, the correction from the same registers; 2 x 100 hidden bytes to LDS.
// Sample loop  one barrier behind the prefix, none inside.  Wave w owns exit w >> 1 and the samples of parity w & 1 (counted from the call's
//              first sample).  Lane k < 25 holds hidden dword k of its exit (4 units), lane c < C the 25 weight dwords of class c with the
//              class's correction and bias.  A sample: lanes 0..13 draw the keep bytes (site_keep8; image b's first element b * 100 is a
//              multiple of 4 only, so the first byte may start 4 elements early), one shuffle hands lane k its nibble, which becomes a byte
//              mask that selects 0x80 into the dropped bytes; 25 v_readlane + v_dot4_i32_i8 (lane = class), the two-step affine, then the
//              max-subtracted softmax by wave shuffles and S1 += p, S2 += p * p, SL += z in float64 registers.  No LDS in a sample.  With a
//              site off the same loop runs on the unmasked dwords with d = 1.
// Join         lenet5_me.hip's: the odd-parity wave of an exit hands its three float64 sums to the even one through LDS, once:
//              S += even-sample sum + odd-sample sum, a fixed order.
// LDS          P1 10 368 + conv2 fragments 11 520 + offsets 240 + corrections 160 + ex1conv1 partials 1 280 + features 160 + hidden
//              units 200 + join 1 536 = 25 464 bytes (25 472 as laid out); 88 VGPRs, no scratch, no spills: five workgroups per CU.
// Deviation    from the plan of one staging area beside the fragments: the fragments' copy into LDS moved behind conv1 (one more barrier),
//              which is what lets the image overlay them.
#include <new>

#include "kernels.h"

#pragma clang fp contract(off)

struct QLenet5MeArgs {
    const float* x;          // fp32 [B][1][28][28]
    const int8_t* w1;        // trunk: as qlenet5.hip (include/bayesnn_fpga_amd.h: bmi_qlenet5_desc)
    const int8_t* b1;
    const int8_t* w2f;
    const int8_t* b2;
    const int8_t* fc1;
    const int8_t* fb1;
    const int8_t* fc2;
    const int8_t* fb2;
    const int8_t* ewf;       // ex1conv1 codes [36][20][16], conv2's fragment layout
    const int8_t* eb;
    const int8_t* efc1;      // ex1fc1 codes [100][80]
    const int8_t* efb1;
    const int8_t* elin;      // ex1linear codes [C][100]
    const int8_t* elinb;
    int W, I;                // quant_tbit, quant_ibit
    int B, C;
    int t0, tc;              // first sample, samples
    SiteArgs site[2];        // on the 100 hidden units in front of exit 0 / exit 1 (kind BMI_SITE_NONE: off)
    double* S1;              // float64 [2][B][C] sums, ADDED to; all three null: logits only
    double* S2;
    double* SL;
    float* logits;           // fp32 [tc][2][B][C] or null
};

namespace {

typedef int qm_i32x4 __attribute__((ext_vector_type(4)));

constexpr int QM_THREADS = 256;
constexpr int QM_P1_W = 18, QM_P1_C = 32, QM_P1_BYTES = QM_P1_W * QM_P1_W * QM_P1_C;      // 10368
constexpr int QM_KG_MAIN = 28, QM_KG = 36, QM_KS_MAIN = 7, QM_KS = 9;      // 16-byte K-groups (25 + 7 live), K-steps of 64
constexpr int QM_EA = 3920, QM_EB = 80, QM_EC = 100;      // per image: the pooled conv1 map, a branch's features, its hidden units
constexpr uint32_t QM_OFF = 0x80808080u;                  // four activation bytes of code 0

// rne(v / 2^sh) on integers, sh in [0, 7]
__device__ __forceinline__ int qm_rne_shift(int v, int sh) {
    const int q = v >> sh, rem = v & ((1 << sh) - 1), half = (1 << sh) >> 1;
    return q + ((rem > half || (sh > 0 && rem == half && (q & 1))) ? 1 : 0);
}

// y = fadd_rn(fmul_rn(float(acc) * 2^-(W+F), d), bias): the power-of-two product is exact, the other two operations round (contraction is off)
__device__ __forceinline__ float qm_affine(int acc, float s_acc, float d, float bias) {
    const float prod = ((float)acc * s_acc) * d;
    return prod + bias;
}

// the stored byte (code ^ 0x80) of a = clip(rintf(y * 2^W), 0, 2^W - 1)
__device__ __forceinline__ uint8_t qm_act_byte(float y, float s_w, float a_max) { return (uint8_t)((int)fminf(fmaxf(rintf(y * s_w), 0.f), a_max) ^ 0x80); }

// raw conv2 sums, maximum over pooling window `wave`, from the haloed map `src`; the lanes with (lane & 15) == 0 return their channels' maxima
// in v[]: v[r] = channel 4 * (lane >> 4) + r, v[4 + r] = channel 16 + r (lanes 0..15 only).  The sums are over a - 128: the caller adds 128 * sum q.
__device__ __forceinline__ void qm_conv2(const int8_t* src, const int8_t* s_w2, const int* s_koff, const int pbase[4], int lane, int v[8]) {
    const int lg = lane >> 4, ln = lane & 15;
    qm_i32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = qm_i32x4{0, 0, 0, 0};
    const qm_i32x4 zero = {0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < QM_KS_MAIN; ++ks) {      // channels 0..15: one 16-byte read per fragment
        const int kg = ks * 4 + lg;
        const int koff = s_koff[kg];
        const qm_i32x4 w0 = *(const qm_i32x4*)(s_w2 + (kg * 20 + ln) * 16);
        const qm_i32x4 w1 = ln < 4 ? *(const qm_i32x4*)(s_w2 + (kg * 20 + 16 + ln) * 16) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const qm_i32x4 px = *(const qm_i32x4*)(src + pbase[mt] + koff);
            acc[mt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, px, acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, px, acc[mt][1], 0, 0, 0);
        }
    }
#pragma unroll 1
    for (int ks = QM_KS_MAIN; ks < QM_KS; ++ks) {      // channels 16..19: four taps per fragment, four 4-byte reads
        const int kg = ks * 4 + lg;
        const qm_i32x4 koff = *(const qm_i32x4*)(s_koff + QM_KG_MAIN + (kg - QM_KG_MAIN) * 4);
        const qm_i32x4 w0 = *(const qm_i32x4*)(s_w2 + (kg * 20 + ln) * 16);
        const qm_i32x4 w1 = ln < 4 ? *(const qm_i32x4*)(s_w2 + (kg * 20 + 16 + ln) * 16) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int8_t* p = src + pbase[mt];
            const qm_i32x4 px = {*(const int*)(p + koff[0]), *(const int*)(p + koff[1]), *(const int*)(p + koff[2]), *(const int*)(p + koff[3])};
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

// K-steps ks0 .. ks1-1 of ex1conv1's position tile: columns 0..3 are the four outputs (oy, ox) = (column >> 1, column & 1), columns 4..15
// repeat them and are dropped.  Rows as in qm_conv2; the weight fragments `wf` [36][20][16] are read from global memory.
__device__ __forceinline__ void qm_exit_conv(const int8_t* s_p1, const int8_t* __restrict__ wf, const int* s_koff, int ks0, int ks1, int lane,
                                             qm_i32x4& acc0, qm_i32x4& acc1) {
    const int lg = lane >> 4, ln = lane & 15, pos = ln & 3;
    const int8_t* p = s_p1 + ((7 * (pos >> 1) + 2) * QM_P1_W + 7 * (pos & 1) + 2) * QM_P1_C;
    const qm_i32x4 zero = {0, 0, 0, 0};
#pragma unroll 1
    for (int ks = ks0; ks < ks1; ++ks) {
        const int kg = ks * 4 + lg;
        const qm_i32x4 w0 = *(const qm_i32x4*)(wf + (kg * 20 + ln) * 16);
        const qm_i32x4 w1 = ln < 4 ? *(const qm_i32x4*)(wf + (kg * 20 + 16 + ln) * 16) : zero;
        qm_i32x4 px;
        if (ks < QM_KS_MAIN) {
            px = *(const qm_i32x4*)(p + s_koff[kg]);
        } else {
            const qm_i32x4 koff = *(const qm_i32x4*)(s_koff + QM_KG_MAIN + (kg - QM_KG_MAIN) * 4);
            px = qm_i32x4{*(const int*)(p + koff[0]), *(const int*)(p + koff[1]), *(const int*)(p + koff[2]), *(const int*)(p + koff[3])};
        }
        acc0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, px, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, px, acc1, 0, 0, 0);
    }
}

__global__ __launch_bounds__(QM_THREADS, 4) void qlenet5_me_kernel(QLenet5MeArgs a) {
    __shared__ __attribute__((aligned(16))) int8_t s_p1[QM_P1_BYTES];
    __shared__ __attribute__((aligned(16))) int8_t s_w2[QM_KG * 20 * 16];      // prefix: the haloed image and conv1's codes
    __shared__ __attribute__((aligned(16))) int s_koff[QM_KG_MAIN + 32];
    __shared__ int s_corr[2][20];                    // 128 * sum q per output channel: [0] conv2, [1] ex1conv1
    __shared__ int s_epart[4][QM_EB];                // ex1conv1's raw sums per wave (its share of the K-steps)
    __shared__ uint32_t s_feat[2][QM_EB / 4], s_h[2][QM_EC / 4];      // [exit]: four stored bytes per dword
    __shared__ double s_join[2][3][32];
    int* const s_img = (int*)s_w2;            // [32][32]
    int* const s_w1 = s_img + 1024;           // [20][25] then the 20 biases

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C;
    const int F = a.W - 1 - a.I;
    const float s_acc = ldexpf(1.f, -(a.W + F)), s_bias = ldexpf(1.f, -F), s_w = (float)(1 << a.W), a_max = (float)((1 << a.W) - 1);

    // ---- prefix: staging ----------------------------------------------------------------------------------------------------------
    uint4 w2r[3];      // conv2's fragments wait here until the image has left their room
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tid + k * QM_THREADS;
        w2r[k] = i < QM_KG * 20 ? ((const uint4*)a.w2f)[i] : uint4{0u, 0u, 0u, 0u};
    }
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += QM_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? (int)fminf(fmaxf(rintf(img[r * 28 + c] * 256.f), 0.f), 255.f) : 0;
    }
    for (int i = tid; i < 520; i += QM_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < QM_P1_BYTES / 16; i += QM_THREADS) ((uint4*)s_p1)[i] = uint4{QM_OFF, QM_OFF, QM_OFF, QM_OFF};
    if (tid < QM_KG_MAIN + 32) {      // K-group -> byte offset of its tap inside the haloed map (taps >= 25: zero weights, any valid offset)
        const int tap = min(tid < QM_KG_MAIN ? tid : tid - QM_KG_MAIN, 24);
        s_koff[tid] = ((tap / 5) * QM_P1_W + tap % 5) * QM_P1_C + (tid < QM_KG_MAIN ? 0 : 16);
    }
    if (tid < 160) {      // 128 * sum q of both convs' output channels: four threads per channel, nine K-groups each
        const int conv = tid / 80, ch = (tid % 80) >> 2;
        const int8_t* wf = conv ? a.ewf : a.w2f;
        int s = 0;
        for (int g = (tid & 3) * 9; g < (tid & 3) * 9 + 9; ++g) {
            const qm_i32x4 w = *(const qm_i32x4*)(wf + (g * 20 + ch) * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_sdot4(w[i], 0x01010101, s, false);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if ((tid & 3) == 0) s_corr[conv][ch] = 128 * s;
    }
    __syncthreads();

    // ---- prefix: conv1 + bias + 2x2 max + quantised ReLU -> P1 -------------------------------------------------------------------------
    const int sh1 = 7 - a.I, i_max = (1 << a.W) - 1;
    for (int i = tid; i < QM_EA; i += QM_THREADS) {
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
        s_p1[((y + 2) * QM_P1_W + x + 2) * QM_P1_C + c] = (int8_t)(min(max(qm_rne_shift(pre, sh1), 0), i_max) - 128);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tid + k * QM_THREADS;
        if (i < QM_KG * 20) ((uint4*)s_w2)[i] = w2r[k];
    }
    __syncthreads();

    // ---- prefix: ex1conv1 (this wave's K-steps) and conv2 (this wave's pooling window) -> the 2 x 80 feature bytes ----------------------
    const int lg = lane >> 4, ln = lane & 15;
    {
        qm_i32x4 e0 = {0, 0, 0, 0}, e1 = {0, 0, 0, 0};
        qm_exit_conv(s_p1, a.ewf, s_koff, 2 * wave, wave == 3 ? QM_KS : 2 * wave + 2, lane, e0, e1);
        if (ln < 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s_epart[wave][(lg * 4 + r) * 4 + ln] = e0[r];
                if (lg == 0) s_epart[wave][(16 + r) * 4 + ln] = e1[r];
            }
        }
        int pbase[4];      // wave = pooling window: position tile mt, column ln
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int s = min(mt * 16 + ln, 48);
            pbase[mt] = (((wave >> 1) * 7 + s / 7) * QM_P1_W + (wave & 1) * 7 + s % 7) * QM_P1_C;
        }
        int v[8];
        qm_conv2(s_p1, s_w2, s_koff, pbase, lane, v);
        if (ln == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (r >= 4 && lg != 0) break;
                const int c = r < 4 ? lg * 4 + r : 12 + r;
                ((uint8_t*)s_feat[1])[c * 4 + wave] = qm_act_byte(qm_affine(v[r] + s_corr[0][c], s_acc, 1.f, (float)a.b2[c] * s_bias), s_w, a_max);      // torch's flatten: channel * 4 + window
            }
        }
    }
    __syncthreads();
    if (tid >= 128 && tid < 128 + QM_EB) {      // ex1conv1: the four waves' sums of feature j = channel * 4 + oy * 2 + ox
        const int j = tid - 128, c = j >> 2;
        const int acc = s_epart[0][j] + s_epart[1][j] + s_epart[2][j] + s_epart[3][j] + s_corr[1][c];
        ((uint8_t*)s_feat[0])[j] = qm_act_byte(qm_affine(acc, s_acc, 1.f, (float)a.eb[c] * s_bias), s_w, a_max);
    }
    __syncthreads();

    // ---- prefix: fc1 (waves 0, 1) | ex1fc1 (waves 2, 3) -> the 2 x 100 hidden bytes ------------------------------------------------------
    {
        const int main_branch = tid < 128, j = tid & 127;
        if (j < QM_EC) {
            const qm_i32x4* row = (const qm_i32x4*)((main_branch ? a.fc1 : a.efc1) + j * QM_EB);
            const uint32_t* f = s_feat[main_branch];
            int acc = 0, corr = 0;
#pragma unroll
            for (int k = 0; k < QM_EB / 16; ++k) {
                const qm_i32x4 w = row[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc = __builtin_amdgcn_sdot4((int)f[k * 4 + i], w[i], acc, false);
                    corr = __builtin_amdgcn_sdot4(w[i], 0x01010101, corr, false);
                }
            }
            const float bias = (float)(main_branch ? a.fb1 : a.efb1)[j] * s_bias;
            ((uint8_t*)s_h[main_branch])[j] = qm_act_byte(qm_affine(acc + 128 * corr, s_acc, 1.f, bias), s_w, a_max);
        }
    }
    __syncthreads();

    // ---- sample loop: wave = (exit, parity of the sample's index in the call); no barrier ---------------------------------------------
    const int e = wave >> 1, par = wave & 1;
    const SiteArgs& st = a.site[e];
    const bool on = st.kind != BMI_SITE_NONE;
    const int cl = min(lane, C - 1);
    const int8_t* wrow = (e ? a.fc2 : a.elin) + cl * QM_EC;
    int w[QM_EC / 4], corr = 0;      // the classifier row of this lane's class
#pragma unroll
    for (int k = 0; k < QM_EC / 4; ++k) {
        w[k] = *(const int*)(wrow + 4 * k);
        corr = __builtin_amdgcn_sdot4(w[k], 0x01010101, corr, false);
    }
    corr *= 128;
    const float bias = (float)(e ? a.fb2 : a.elinb)[cl] * s_bias;
    const float d = on ? st.scale : 1.f;
    const int kd = min(lane, QM_EC / 4 - 1);
    const uint32_t hd = s_h[e][kd];                                 // units 4 kd .. 4 kd + 3
    const uint64_t eC = (uint64_t)b * QM_EC, eC0 = eC & ~7ull;      // 100 is a multiple of 4 only: the first keep byte starts up to 4 elements early
    const int offC = (int)(eC - eC0), nC = (offC + QM_EC + 7) / 8;
    const int kbyte = (offC + 4 * kd) >> 3, kshift = (offC + 4 * kd) & 7;      // this lane's nibble: a shift of 0 or 4
    double s1 = 0.0, s2 = 0.0, sl = 0.0;

    for (int it = par; it < a.tc; it += 2) {
        uint32_t hm = hd;
        if (on) {
            const uint32_t keep = lane < nC ? site_keep8(st, eC0 + 8u * (uint32_t)lane, (uint32_t)(a.t0 + it)) : 0u;
            const uint32_t nib = __shfl(keep, kbyte) >> kshift;
            const uint32_t m = ((nib & 1u) ? 0xFFu : 0u) | ((nib & 2u) ? 0xFF00u : 0u) | ((nib & 4u) ? 0xFF0000u : 0u) | ((nib & 8u) ? 0xFF000000u : 0u);
            hm = (hd & m) | (QM_OFF & ~m);
        }
        int acc = corr;
#pragma unroll
        for (int k = 0; k < QM_EC / 4; ++k) acc = __builtin_amdgcn_sdot4(__builtin_amdgcn_readlane((int)hm, k), w[k], acc, false);
        const float z = qm_affine(acc, s_acc, d, bias);
        float m = lane < C ? z : -INFINITY;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        const float ex = lane < C ? expf(z - m) : 0.f;
        float sum = ex;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane < C) {
            const double p = (double)(ex / sum);
            s1 += p;
            s2 += p * p;
            sl += (double)z;
            if (a.logits) a.logits[(((size_t)it * 2 + e) * a.B + b) * C + lane] = z;
        }
    }

    // ---- the two waves of an exit join their sums: even samples + odd samples ----------------------------------------------------------
    if (!a.S1) return;
    if (par == 1 && lane < 32) {
        s_join[e][0][lane] = s1;
        s_join[e][1][lane] = s2;
        s_join[e][2][lane] = sl;
    }
    __syncthreads();
    if (par == 0 && lane < C) {
        const size_t i = ((size_t)e * a.B + b) * C + lane;
        a.S1[i] += s1 + s_join[e][0][lane];
        a.S2[i] += s2 + s_join[e][1][lane];
        a.SL[i] += sl + s_join[e][2][lane];
    }
}

int launch_qlenet5_me(const QLenet5MeArgs& a, hipStream_t s) {
    if (a.B < 1 || a.tc < 1 || a.C < 2 || a.C > 32 || a.W < 2 || a.W > 8 || a.I < 0 || a.I >= a.W) return BMI_ERR_INVALID;
    hipLaunchKernelGGL(qlenet5_me_kernel, dim3((unsigned)a.B), dim3(QM_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

}  // namespace

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
struct bmi_qlenet5_me_s {
    QLenet5MeArgs args;
    bmi_site sites[2];
};

extern "C" {

int bmi_qlenet5_me_create(const bmi_qlenet5_me_desc* d, bmi_qlenet5_me_handle* out) {
    if (!d || !out) return BMI_ERR_INVALID;
    if (!d->conv1_q || !d->conv1_bq || !d->conv2_q_frag || !d->conv2_bq || !d->fc1_q || !d->fc1_bq || !d->fc2_q || !d->fc2_bq) return BMI_ERR_INVALID;
    if (!d->ex1conv1_q_frag || !d->ex1conv1_bq || !d->ex1fc1_q || !d->ex1fc1_bq || !d->ex1linear_q || !d->ex1linear_bq) return BMI_ERR_INVALID;
    if (d->quant_tbit < 2 || d->quant_tbit > 8 || d->quant_ibit < 0 || d->quant_ibit >= d->quant_tbit) return BMI_ERR_UNSUPPORTED;
    if (d->out_dim < 2 || d->out_dim > 32) return BMI_ERR_UNSUPPORTED;
    for (const bmi_site& st : d->sites) {
        if (st.kind == BMI_SITE_NONE) continue;
        if (st.kind == BMI_SITE_MASKSEMBLE || st.kind == BMI_SITE_CHANNEL) return BMI_ERR_UNSUPPORTED;
        if (st.kind != BMI_SITE_ELEMENTWISE) return BMI_ERR_INVALID;
        if (!(st.p >= 0.f && st.p < 1.f) || st.site_id < 0) return BMI_ERR_INVALID;      // (a NaN fails the comparison)
    }
    bmi_qlenet5_me_s* h = new (std::nothrow) bmi_qlenet5_me_s();
    if (!h) return BMI_ERR_NOMEM;
    QLenet5MeArgs& a = h->args;
    a.w1 = d->conv1_q; a.b1 = d->conv1_bq; a.w2f = d->conv2_q_frag; a.b2 = d->conv2_bq;
    a.fc1 = d->fc1_q; a.fb1 = d->fc1_bq; a.fc2 = d->fc2_q; a.fb2 = d->fc2_bq;
    a.ewf = d->ex1conv1_q_frag; a.eb = d->ex1conv1_bq; a.efc1 = d->ex1fc1_q; a.efb1 = d->ex1fc1_bq;
    a.elin = d->ex1linear_q; a.elinb = d->ex1linear_bq;
    a.C = d->out_dim; a.W = d->quant_tbit; a.I = d->quant_ibit;
    for (int i = 0; i < 2; ++i) h->sites[i] = d->sites[i];
    *out = h;
    return BMI_OK;
}

int bmi_qlenet5_me_destroy(bmi_qlenet5_me_handle h) {
    delete h;
    return BMI_OK;
}

int bmi_qlenet5_me_forward_mcd(bmi_qlenet5_me_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed,
                               double* S1, double* S2, double* SL, float* logits, bmi_stream stream) {
    if (!h || !x_nchw || batch < 1 || t_count < 1 || t_begin < 0) return BMI_ERR_INVALID;
    const bool sums = S1 || S2 || SL;
    if ((sums && !(S1 && S2 && SL)) || (!sums && !logits)) return BMI_ERR_INVALID;
    QLenet5MeArgs a = h->args;
    a.x = x_nchw; a.B = batch; a.t0 = t_begin; a.tc = t_count;
    a.S1 = S1; a.S2 = S2; a.SL = SL; a.logits = logits;
    for (int i = 0; i < 2; ++i) a.site[i] = resolve_site(h->sites[i].kind == BMI_SITE_NONE ? nullptr : &h->sites[i], seed, 0);
    return launch_qlenet5_me(a, (hipStream_t)stream);
}

}  // extern "C"
