// Multi-exit MC-dropout LeNet-5 as ONE kernel: the LeNet of lenet5.hip plus an early exit on the pooled conv1 map (conv 5x5x20 stride 7 ->
// ReLU -> 80 -> 100 -> ReLU -> C) and one elementwise MC-dropout site in front of each exit's classifier.  Replaces T forwards of
// T_Qlenet_bayes_me (Hardware_Artifact/bayes_hw/models/t_qmodels_bayes_me.py:41-147) plus the softmax / averaging of
// FullAnalysis._get_output (SA/train/results_analyzer.py:236-248).  Exit 0 is the early exit, exit 1 the main exit.
//
// Shape of the work: everything up to the two 100-unit hidden vectors is deterministic (2.4 M MAC + 50 k MAC per image); a Monte-Carlo
// sample is 2 x 100 x C multiply-adds, a softmax and one Philox call per 8 .. 64 hidden units.  So the opposite of lenet5_kernel: a heavy
// prefix, once, then a sample loop in which the waves never meet.
//
// Work split   grid.x = image, 256 threads = 4 waves, all t_count samples of the call.  No sample chunks, no partials, no join launch: the
//              float64 sums are added straight onto S1 / S2 / SL, no workgroup waits on another.
// Prefix       as lenet5_kernel (its device functions are restated here: sharing them through a header changed lenet5_kernel's register
//              allocation, and that kernel stays as it is): the haloed fp32 image -> conv1 + bias + ReLU + 2x2 max -> P1, fp16
//              [18][18][24]; conv2 on v_mfma_f32_16x16x32_f16, wave q = pooling window q, four position tiles -> the 80 features.
// Early exit   ex1conv1 has conv2's K structure (25 taps x 24 padded channels, 19 K-steps) and reads the same map: tap (ky, kx) of output
//              (oy, ox) lies at ((7 oy + ky + 2) * 18 + 7 ox + kx + 2) * 24, so it is ONE more position tile of the same walk with 4 live
//              columns of 16.  Wave 3 runs it behind its own window (5 tiles where the others have 4); its weight fragments come straight
//              from global memory (used once per image).  Then both hidden layers run side by side: threads 0..99 fc1 of the main branch,
//              threads 128..227 ex1fc1 — fp32, one FMA chain per output in ascending k from the bias.
// Sample loop  one barrier behind the prefix, none inside.  Wave w owns exit w >> 1 and the samples of parity w & 1 (counted from the
//              call's first sample).  It keeps its exit's hidden units in two registers (lane j: units j and 64 + j) and the classifier
//              column of class `lane` in 100 registers, so a sample touches no LDS at all: lanes 0..13 draw the keep bytes
//              (site_keep8; image b's first element b * 100 is a multiple of 4 only, so the first byte may start 4 elements early), two
//              shuffles hand every lane its units' bits, the fc is 100 v_readlane + FMA in ascending k from the bias (lane = class), then
//              the max-subtracted softmax by wave shuffles and S1 += p, S2 += p * p, SL += z in float64 registers.  A logit row depends on
//              (seed, t, image) alone.  With a site off the wave runs the same loop on the unmasked units.
// Join         the odd-parity wave of an exit hands its three float64 sums to the even one through LDS, once, behind the loop:
//              S += even-sample sum + odd-sample sum, a fixed order.
// LDS          P1 15 552 + conv2 fragments 24 320 + image and conv1 weights 6 176 + offsets 304 + features 640 + hidden units 800 + join
//              1 536 = 49 328 bytes: two workgroups per CU.  (The classifier matrices live in registers, not in LDS.)
#include <new>

#include "kernels.h"

namespace {

typedef _Float16 lm_half8 __attribute__((ext_vector_type(8)));
typedef float lm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LM_THREADS = 256;
constexpr int LM_P1_W = 18, LM_P1_C = 24, LM_P1_HALVES = LM_P1_W * LM_P1_W * LM_P1_C;     // 7776
constexpr int LM_KG = 76, LM_KSTEPS = 19;       // K-groups of 8 (75 live), K-steps of 32
constexpr int LM_EA = 3920, LM_EB = 80, LM_EC = 100;      // per image: the pooled conv1 map, a branch's features, its hidden units

// conv1 + bias + ReLU + 2x2 max -> P1: one item = one pooled position x channel, its 6 x 6 input patch in registers
__device__ __forceinline__ void lm_conv1_pool(const float* s_img, const float* s_w1, _Float16* s_p1, int tid) {
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
}

// conv2 + bias + ReLU + 7x7 max of pooling window `wave` -> feat[channel * 4 + wave] (torch's flatten).  Channels are the MFMA rows
// (lane (ln, lg) holds rows 4 lg + r of tile 0 and, for lg == 0, 16 + r of tile 1), positions the columns: four tiles of 16 of the window's
// 49 positions (the last repeats position 48: a duplicate cannot change a maximum).
__device__ __forceinline__ void lm_conv2_pool(const _Float16* s_p1, const _Float16* s_w2, const int* s_koff, const float* b2, int wave, int lane,
                                              float* feat) {
    const int lg = lane >> 4, ln = lane & 15;
    int pbase[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int s = min(mt * 16 + ln, 48);
        pbase[mt] = (((wave >> 1) * 7 + s / 7) * LM_P1_W + (wave & 1) * 7 + s % 7) * LM_P1_C;
    }
    lm_f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = lm_f32x4{0.f, 0.f, 0.f, 0.f};
    const lm_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < LM_KSTEPS; ++ks) {
        const int kg = ks * 4 + lg;
        const int koff = s_koff[kg];
        const lm_half8 w0 = *(const lm_half8*)(s_w2 + (kg * 20 + ln) * 8);
        const lm_half8 w1 = ln < 4 ? *(const lm_half8*)(s_w2 + (kg * 20 + 16 + ln) * 8) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const lm_half8 px = *(const lm_half8*)(s_p1 + pbase[mt] + koff);
            acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, px, acc[mt][0], 0, 0, 0);
            acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, px, acc[mt][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = nt ? 16 + r : lg * 4 + r;
            float m = fmaxf(fmaxf(acc[0][nt][r], acc[1][nt][r]), fmaxf(acc[2][nt][r], acc[3][nt][r]));
            m = fmaxf(m + b2[c], 0.f);      // the maximum commutes with the bias and ReLU
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
            if (ln == 0 && (nt == 0 || lg == 0)) feat[c * 4 + wave] = m;
        }
}

// ex1conv1 + bias + ReLU -> feat[channel * 4 + oy * 2 + ox]: one position tile whose columns 0..3 are the four outputs (columns 4..15
// repeat them and are dropped); the weight fragments `wf` [76][20][8] are read from global memory
__device__ __forceinline__ void lm_exit_conv(const _Float16* s_p1, const _Float16* __restrict__ wf, const int* s_koff, const float* eb, int lane,
                                             float* feat) {
    const int lg = lane >> 4, ln = lane & 15, pos = ln & 3;
    const int pbase = ((7 * (pos >> 1) + 2) * LM_P1_W + 7 * (pos & 1) + 2) * LM_P1_C;
    lm_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const lm_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (int ks = 0; ks < LM_KSTEPS; ++ks) {
        const int kg = ks * 4 + lg;
        const lm_half8 w0 = *(const lm_half8*)(wf + (kg * 20 + ln) * 8);
        const lm_half8 w1 = ln < 4 ? *(const lm_half8*)(wf + (kg * 20 + 16 + ln) * 8) : zero;
        const lm_half8 px = *(const lm_half8*)(s_p1 + pbase + s_koff[kg]);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, px, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, px, acc1, 0, 0, 0);
    }
    if (ln < 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            feat[(lg * 4 + r) * 4 + ln] = fmaxf(acc0[r] + eb[lg * 4 + r], 0.f);
            if (lg == 0) feat[(16 + r) * 4 + ln] = fmaxf(acc1[r] + eb[16 + r], 0.f);
        }
    }
}

__device__ __forceinline__ float lm_readlane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

__global__ __launch_bounds__(LM_THREADS, 2) void lenet5_me_kernel(Lenet5MeArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 s_p1[LM_P1_HALVES];
    __shared__ __attribute__((aligned(16))) _Float16 s_w2[LM_KG * 20 * 8];
    __shared__ float s_img[1024];            // [32][32]: the image with a 2-pixel zero halo
    __shared__ float s_w1[520];              // [20][25] then the 20 biases
    __shared__ int s_koff[LM_KG];
    __shared__ float s_feat[2][LM_EB], s_h[2][LM_EC];      // [exit]
    __shared__ double s_join[2][3][32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C;

    // ---- prefix: staging -> conv1 + pool -> conv2 + pool | ex1conv1 -> fc1 | ex1fc1 --------------------------------------------------
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += LM_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? img[r * 28 + c] : 0.f;
    }
    for (int i = tid; i < 520; i += LM_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < LM_P1_HALVES / 8; i += LM_THREADS) ((uint4*)s_p1)[i] = uint4{0u, 0u, 0u, 0u};      // halo and padding channels stay zero
    for (int i = tid; i < LM_KG * 20; i += LM_THREADS) ((uint4*)s_w2)[i] = ((const uint4*)a.w2f)[i];
    if (tid < LM_KG) {      // K-group -> offset of its tap and channel group inside the haloed map (group 75: zero weights, any valid offset)
        const int kg = min(tid, LM_KG - 2), tap = kg / 3;
        s_koff[tid] = ((tap / 5) * LM_P1_W + tap % 5) * LM_P1_C + (kg % 3) * 8;
    }
    __syncthreads();
    lm_conv1_pool(s_img, s_w1, s_p1, tid);
    __syncthreads();
    lm_conv2_pool(s_p1, s_w2, s_koff, a.b2, wave, lane, s_feat[1]);
    if (wave == 3) lm_exit_conv(s_p1, a.ewf, s_koff, a.eb, lane, s_feat[0]);
    __syncthreads();
    {
        const int main_branch = tid < 128, j = tid & 127;      // waves 0, 1: fc1; waves 2, 3: ex1fc1
        if (j < LM_EC) {
            const float* wt = main_branch ? a.fc1t : a.efc1t;
            const float* f = s_feat[main_branch];
            float h = (main_branch ? a.fb1 : a.efb1)[j];
#pragma unroll 16
            for (int k = 0; k < LM_EB; ++k) h = fmaf(f[k], wt[k * LM_EC + j], h);
            s_h[main_branch][j] = fmaxf(h, 0.f);
        }
    }
    __syncthreads();

    // ---- sample loop: wave = (exit, parity of the sample's index in the call); no barrier ---------------------------------------------
    const int e = wave >> 1, par = wave & 1;
    const SiteArgs& st = a.site[e];
    const bool on = st.kind != BMI_SITE_NONE;
    const int cl = min(lane, C - 1);
    const float* wt = e ? a.fc2t : a.elint;
    float w[LM_EC];      // the classifier column of this lane's class
#pragma unroll
    for (int k = 0; k < LM_EC; ++k) w[k] = wt[k * C + cl];
    const float bias = (e ? a.fb2 : a.elinb)[cl];
    const float h0 = s_h[e][lane], h1 = lane < LM_EC - 64 ? s_h[e][64 + lane] : 0.f;      // units lane and 64 + lane
    const uint64_t eC = (uint64_t)b * LM_EC, eC0 = eC & ~7ull;      // 100 is a multiple of 4 only: the first keep byte starts up to 4 elements early
    const int offC = (int)(eC - eC0), nC = (offC + LM_EC + 7) / 8;
    const int bit = (offC + lane) & 7, byte0 = (offC + lane) >> 3, byte1 = (offC + 64 + lane) >> 3;      // (offC + 64 + lane) & 7 == bit
    double s1 = 0.0, s2 = 0.0, sl = 0.0;

    for (int it = par; it < a.tc; it += 2) {
        float m0 = h0, m1 = h1;
        if (on) {
            const uint32_t keep = lane < nC ? site_keep8(st, eC0 + 8u * (uint32_t)lane, (uint32_t)(a.t0 + it)) : 0u;
            const uint32_t k0 = __shfl(keep, byte0), k1 = __shfl(keep, byte1);
            m0 = ((k0 >> bit) & 1u) ? h0 * st.scale : 0.f;
            m1 = ((k1 >> bit) & 1u) ? h1 * st.scale : 0.f;
        }
        float z = bias;
#pragma unroll
        for (int k = 0; k < 64; ++k) z = fmaf(lm_readlane(m0, k), w[k], z);
#pragma unroll
        for (int k = 64; k < LM_EC; ++k) z = fmaf(lm_readlane(m1, k - 64), w[k], z);
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

}  // namespace

int launch_lenet5_me(const Lenet5MeArgs& a, hipStream_t s) {
    if (a.B < 1 || a.tc < 1 || a.C < 2 || a.C > 32) return BMI_ERR_INVALID;
    hipLaunchKernelGGL(lenet5_me_kernel, dim3((unsigned)a.B), dim3(LM_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
struct bmi_lenet5_me_s {
    Lenet5MeArgs args;
    bmi_site sites[2];
};

extern "C" {

int bmi_lenet5_me_create(const bmi_lenet5_me_desc* d, bmi_lenet5_me_handle* out) {
    if (!d || !out) return BMI_ERR_INVALID;
    if (!d->conv1_w || !d->conv1_b || !d->conv2_w_frag || !d->conv2_b || !d->fc1_wt || !d->fc1_b || !d->fc2_wt || !d->fc2_b) return BMI_ERR_INVALID;
    if (!d->ex1conv1_w_frag || !d->ex1conv1_b || !d->ex1fc1_wt || !d->ex1fc1_b || !d->ex1linear_wt || !d->ex1linear_b) return BMI_ERR_INVALID;
    if (d->out_dim < 2 || d->out_dim > 32) return BMI_ERR_UNSUPPORTED;
    for (const bmi_site& st : d->sites) {
        if (st.kind == BMI_SITE_NONE) continue;
        if (st.kind != BMI_SITE_ELEMENTWISE) return (st.kind == BMI_SITE_CHANNEL || st.kind == BMI_SITE_MASKSEMBLE) ? BMI_ERR_UNSUPPORTED : BMI_ERR_INVALID;
        if (!(st.p >= 0.f && st.p < 1.f) || st.site_id < 0) return BMI_ERR_INVALID;      // (a NaN fails the comparison)
    }
    bmi_lenet5_me_s* h = new (std::nothrow) bmi_lenet5_me_s();
    if (!h) return BMI_ERR_NOMEM;
    Lenet5MeArgs& a = h->args;
    a.w1 = d->conv1_w; a.b1 = d->conv1_b; a.w2f = (const _Float16*)d->conv2_w_frag; a.b2 = d->conv2_b;
    a.fc1t = d->fc1_wt; a.fb1 = d->fc1_b; a.fc2t = d->fc2_wt; a.fb2 = d->fc2_b;
    a.ewf = (const _Float16*)d->ex1conv1_w_frag; a.eb = d->ex1conv1_b; a.efc1t = d->ex1fc1_wt; a.efb1 = d->ex1fc1_b;
    a.elint = d->ex1linear_wt; a.elinb = d->ex1linear_b;
    a.C = d->out_dim;
    for (int i = 0; i < 2; ++i) h->sites[i] = d->sites[i];
    *out = h;
    return BMI_OK;
}

int bmi_lenet5_me_destroy(bmi_lenet5_me_handle h) {
    delete h;
    return BMI_OK;
}

int bmi_lenet5_me_forward_mcd(bmi_lenet5_me_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed,
                              double* S1, double* S2, double* SL, float* logits, bmi_stream stream) {
    if (!h || !x_nchw || batch < 1 || t_count < 1 || t_begin < 0) return BMI_ERR_INVALID;
    const bool sums = S1 || S2 || SL;
    if ((sums && !(S1 && S2 && SL)) || (!sums && !logits)) return BMI_ERR_INVALID;
    Lenet5MeArgs a = h->args;
    a.x = x_nchw; a.B = batch; a.t0 = t_begin; a.tc = t_count;
    a.S1 = S1; a.S2 = S2; a.SL = SL; a.logits = logits;
    for (int i = 0; i < 2; ++i) a.site[i] = resolve_site(h->sites[i].kind == BMI_SITE_NONE ? nullptr : &h->sites[i], seed, 0);
    return launch_lenet5_me(a, (hipStream_t)stream);
}

}  // extern "C"
