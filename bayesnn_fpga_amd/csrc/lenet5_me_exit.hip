// The multi-exit MC-dropout LeNet-5 of lenet5_me.hip with the staged early exit INSIDE the launch: an image whose early exit is confident
// (bmi_exit_rule, exit_rule.h) stops there and never pays for conv2 (1.96 M of the image's 2.4 M MAC), for its 24 KB of fragments, for fc1 or
// for the main exit's samples.  A workgroup owns one image, so "this image leaves" is a workgroup-uniform return: no compaction, no second
// launch, no workgroup waits on another.  Every row the kernel writes has the bits lenet5_me_kernel writes for samples 0 .. t_count-1.
//
// Work split   grid.x = image, 256 threads = 4 waves, all t_count samples of the call, two stages in one launch.
// Stage 0      every image.  Staging (haloed fp32 image, conv1's weights, zeroed P1, K-group offsets) -> conv1 + bias + ReLU + 2x2 max -> P1,
//              fp16 [18][18][24] -> ex1conv1 on v_mfma_f32_16x16x32_f16 by wave 3 alone, the 19 K-steps in lenet5_me_kernel's order, weight
//              fragments from global memory -> ex1fc1 on threads 0..99, one FMA chain per output in ascending k from the bias -> the T
//              samples of exit 0 -> the decision.  The device functions are restated from lenet5_me.hip, which stays as it is.
// Prefetch     while wave 3 runs ex1conv1, waves 0..2 would idle: they copy conv2's fragments into LDS instead.  An image that leaves has
//              read 24 KB from L2 for nothing; an image that stays finds them there behind the decision (measured both ways:
//              profiles/lenet5.md).
// Samples      lenet5_me_kernel gives an exit two waves; here the other exit is not running, so all four waves take the exit's samples: wave
//              w those with it % 4 == w.  A wave keeps the classifier column of class `lane` in 100 registers and the hidden units in two
//              (lane j: units j and 64 + j); keep bytes by site_keep8 on lanes 0..13, the fc as 100 v_readlane + FMA in ascending k from the
//              bias, the max-subtracted softmax by wave shuffles: a sample touches no LDS until its result.
// Hand-off     the float64 sums must be added in the full kernel's order (even samples ascending, odd samples ascending, S += even + odd),
//              and no wave owns a parity now.  So the waves work in rounds of 64 samples: each writes its samples' fp32 (p, z) into the LDS
//              table [sample of the round][class], one barrier, then wave 0 adds the even rows in ascending order into float64 registers
//              and wave 1 the odd rows (p, p * p, z), one barrier before the next round overwrites the table.  No cap on T.  Behind the last
//              round wave 1 hands its three sums to wave 0 through LDS: S += even + odd, as lenet5_me_kernel's join.
// Decision     wave 0 leaves the new S1 row of exit 0 in LDS; behind one barrier EVERY thread evaluates exit_rule_stat (the function the graph
//              engine's rule runs: float64 p_c = S1 / t_count, no contraction) on it, so the branch is uniform without another barrier.
//              stat > threshold (strict: a NaN keeps the image): exit_of_image[b] = 0 and the workgroup returns; exit 1's rows stay zero.
// Stage 1      images that stay: conv2 + bias + ReLU + 7x7 max on the MFMA (wave q = pooling window q, four position tiles) -> fc1 on threads
//              0..99 -> the T samples of exit 1 by the same rounds -> exit 1's rows, exit_of_image[b] = 1.
// LDS          P1 15 552 + conv2 fragments 24 320 + image and conv1 weights 6 176 + offsets 304 + features 640 + hidden units 800 + sample
//              table 16 384 + join 768 + decision row 256 = 65 200 bytes: two workgroups per CU.
// Registers    165 VGPRs (100 of them a lane's classifier column), no AGPRs, no scratch, no VGPR spills (3 SGPRs spill into VGPR lanes).
#include "kernels.h"

#include "exit_rule.h"

namespace {

typedef _Float16 lx_half8 __attribute__((ext_vector_type(8)));
typedef float lx_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LX_THREADS = 256;
constexpr int LX_P1_W = 18, LX_P1_C = 24, LX_P1_HALVES = LX_P1_W * LX_P1_W * LX_P1_C;     // 7776
constexpr int LX_KG = 76, LX_KSTEPS = 19;       // K-groups of 8 (75 live), K-steps of 32
constexpr int LX_EA = 3920, LX_EB = 80, LX_EC = 100;      // per image: the pooled conv1 map, a branch's features, its hidden units
constexpr int LX_ROUND = 64;                    // samples whose (p, z) the table holds at once

// conv1 + bias + ReLU + 2x2 max -> P1: one item = one pooled position x channel, its 6 x 6 input patch in registers
__device__ __forceinline__ void lx_conv1_pool(const float* s_img, const float* s_w1, _Float16* s_p1, int tid) {
    for (int i = tid; i < LX_EA; i += LX_THREADS) {
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
        s_p1[((y + 2) * LX_P1_W + x + 2) * LX_P1_C + c] = (_Float16)fmaxf(fmaxf(fmaxf(o00, o01), fmaxf(o10, o11)), 0.f);
    }
}

// conv2 + bias + ReLU + 7x7 max of pooling window `wave` -> feat[channel * 4 + wave] (torch's flatten).  Channels are the MFMA rows
// (lane (ln, lg) holds rows 4 lg + r of tile 0 and, for lg == 0, 16 + r of tile 1), positions the columns: four tiles of 16 of the window's
// 49 positions (the last repeats position 48: a duplicate cannot change a maximum).
__device__ __forceinline__ void lx_conv2_pool(const _Float16* s_p1, const _Float16* s_w2, const int* s_koff, const float* b2, int wave, int lane,
                                              float* feat) {
    const int lg = lane >> 4, ln = lane & 15;
    int pbase[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int s = min(mt * 16 + ln, 48);
        pbase[mt] = (((wave >> 1) * 7 + s / 7) * LX_P1_W + (wave & 1) * 7 + s % 7) * LX_P1_C;
    }
    lx_f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = lx_f32x4{0.f, 0.f, 0.f, 0.f};
    const lx_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < LX_KSTEPS; ++ks) {
        const int kg = ks * 4 + lg;
        const int koff = s_koff[kg];
        const lx_half8 w0 = *(const lx_half8*)(s_w2 + (kg * 20 + ln) * 8);
        const lx_half8 w1 = ln < 4 ? *(const lx_half8*)(s_w2 + (kg * 20 + 16 + ln) * 8) : zero;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const lx_half8 px = *(const lx_half8*)(s_p1 + pbase[mt] + koff);
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
// repeat them and are dropped); tap (ky, kx) of output (oy, ox) lies at ((7 oy + ky + 2) * 18 + 7 ox + kx + 2) * 24 of the haloed map; the
// weight fragments `wf` [76][20][8] are read from global memory (used once per image)
__device__ __forceinline__ void lx_exit_conv(const _Float16* s_p1, const _Float16* __restrict__ wf, const int* s_koff, const float* eb, int lane,
                                             float* feat) {
    const int lg = lane >> 4, ln = lane & 15, pos = ln & 3;
    const int pbase = ((7 * (pos >> 1) + 2) * LX_P1_W + 7 * (pos & 1) + 2) * LX_P1_C;
    lx_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const lx_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (int ks = 0; ks < LX_KSTEPS; ++ks) {
        const int kg = ks * 4 + lg;
        const lx_half8 w0 = *(const lx_half8*)(wf + (kg * 20 + ln) * 8);
        const lx_half8 w1 = ln < 4 ? *(const lx_half8*)(wf + (kg * 20 + 16 + ln) * 8) : zero;
        const lx_half8 px = *(const lx_half8*)(s_p1 + pbase + s_koff[kg]);
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

// a branch's hidden layer: threads 0..99, fp32, one FMA chain per output in ascending k from the bias, then ReLU
__device__ __forceinline__ void lx_hidden(const float* feat, const float* wt, const float* bias, float* s_h, int tid) {
    if (tid < LX_EC) {
        float h = bias[tid];
#pragma unroll 16
        for (int k = 0; k < LX_EB; ++k) h = fmaf(feat[k], wt[k * LX_EC + tid], h);
        s_h[tid] = fmaxf(h, 0.f);
    }
}

__device__ __forceinline__ float lx_readlane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// All tc samples of exit `e` from the hidden units s_h, and the exit's three rows: S[e][b] += (even samples in ascending order) + (odd
// samples in ascending order), lenet5_me_kernel's order and bits.  Called by the whole workgroup (it holds barriers); the caller has a
// barrier between s_h's writes and this.  With `s_row`, wave 0 also leaves the new S1 row there (the caller's barrier publishes it).
__device__ __forceinline__ void lx_exit_samples(const Lenet5MeArgs& a, const SiteArgs& st, const float* wt, const float* bv,
                                                const float* s_h, float2 (*s_tab)[32], double (*s_join)[32], double* s_row, int e, int b, int wave,
                                                int lane) {
    const int C = a.C;
    const bool on = st.kind != BMI_SITE_NONE;
    const uint32_t cl = (uint32_t)min(lane, C - 1);
    float w[LX_EC];      // the classifier column of this lane's class (row k is a uniform base, the class a 32-bit lane offset)
#pragma unroll
    for (int k = 0; k < LX_EC; ++k) w[k] = (wt + k * C)[cl];
    const float bias = bv[cl];
    const float h0 = s_h[lane], h1 = lane < LX_EC - 64 ? s_h[64 + lane] : 0.f;      // units lane and 64 + lane
    const uint64_t eC = (uint64_t)b * LX_EC, eC0 = eC & ~7ull;      // 100 is a multiple of 4 only: the first keep byte starts up to 4 elements early
    const int offC = (int)(eC - eC0), nC = (offC + LX_EC + 7) / 8;
    const int bit = (offC + lane) & 7, byte0 = (offC + lane) >> 3, byte1 = (offC + 64 + lane) >> 3;      // (offC + 64 + lane) & 7 == bit
    double s1 = 0.0, s2 = 0.0, sl = 0.0;

    for (int r0 = 0; r0 < a.tc; r0 += LX_ROUND) {      // r0 is a multiple of 4 and of 2: a sample's wave and parity are those of its row
        const int r1 = min(r0 + LX_ROUND, a.tc);
        if (r0) __syncthreads();                       // the adders are done with the previous round's rows
        for (int it = r0 + wave; it < r1; it += 4) {
            float m0 = h0, m1 = h1;
            if (on) {
                const uint32_t keep = lane < nC ? site_keep8(st, eC0 + 8u * (uint32_t)lane, (uint32_t)(a.t0 + it)) : 0u;
                const uint32_t k0 = __shfl(keep, byte0), k1 = __shfl(keep, byte1);
                m0 = ((k0 >> bit) & 1u) ? h0 * st.scale : 0.f;
                m1 = ((k1 >> bit) & 1u) ? h1 * st.scale : 0.f;
            }
            float z = bias;
#pragma unroll
            for (int k = 0; k < 64; ++k) z = fmaf(lx_readlane(m0, k), w[k], z);
#pragma unroll
            for (int k = 64; k < LX_EC; ++k) z = fmaf(lx_readlane(m1, k - 64), w[k], z);
            float m = lane < C ? z : -INFINITY;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            const float ex = lane < C ? expf(z - m) : 0.f;
            float sum = ex;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
            if (lane < C) s_tab[it - r0][lane] = float2{ex / sum, z};
        }
        __syncthreads();
        if (wave < 2 && lane < C)                      // wave 0: the even samples, wave 1: the odd ones, each in ascending order
            for (int it = r0 + wave; it < r1; it += 2) {
                const float2 v = s_tab[it - r0][lane];
                const double p = (double)v.x;
                s1 += p;
                s2 += p * p;
                sl += (double)v.y;
            }
    }
    if (wave == 1 && lane < 32) {
        s_join[0][lane] = s1;
        s_join[1][lane] = s2;
        s_join[2][lane] = sl;
    }
    __syncthreads();
    if (wave == 0 && lane < C) {
        const size_t i = ((size_t)e * a.B + b) * C + lane;
        const double n1 = a.S1[i] + (s1 + s_join[0][lane]);
        a.S1[i] = n1;
        a.S2[i] += s2 + s_join[1][lane];
        a.SL[i] += sl + s_join[2][lane];
        if (s_row) s_row[lane] = n1;
    }
}

__global__ __launch_bounds__(LX_THREADS, 2) void lenet5_me_exit_kernel(Lenet5MeExitArgs xa) {
    __shared__ __attribute__((aligned(16))) _Float16 s_p1[LX_P1_HALVES];
    __shared__ __attribute__((aligned(16))) _Float16 s_w2[LX_KG * 20 * 8];
    __shared__ float s_img[1024];            // [32][32]: the image with a 2-pixel zero halo
    __shared__ float s_w1[520];              // [20][25] then the 20 biases
    __shared__ int s_koff[LX_KG];
    __shared__ float s_feat[2][LX_EB], s_h[2][LX_EC];      // [exit]
    __shared__ float2 s_tab[LX_ROUND][32];   // a round's (p, z): [sample of the round][class]
    __shared__ double s_join[3][32];
    __shared__ double s_row[32];             // exit 0's S1 row, for the decision

    const Lenet5MeArgs& a = xa.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;

    // ---- stage 0: staging -> conv1 + pool -> ex1conv1 (wave 3) | conv2's fragments into LDS (waves 0..2) -> ex1fc1 -> exit 0's samples ------
    const float* img = a.x + (size_t)b * 784;
    for (int i = tid; i < 1024; i += LX_THREADS) {
        const int r = (i >> 5) - 2, c = (i & 31) - 2;
        s_img[i] = ((unsigned)r < 28u && (unsigned)c < 28u) ? img[r * 28 + c] : 0.f;
    }
    for (int i = tid; i < 520; i += LX_THREADS) s_w1[i] = i < 500 ? a.w1[i] : a.b1[i - 500];
    for (int i = tid; i < LX_P1_HALVES / 8; i += LX_THREADS) ((uint4*)s_p1)[i] = uint4{0u, 0u, 0u, 0u};      // halo and padding channels stay zero
    if (tid < LX_KG) {      // K-group -> offset of its tap and channel group inside the haloed map (group 75: zero weights, any valid offset)
        const int kg = min(tid, LX_KG - 2), tap = kg / 3;
        s_koff[tid] = ((tap / 5) * LX_P1_W + tap % 5) * LX_P1_C + (kg % 3) * 8;
    }
    __syncthreads();
    lx_conv1_pool(s_img, s_w1, s_p1, tid);
    __syncthreads();
    if (wave == 3) lx_exit_conv(s_p1, a.ewf, s_koff, a.eb, lane, s_feat[0]);
    else for (int i = tid; i < LX_KG * 20; i += LX_THREADS - 64) ((uint4*)s_w2)[i] = ((const uint4*)a.w2f)[i];
    __syncthreads();
    lx_hidden(s_feat[0], a.efc1t, a.efb1, s_h[0], tid);
    __syncthreads();
    lx_exit_samples(a, a.site[0], a.elint, a.elinb, s_h[0], s_tab, s_join, s_row, 0, b, wave, lane);
    __syncthreads();

    // ---- the decision: every thread evaluates the rule on exit 0's row, so the return is uniform --------------------------------------
    const double stat = exit_rule_stat(s_row, 1, a.C, 0, 0, (double)a.tc, xa.margin, 0, nullptr);
    if (stat > xa.threshold) {
        if (tid == 0) xa.exit_of_image[b] = 0;
        return;
    }

    // ---- stage 1: conv2 + pool -> fc1 -> exit 1's samples ---------------------------------------------------------------------------
    lx_conv2_pool(s_p1, s_w2, s_koff, a.b2, wave, lane, s_feat[1]);
    __syncthreads();
    lx_hidden(s_feat[1], a.fc1t, a.fb1, s_h[1], tid);
    __syncthreads();
    lx_exit_samples(a, a.site[1], a.fc2t, a.fb2, s_h[1], s_tab, s_join, nullptr, 1, b, wave, lane);
    if (tid == 0) xa.exit_of_image[b] = 1;
}

}  // namespace

int launch_lenet5_me_exit(const Lenet5MeExitArgs& a, hipStream_t s) {
    if (a.m.B < 1 || a.m.tc < 1 || a.m.C < 2 || a.m.C > 32 || !a.m.S1 || !a.m.S2 || !a.m.SL || !a.exit_of_image) return BMI_ERR_INVALID;
    hipLaunchKernelGGL(lenet5_me_exit_kernel, dim3((unsigned)a.m.B), dim3(LX_THREADS), 0, s, a);
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
// The handle of bmi_lenet5_me_create, as lenet5_me.hip defines it (that file stays untouched, so the definition is repeated, token for token)
struct bmi_lenet5_me_s {
    Lenet5MeArgs args;
    bmi_site sites[2];
};

extern "C" int bmi_lenet5_me_forward_exit_staged(bmi_lenet5_me_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed,
                                                 const bmi_exit_rule* rule, double* S1, double* S2, double* SL, int32_t* exit_of_image,
                                                 bmi_stream stream) {
    if (!h || !x_nchw || !rule || !S1 || !S2 || !SL || !exit_of_image || batch < 1 || t_count < 1) return BMI_ERR_INVALID;
    if (rule->criterion != BMI_EXIT_CONFIDENCE && rule->criterion != BMI_EXIT_MARGIN) return BMI_ERR_INVALID;
    if (rule->first_exit != 0) return BMI_ERR_INVALID;
    if (rule->ensemble != 0) return BMI_ERR_UNSUPPORTED;      // only exit 0 is tested, and the ensemble of exits 0..0 is exit 0 itself
    Lenet5MeExitArgs xa;
    Lenet5MeArgs& a = xa.m;
    a = h->args;
    a.x = x_nchw; a.B = batch; a.t0 = 0; a.tc = t_count;
    a.S1 = S1; a.S2 = S2; a.SL = SL; a.logits = nullptr;
    for (int i = 0; i < 2; ++i) a.site[i] = resolve_site(h->sites[i].kind == BMI_SITE_NONE ? nullptr : &h->sites[i], seed, 0);
    xa.threshold = rule->threshold;
    xa.margin = rule->criterion == BMI_EXIT_MARGIN;
    xa.exit_of_image = exit_of_image;
    return launch_lenet5_me_exit(xa, (hipStream_t)stream);
}
