// Exit head, fused: relu -> global average pool -> [site] -> Linear -> [site on the logits] -> softmax -> T-sample moments
// in ONE kernel per exit (ex{1,2,3}linear / linear with their avg_pool2d / exit dropout, SA/models/resnet18/resnet18.py:
// 309-314, :320-325, :331-335, :338-344; the softmax and the np.average over the passes of FullAnalysis._get_output,
// SA/train/results_analyzer.py:242-248).  Round 1 ran this as pool_mask + linear_softmax + a per-sample [E][N][C]
// probability / logit scratch + a moments kernel (9 launches per chunk); here nothing per-sample is materialised.
//
//   workgroup   = one image b of the batch x one group of 32 of the launch's samples, 256 threads (one workgroup per image
//                 walking all groups left 250 workgroups of latency-bound work on 256 CUs: 2x slower than the three kernels
//                 it replaced); the groups of an image leave float64 partial sums in a workspace scratch that head_join_kernel
//                 adds into S1/S2/SL[b][:] in group order (round 3: bit-reproducible; round 2 used hardware float64 atomics,
//                 whose order varied from run to run).
//   phase A     = pooling, coalesced: wave w pools columns (samples) w, w+4, .. of the group, lane = one 8-channel group
//                 (16 B per pixel row: 64 lanes cover a 512-channel row = 1 KB contiguous), ReLU + mean in fp32, the
//                 feature-side site (MC dropout / Masksembles1D on the [B, K] tensor), then fp32 into LDS
//                 feat[32 samples][KC] with the 16-byte chunks XOR-swizzled by the sample index.
//   phase B     = logits[class][sample] on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), classes on the row axis, the 32
//                 samples on the column axis; the 4 waves split K, partial sums meet in LDS.
//   finalize    = wave 0: bias, [dropout on the logits], softmax in registers (one cross-half shuffle) -> LDS [class][sample];
//                 then all waves: the sums over the group's samples of p, p^2 and logit by WAVEFRONT SHUFFLE REDUCTION in
//                 float64 (32 lanes = 32 samples of one class; the reference averages in float64; per-sample values are
//                 bit-identical however the samples are chunked or sharded, so only the float64 summation order depends
//                 on it: <= 1e-13 relative).
#include "head_fused_body.h"

// the tempered instantiations (HeadArgs::inv_tau != 0): head_fused_temp.hip
void launch_head_rt_temp(const HeadArgs& a, hipStream_t s);
void launch_head_rt_multi_temp(const HeadArgsPack& p, int n, hipStream_t s);
// the vector-scaling instantiations (HeadArgs::vec_scale != null): head_fused_vec.hip
void launch_head_rt_vec(const HeadArgs& a, hipStream_t s);
void launch_head_rt_multi_vec(const HeadArgsPack& p, int n, hipStream_t s);
// the matrix-scaling instantiations (HeadArgs::mat != null): head_fused_mat.hip
void launch_head_rt_mat(const HeadArgs& a, hipStream_t s);
void launch_head_rt_multi_mat(const HeadArgsPack& p, int n, hipStream_t s);

// Joins the per-group partial sums of an image in GROUP ORDER into the caller's accumulators: with hardware float64 atomics the
// groups met in whatever order the workgroups finished, and the last bit of the sums of more than 64 samples changed from run to
// run (round-2 verdict); an ordered "last arriver adds all" reduction inside the head kernel needed agent-scope fences that doubled
// it.  This is one more launch of B x C threads per exit and chunk (~3 us), only when a launch carries more than 32 samples.
// SH (or null): the [groups][B] entropy plane behind the moment planes joins the same way, by the thread of class 0 of each image.
__global__ __launch_bounds__(256) void head_join_kernel(const double* __restrict__ part, int groups, int B, int C, const int* imap, int Bc,
                                                        double* S1, double* S2, double* SL, double* SH) {
    const int rows = imap ? Bc : B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * C) return;
    const int row = i / C, c = i - row * C;
    const int b = imap ? imap[row] : row;
    const size_t o = (size_t)b * C + c, plane = (size_t)B * C;
    double s1 = 0.0, s2 = 0.0, sl = 0.0;
    for (int g = 0; g < groups; ++g) {
        const double* pp = part + (size_t)g * 3 * plane + o;
        s1 += pp[0]; s2 += pp[plane]; sl += pp[2 * plane];
    }
    S1[o] += s1; S2[o] += s2; SL[o] += sl;
    if (SH && c == 0) {
        const double* ph = part + (size_t)groups * 3 * plane + b;
        double sh = 0.0;
        for (int g = 0; g < groups; ++g) sh += ph[(size_t)g * B];
        SH[b] += sh;
    }
}

struct HeadJoinPack {
    const double* part[BMI_HEAD_PACK_MAX];
    double *S1[BMI_HEAD_PACK_MAX], *S2[BMI_HEAD_PACK_MAX], *SL[BMI_HEAD_PACK_MAX], *SH[BMI_HEAD_PACK_MAX];
};
__global__ __launch_bounds__(256) void head_join_multi_kernel(HeadJoinPack p, int groups, int B, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int z = blockIdx.y;
    const size_t o = (size_t)i, plane = (size_t)B * C;
    double s1 = 0.0, s2 = 0.0, sl = 0.0;
    for (int g = 0; g < groups; ++g) {
        const double* pp = p.part[z] + (size_t)g * 3 * plane + o;
        s1 += pp[0]; s2 += pp[plane]; sl += pp[2 * plane];
    }
    p.S1[z][o] += s1; p.S2[z][o] += s2; p.SL[z][o] += sl;
    if (p.SH[z] && i % C == 0) {
        const int b = i / C;
        const double* ph = p.part[z] + (size_t)groups * 3 * plane + b;
        double sh = 0.0;
        for (int g = 0; g < groups; ++g) sh += ph[(size_t)g * B];
        p.SH[z][b] += sh;
    }
}


static int head_prepare(HeadArgs& a) {
    const int groups = (a.tc + 31) / 32;
    if (groups <= 1) a.part = nullptr;             // one group per image: the workgroup adds into S1 / S2 / SL itself
    if (!a.in || !a.w || !a.bias) return BMI_ERR_INVALID;
    if (!a.S1 || !a.S2 || !a.SL) { if (!a.logits) return BMI_ERR_INVALID; a.S1 = a.S2 = a.SL = a.SH = nullptr; a.part = nullptr; }     // logits only
    if (a.B <= 0 || a.tc <= 0 || a.in_mod <= 0 || a.HW <= 0 || a.C <= 0 || a.in_kind < 0 || a.in_kind > 4) return BMI_ERR_INVALID;
    if (a.in_mod != a.B && a.in_mod != a.B * a.tc) return BMI_ERR_INVALID;
    if (a.imap && (a.Bc <= 0 || a.Bc > a.B)) return BMI_ERR_INVALID;
    if (!(a.inv_tau >= 0.f) || a.inv_tau > 3.0e38f) return BMI_ERR_INVALID;       // 0: off; else a finite positive 1 / tau
    if ((a.vec_scale != nullptr) != (a.vec_bias != nullptr) || (a.vec_scale && a.inv_tau != 0.f)) return BMI_ERR_INVALID;   // at most one map (Calibration::check's rule, on the kernel's own arguments)
    if ((a.mat != nullptr) != (a.mat_bias != nullptr) || (a.mat && (a.inv_tau != 0.f || a.vec_scale))) return BMI_ERR_INVALID;
    if (a.K % 32 != 0 || a.C > 128) return BMI_ERR_UNSUPPORTED;
    if (a.site_logits.kind != BMI_SITE_NONE && a.site_logits.kind != BMI_SITE_ELEMENTWISE) return BMI_ERR_UNSUPPORTED;
    return BMI_OK;
}

int launch_head_fused(const HeadArgs& a_in, hipStream_t s) {
    HeadArgs a = a_in;
    const int groups = (a.tc + 31) / 32;
    const int rcp = head_prepare(a);
    if (rcp != BMI_OK) return rcp;
    if (a.mat) launch_head_rt_mat(a, s);
    else if (a.vec_scale) launch_head_rt_vec(a, s);
    else if (a.inv_tau != 0.f) launch_head_rt_temp(a, s);
    else
        switch ((a.C + 31) / 32) {
            case 1: launch_rt<1, 0>(a, s); break;
            case 2: launch_rt<2, 0>(a, s); break;
            case 3: launch_rt<3, 0>(a, s); break;
            default: launch_rt<4, 0>(a, s); break;
        }
    BMI_CHECK_LAUNCH();
    if (a.part) {
        const int n = (a.imap ? a.Bc : a.B) * a.C;
        hipLaunchKernelGGL(head_join_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.part, groups, a.B, a.C, a.imap, a.Bc, a.S1,
                           a.S2, a.SL, a.SH);
        BMI_CHECK_LAUNCH();
    }
    return BMI_OK;
}

// n heads in one launch (n <= BMI_HEAD_PACK_MAX); BMI_ERR_UNSUPPORTED when the pack is not uniform (the caller launches them one by one).
// Every head needs its OWN partial-sum scratch (`part`): they run concurrently.
int launch_head_fused_multi(const HeadArgs* list, int n, hipStream_t s) {
    if (!list || n < 1 || n > BMI_HEAD_PACK_MAX) return BMI_ERR_INVALID;
    if (n == 1) return launch_head_fused(list[0], s);
    HeadArgsPack p;
    for (int i = 0; i < n; ++i) {
        p.a[i] = list[i];
        const int rcp = head_prepare(p.a[i]);
        if (rcp != BMI_OK) return rcp;
        const HeadArgs &x = p.a[i], &y = p.a[0];
        if (x.imap || x.C != y.C || x.in_kind != y.in_kind || x.B != y.B || x.tc != y.tc || (x.part != nullptr) != (y.part != nullptr) ||
            (x.S1 != nullptr) != (y.S1 != nullptr) || (x.SH != nullptr) != (y.SH != nullptr) || (x.inv_tau != 0.f) != (y.inv_tau != 0.f) ||
            (x.vec_scale != nullptr) != (y.vec_scale != nullptr) || (x.mat != nullptr) != (y.mat != nullptr))
            return BMI_ERR_UNSUPPORTED;
        for (int j = 0; j < i; ++j)
            if (x.part && x.part == p.a[j].part) return BMI_ERR_INVALID;
    }
    for (int i = n; i < BMI_HEAD_PACK_MAX; ++i) p.a[i] = p.a[0];
    const HeadArgs& a = p.a[0];
    if (a.mat) launch_head_rt_multi_mat(p, n, s);
    else if (a.vec_scale) launch_head_rt_multi_vec(p, n, s);
    else if (a.inv_tau != 0.f) launch_head_rt_multi_temp(p, n, s);
    else
        switch ((a.C + 31) / 32) {
            case 1: launch_rt_multi<1, 0>(p, n, s); break;
            case 2: launch_rt_multi<2, 0>(p, n, s); break;
            case 3: launch_rt_multi<3, 0>(p, n, s); break;
            default: launch_rt_multi<4, 0>(p, n, s); break;
        }
    BMI_CHECK_LAUNCH();
    if (a.part) {
        HeadJoinPack j;
        for (int i = 0; i < BMI_HEAD_PACK_MAX; ++i) {
            const HeadArgs& x = p.a[i < n ? i : 0];
            j.part[i] = x.part; j.S1[i] = x.S1; j.S2[i] = x.S2; j.SL[i] = x.SL; j.SH[i] = x.SH;
        }
        const int groups = (a.tc + 31) / 32, m = a.B * a.C;
        hipLaunchKernelGGL(head_join_multi_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)n), dim3(256), 0, s, j, groups, a.B, a.C);
        BMI_CHECK_LAUNCH();
    }
    return BMI_OK;
}
