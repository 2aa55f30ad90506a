// The decision statistic of the staged early exit (bmi_exit_rule), shared by the rule itself (misc_kernels.hip: exit_rule_decide_kernel) and
// by the record of it (exit_policy.hip: bmi_exit_stat_record), so that both translation units compile the same function.
#pragma once
#include <cstddef>

// float64 as the header states it: p_c = S1[e][b][c] / t (ensemble: the exits 0..e's p_c summed in exit order, / (e + 1)); confidence =
// max_c p_c, margin = top-1 minus top-2 (0 on a tie).  No contraction into fma: a numpy restatement gets the same statistic.  w (ensemble
// only; row e of the weights of bmi_engine_set_ensemble_weights, null: the equal mean, the expression as it was): p_c = sum_{x<=e} w[x] *
// (S1[x][b][c] / t), each product rounded, added in exit order from 0.0.
__device__ double exit_rule_stat(const double* __restrict__ S1, int B, int C, int b, int e, double t, int margin, int ensemble,
                                 const double* __restrict__ w) {
#pragma clang fp contract(off)
    double m1 = -1.0, m2 = -1.0;
    for (int c = 0; c < C; ++c) {
        double p;
        if (ensemble && w) {
            p = 0.0;
            for (int x = 0; x <= e; ++x) p = p + w[x] * (S1[((size_t)x * B + b) * C + c] / t);
        } else if (ensemble) {
            double acc = 0.0;
            for (int x = 0; x <= e; ++x) acc = acc + S1[((size_t)x * B + b) * C + c] / t;
            p = acc / (double)(e + 1);
        } else {
            p = S1[((size_t)e * B + b) * C + c] / t;
        }
        if (p > m1) { m2 = m1; m1 = p; }
        else if (p > m2) m2 = p;
    }
    return margin ? m1 - (C > 1 ? m2 : 0.0) : m1;
}
