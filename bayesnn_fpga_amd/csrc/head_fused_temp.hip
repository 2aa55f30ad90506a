// The exit head under temperature scaling (bmi_engine_set_temperature): the TEMP = true instantiations of head_fused_body.h's kernels,
// in a translation unit of their own so that they compile beside the untempered ones of head_fused.hip instead of behind them.
#include "head_fused_body.h"

void launch_head_rt_temp(const HeadArgs& a, hipStream_t s) {
    switch ((a.C + 31) / 32) {
        case 1: launch_rt<1, 1>(a, s); break;
        case 2: launch_rt<2, 1>(a, s); break;
        case 3: launch_rt<3, 1>(a, s); break;
        default: launch_rt<4, 1>(a, s); break;
    }
}

void launch_head_rt_multi_temp(const HeadArgsPack& p, int n, hipStream_t s) {
    switch ((p.a[0].C + 31) / 32) {
        case 1: launch_rt_multi<1, 1>(p, n, s); break;
        case 2: launch_rt_multi<2, 1>(p, n, s); break;
        case 3: launch_rt_multi<3, 1>(p, n, s); break;
        default: launch_rt_multi<4, 1>(p, n, s); break;
    }
}
