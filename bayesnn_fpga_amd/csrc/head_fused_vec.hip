// The exit head under vector scaling (bmi_engine_set_vector_scaling): the TEMP == 2 instantiations of head_fused_body.h's kernels, in a
// translation unit of their own like the tempered ones of head_fused_temp.hip.
#include "head_fused_body.h"

void launch_head_rt_vec(const HeadArgs& a, hipStream_t s) {
    switch ((a.C + 31) / 32) {
        case 1: launch_rt<1, 2>(a, s); break;
        case 2: launch_rt<2, 2>(a, s); break;
        case 3: launch_rt<3, 2>(a, s); break;
        default: launch_rt<4, 2>(a, s); break;
    }
}

void launch_head_rt_multi_vec(const HeadArgsPack& p, int n, hipStream_t s) {
    switch ((p.a[0].C + 31) / 32) {
        case 1: launch_rt_multi<1, 2>(p, n, s); break;
        case 2: launch_rt_multi<2, 2>(p, n, s); break;
        case 3: launch_rt_multi<3, 2>(p, n, s); break;
        default: launch_rt_multi<4, 2>(p, n, s); break;
    }
}
