// The exit head under matrix scaling (bmi_engine_set_matrix_scaling): the TEMP == 3 instantiations of head_fused_body.h's kernels, in a
// translation unit of their own like the vector-scaling ones of head_fused_vec.hip.
#include "head_fused_body.h"

void launch_head_rt_mat(const HeadArgs& a, hipStream_t s) {
    switch ((a.C + 31) / 32) {
        case 1: launch_rt<1, 3>(a, s); break;
        case 2: launch_rt<2, 3>(a, s); break;
        case 3: launch_rt<3, 3>(a, s); break;
        default: launch_rt<4, 3>(a, s); break;
    }
}

void launch_head_rt_multi_mat(const HeadArgsPack& p, int n, hipStream_t s) {
    switch ((p.a[0].C + 31) / 32) {
        case 1: launch_rt_multi<1, 3>(p, n, s); break;
        case 2: launch_rt_multi<2, 3>(p, n, s); break;
        case 3: launch_rt_multi<3, 3>(p, n, s); break;
        default: launch_rt_multi<4, 3>(p, n, s); break;
    }
}
