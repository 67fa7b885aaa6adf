// The grid weights and the two separately rounded steps shared by the expansions and folds of the slider (kernels_line.hip) and of the
// gallery patch (kernels_patch.hip).  The bit contracts of both (include/sls_hip.h: mirror symmetry, the fold of the set gradient)
// are statements about exactly these three functions.
#pragma once
#include <hip/hip_runtime.h>

namespace slsk {

// u_i = (q-1-i)/(q-1), t_i = i/(q-1): each ONE division of two exact integers, so u_i = t_{q-1-i} to the bit
__device__ __forceinline__ void line_weights(int i, int q, double& u, double& t) {
    const double den = (double)(q - 1);
    u = (double)(q - 1 - i) / den;
    t = (double)i / den;
}
// u a + t b and acc + w g: products and sum are separate roundings.  A fused multiply-add would round u a + t b differently from
// t b + u a, and the mirror contract needs the two to be the same number.
__device__ __forceinline__ double line_mix(double u, double a, double t, double b) {
#pragma clang fp contract(off)
    const double ua = u * a;
    const double tb = t * b;
    return ua + tb;
}
__device__ __forceinline__ double line_acc(double acc, double w, double g) {
#pragma clang fp contract(off)
    const double wg = w * g;
    return acc + wg;
}

}  // namespace slsk
