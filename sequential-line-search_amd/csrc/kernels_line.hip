// Line EUBO, the expected utility of the best of q grid positions on a slider from a to b (include/sls_hip.h "expected utility of the
// best slider position"): the two kernels the line objective adds around the qEUBO pass (capi_path.hip: line_eval_device).  A line is
// expanded into the set (x_0..x_{q-1}) the pass evaluates, and the set gradient is folded back onto the ends by the chain rule.
#include "common.hpp"
#include "kernels.hpp"
#include "line_mix.hpp"   // line_weights, line_mix, line_acc

namespace slsk {

// ONE lane per (n, d), lanes along n: a = anchor[d] (anchored form, the line block has D rows) or trial[n + d ld] (free form, 2D rows),
// b = the block's last D rows; sets[n + (i D + d) lds] = u_i a + t_i b for i = 0..q-1.  No clamp.
__global__ __launch_bounds__(256) void line_expand_kernel(int nlines, int D, int q, const double* __restrict__ trial, long ld,
                                                          const double* __restrict__ anchor, double* __restrict__ sets, long lds) {
    const int n = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
    if (n >= nlines) return;
    const double a = anchor ? anchor[d] : trial[n + (long)d * ld];
    const double b = trial[n + (long)(anchor ? d : D + d) * ld];
    for (int i = 0; i < q; ++i) {
        double u, t;
        line_weights(i, q, u, t);
        sets[n + (long)(i * D + d) * lds] = line_mix(u, a, t, b);
    }
}
void launch_line_expand(hipStream_t s, int nlines, int D, int q, const double* trial, long ld, const double* anchor, double* sets,
                        long lds) {
    if (nlines <= 0) return;
    hipLaunchKernelGGL(line_expand_kernel, dim3((nlines + 255) / 256, D), dim3(256), 0, s, nlines, D, q, trial, ld, anchor, sets, lds);
}

// ONE lane per (n, d): grad_a = sum_i u_i g_i from zero in INCREASING i, grad_b = sum_i t_i g_i from zero in DECREASING i, over the set
// gradient sgrad[n + (i D + d) lds].  The two orders mirror each other (u_i = t_{q-1-i}): the line with its ends swapped has the reversed
// set gradient and adds, for its grad_b, the same products in the same order as this line's grad_a -- the blocks swap bit for bit.
// Free form: grad[n + d ldo] = grad_a, grad[n + (D + d) ldo] = grad_b; anchored: grad[n + d ldo] = grad_b alone.
__global__ __launch_bounds__(256) void line_fold_kernel(int nlines, int D, int q, int anchored, const double* __restrict__ sgrad, long lds,
                                                        double* __restrict__ grad, long ldo) {
    const int n = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
    if (n >= nlines) return;
    double ga = 0.0, gb = 0.0;
    for (int i = 0; i < q; ++i) {
        const int j = q - 1 - i;
        double ui, ti, uj, tj;
        line_weights(i, q, ui, ti);
        line_weights(j, q, uj, tj);
        ga = line_acc(ga, ui, sgrad[n + (long)(i * D + d) * lds]);
        gb = line_acc(gb, tj, sgrad[n + (long)(j * D + d) * lds]);
    }
    if (anchored) {
        grad[n + (long)d * ldo] = gb;
    } else {
        grad[n + (long)d * ldo] = ga;
        grad[n + (long)(D + d) * ldo] = gb;
    }
}
void launch_line_fold(hipStream_t s, int nlines, int D, int q, bool anchored, const double* sgrad, long lds, double* grad, long ldo) {
    if (nlines <= 0) return;
    hipLaunchKernelGGL(line_fold_kernel, dim3((nlines + 255) / 256, D), dim3(256), 0, s, nlines, D, q, anchored ? 1 : 0, sgrad, lds, grad,
                       ldo);
}

}  // namespace slsk
