// Gallery EUBO, the expected utility of the best cell of a qs x qt grid on the bilinear patch spanned by four corner designs
// (include/sls_hip.h "expected utility of the best gallery cell"): the two kernels the patch objective adds around the qEUBO pass
// (capi_path.hip: patch_eval_device).  A patch is expanded into the set (x_0..x_{qs qt - 1}) the pass evaluates, option k = i + qs j,
// and the set gradient is folded back onto the corners by the chain rule.  Weights and roundings are those of the slider
// (line_mix.hpp): both kernels are the line's, one dimension up.
#include "common.hpp"
#include "kernels.hpp"
#include "line_mix.hpp"   // line_weights, line_mix, line_acc

namespace slsk {

// The rows of a patch's corners in its candidate-major block: c00, c10, c01, c11 at rows 0, D, 2D, 3D (free form), or c10, c01, c11 at
// rows 0, D, 2D with c00 = anchor[d] (anchored form).  corner c = 0..3 in that order; the anchored c00 has no row.
__device__ __forceinline__ long patch_row(int c, int D, int d, bool anchored) { return (long)(anchored ? c - 1 : c) * D + d; }

// ONE lane per (n, d), lanes along n (consecutive lanes read and write consecutive doubles of every row).  Cell (i, j):
// lo = u_i c00 + s_i c10, hi = u_i c01 + s_i c11, x = v_j lo + t_j hi -> sets[n + ((i + qs j) D + d) lds].  No clamp.
__global__ __launch_bounds__(256) void patch_expand_kernel(int npatches, int D, int qs, int qt, const double* __restrict__ trial, long ld,
                                                           const double* __restrict__ anchor, double* __restrict__ sets, long lds) {
    const int n = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
    if (n >= npatches) return;
    const bool anchored = anchor != nullptr;
    const double c00 = anchored ? anchor[d] : trial[n + patch_row(0, D, d, false) * ld];
    const double c10 = trial[n + patch_row(1, D, d, anchored) * ld];
    const double c01 = trial[n + patch_row(2, D, d, anchored) * ld];
    const double c11 = trial[n + patch_row(3, D, d, anchored) * ld];
    for (int i = 0; i < qs; ++i) {
        double u, s;
        line_weights(i, qs, u, s);
        const double lo = line_mix(u, c00, s, c10);
        const double hi = line_mix(u, c01, s, c11);
        for (int j = 0; j < qt; ++j) {
            double v, t;
            line_weights(j, qt, v, t);
            sets[n + (long)((i + qs * j) * D + d) * lds] = line_mix(v, lo, t, hi);
        }
    }
}
void launch_patch_expand(hipStream_t s, int npatches, int D, int qs, int qt, const double* trial, long ld, const double* anchor,
                         double* sets, long lds) {
    if (npatches <= 0) return;
    hipLaunchKernelGGL(patch_expand_kernel, dim3((npatches + 255) / 256, D), dim3(256), 0, s, npatches, D, qs, qt, trial, ld, anchor, sets,
                       lds);
}

// qs >= 2 and qs qt <= SLS_QEUBO_MAX_OPTIONS = 16: at most 8 rows
constexpr int PATCH_MAX_ROWS = 8;

// ONE lane per (n, d).  Per grid row j the line's fold along i: A_j = sum_i u_i g_{i + qs j} from zero in INCREASING i, B_j =
// sum_i s_i g_{i + qs j} from zero in DECREASING i.  Then the same fold along j: grad_c00 = sum_j v_j A_j and grad_c10 = sum_j v_j B_j
// in increasing j, grad_c01 = sum_j t_j A_j and grad_c11 = sum_j t_j B_j in DECREASING j.  Either mirror reverses the set gradient
// along its axis bit for bit, and the reversed order adds the same products in the same order: the gradient blocks swap bit for bit.
// The row sums stay in registers (every index below is a constant after unrolling); a set gradient entry is read twice, once for each
// direction along i, as line_fold reads it.
// Free form: grad rows 0, D, 2D, 3D = c00, c10, c01, c11; anchored: rows 0, D, 2D = c10, c01, c11.
__global__ __launch_bounds__(256) void patch_fold_kernel(int npatches, int D, int qs, int qt, int anchored,
                                                         const double* __restrict__ sgrad, long lds, double* __restrict__ grad, long ldo) {
    const int n = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
    if (n >= npatches) return;
    double A[PATCH_MAX_ROWS], B[PATCH_MAX_ROWS];
#pragma unroll
    for (int j = 0; j < PATCH_MAX_ROWS; ++j) {
        A[j] = 0.0;
        B[j] = 0.0;
        if (j >= qt) continue;
        const double* g = sgrad + n + (long)(qs * j * D + d) * lds;   // option i of row j at g[i D lds]
        for (int i = 0; i < qs; ++i) {
            const int r = qs - 1 - i;
            double ui, si, ur, sr;
            line_weights(i, qs, ui, si);
            line_weights(r, qs, ur, sr);
            A[j] = line_acc(A[j], ui, g[(long)i * D * lds]);
            B[j] = line_acc(B[j], sr, g[(long)r * D * lds]);
        }
    }
    double g00 = 0.0, g10 = 0.0, g01 = 0.0, g11 = 0.0;
#pragma unroll
    for (int j = 0; j < PATCH_MAX_ROWS; ++j) {
        if (j >= qt) continue;
        double v, t;
        line_weights(j, qt, v, t);
        g00 = line_acc(g00, v, A[j]);
        g10 = line_acc(g10, v, B[j]);
    }
#pragma unroll
    for (int j = PATCH_MAX_ROWS - 1; j >= 0; --j) {
        if (j >= qt) continue;
        double v, t;
        line_weights(j, qt, v, t);
        g01 = line_acc(g01, t, A[j]);
        g11 = line_acc(g11, t, B[j]);
    }
    if (!anchored) grad[n + patch_row(0, D, d, false) * ldo] = g00;
    grad[n + patch_row(1, D, d, anchored) * ldo] = g10;
    grad[n + patch_row(2, D, d, anchored) * ldo] = g01;
    grad[n + patch_row(3, D, d, anchored) * ldo] = g11;
}
void launch_patch_fold(hipStream_t s, int npatches, int D, int qs, int qt, bool anchored, const double* sgrad, long lds, double* grad,
                       long ldo) {
    if (npatches <= 0) return;
    hipLaunchKernelGGL(patch_fold_kernel, dim3((npatches + 255) / 256, D), dim3(256), 0, s, npatches, D, qs, qt, anchored ? 1 : 0, sgrad,
                       lds, grad, ldo);
}

}  // namespace slsk
