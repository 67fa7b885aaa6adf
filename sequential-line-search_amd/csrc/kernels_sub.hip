// Search over affine subspaces (include/sls_hip.h "maximisation over affine subspaces"): the two kernels the *_sub entry points add
// around an evaluation that stays what it is (sub_maps.hpp: sub_eval).  A column's variables z in R^d are expanded
// into the point x = c_k + A_k z in R^D the evaluation reads, and the gradient in x is folded back onto z by the chain rule.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

namespace {

constexpr int SUB_LANES = 256;   // lanes of a block, along the columns n: every z, X and gradient access is coalesced
constexpr int SUB_TILE = 8;      // rows of x (expand) / variables of z (fold) one lane carries: the operand block is read D / 8 (d / 8) times

// acc + a v: the product and the sum are separate roundings, as the contract states them
__device__ __forceinline__ double sub_acc(double acc, double a, double v) {
#pragma clang fp contract(off)
    const double av = a * v;
    return acc + av;
}
// the map of column n: map_of_column[live ? live[n] : n], 0 without a table
__device__ __forceinline__ int sub_map_of(const SubMaps& m, const int* __restrict__ live, int n) {
    if (!m.map_of_column) return 0;
    return m.map_of_column[live ? live[n] : n];
}

}  // namespace

// ONE lane per (n, tile of 8 rows r): x_r = c_r, then x_r = x_r + A_rj z_j for j = 0..d-1 in increasing order.  The lanes of a wavefront
// that share a map read the same 8 consecutive doubles of A per j (one 64-byte line, broadcast); lanes with different maps read their own.
// The columns ncols <= n < npad -- the rest of the last 128-wide tile the evaluation reads -- get the centre of the box, as host_to_cm
// pads the plain routes' blocks: no tile ever holds memory that was never written.
__global__ __launch_bounds__(SUB_LANES) void sub_expand_kernel(SubMaps m, int ncols, int npad, const int* __restrict__ live,
                                                               const double* __restrict__ z, long ld, double* __restrict__ X, long ldx) {
    const int n = blockIdx.x * SUB_LANES + threadIdx.x;
    if (n >= npad) return;
    const int r0 = blockIdx.y * SUB_TILE;
    const int D = m.D, d = m.d;
    if (n >= ncols) {
#pragma unroll
        for (int i = 0; i < SUB_TILE; ++i)
            if (r0 + i < D) X[n + (long)(r0 + i) * ldx] = 0.5;
        return;
    }
    const int k = sub_map_of(m, live, n);
    const double* __restrict__ A = m.A + (size_t)k * D * d;
    const double* __restrict__ c = m.c + (size_t)k * D;
    double x[SUB_TILE];
#pragma unroll
    for (int i = 0; i < SUB_TILE; ++i) x[i] = r0 + i < D ? c[r0 + i] : 0.0;
    for (int j = 0; j < d; ++j) {
        const double zj = z[n + (long)j * ld];
        const double* __restrict__ Aj = A + (size_t)j * D + r0;
#pragma unroll
        for (int i = 0; i < SUB_TILE; ++i)
            if (r0 + i < D) x[i] = sub_acc(x[i], Aj[i], zj);
    }
#pragma unroll
    for (int i = 0; i < SUB_TILE; ++i)
        if (r0 + i < D) X[n + (long)(r0 + i) * ldx] = x[i];
}
void launch_sub_expand(hipStream_t s, const SubMaps& m, int ncols, const int* live, const double* z, long ld, double* X, long ldx) {
    if (ncols <= 0) return;
    const int npad = (int)std::min<long>((ncols + 127) / 128 * 128, ldx);   // never past the block's leading dimension
    hipLaunchKernelGGL(sub_expand_kernel, dim3((npad + SUB_LANES - 1) / SUB_LANES, (m.D + SUB_TILE - 1) / SUB_TILE), dim3(SUB_LANES), 0, s, m,
                       ncols, npad, live, z, ld, X, ldx);
}

// ONE lane per (n, tile of 8 variables j): gz_j = 0, then gz_j = gz_j + A_rj gx_r for r = 0..D-1 in increasing order.
__global__ __launch_bounds__(SUB_LANES) void sub_fold_kernel(SubMaps m, int ncols, const int* __restrict__ live,
                                                             const double* __restrict__ gx, long ldx, double* __restrict__ gz, long ldo) {
    const int n = blockIdx.x * SUB_LANES + threadIdx.x;
    if (n >= ncols) return;
    const int j0 = blockIdx.y * SUB_TILE;
    const int D = m.D, d = m.d;
    const int k = sub_map_of(m, live, n);
    const double* __restrict__ A = m.A + (size_t)k * D * d;
    double g[SUB_TILE];
#pragma unroll
    for (int i = 0; i < SUB_TILE; ++i) g[i] = 0.0;
    for (int r = 0; r < D; ++r) {
        const double gr = gx[n + (long)r * ldx];
#pragma unroll
        for (int i = 0; i < SUB_TILE; ++i)
            if (j0 + i < d) g[i] = sub_acc(g[i], A[r + (size_t)(j0 + i) * D], gr);
    }
#pragma unroll
    for (int i = 0; i < SUB_TILE; ++i)
        if (j0 + i < d) gz[n + (long)(j0 + i) * ldo] = g[i];
}
void launch_sub_fold(hipStream_t s, const SubMaps& m, int ncols, const int* live, const double* gx, long ldx, double* gz, long ldo) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL(sub_fold_kernel, dim3((ncols + SUB_LANES - 1) / SUB_LANES, (m.d + SUB_TILE - 1) / SUB_TILE), dim3(SUB_LANES), 0, s, m,
                       ncols, live, gx, ldx, gz, ldo);
}

}  // namespace slsk
