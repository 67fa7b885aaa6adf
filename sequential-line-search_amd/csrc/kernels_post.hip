// Joint posterior of the latent function at M query points (sls_gp_predict_cov, sls_gp_sample_posterior; capi_post.hip):
//   Sigma = K(Xs, Xs) - V V^T with V = K* L^-T           (post_cov_kernel, one workgroup per lower 128 x 128 tile)
//   F     = mu 1^T + chol(Sigma + j I) Z                 (normal_fill_kernel for Z; the products run on kernels_tri.hip)
// and the counter-based normal generator behind the samples (Philox4x64-10 + Box-Muller, also exported as sls_random_normal).
#include "gemm_f64.hpp"
#include "kernels.hpp"

namespace slsk {

// One lower tile (tm >= tn) of Sigma per workgroup, enumerated row by row as gram_sym_kernel's lower_only path.  Both contractions
// share ONE accumulator: the Dp-contraction x~_i . x~_j runs first, the epilogue of that pass turns it in place into -k(x_i, x_j)
// (q = 0 on the diagonal), and the Kv-contraction V V^T then accumulates on top of it, so the tile leaves the k loop as
// -(k - V V^T) and is written, negated, with its mirror.  No second set of 128 accumulator registers, no LDS copy of the prior
// and no HBM pass over K(Xs, Xs).  Diagonal tiles write their lower half and mirror it: C is exactly symmetric.
template <bool MATERN>
__global__ __launch_bounds__(256, 2) void post_cov_kernel(const double* __restrict__ XsT, long ldx, int Dp, const double* __restrict__ ns,
                                                          const double* __restrict__ V, const double* __restrict__ V2, long ldv,
                                                          int Kv, int Mp, int M, double a, double* __restrict__ C) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    const int nt = Mp / GEMM_BM;
    const int t = xcd_remap(blockIdx.x, nt * (nt + 1) / 2);
    int tm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (tm * (tm + 1) / 2 > t) --tm;
    while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
    const int tn = t - tm * (tm + 1) / 2;
    const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
    Acc acc;
    acc.zero();
    gemm_tile_mc(acc, XsT + m0, ldx, XsT + n0, ldx, 0, Dp, lds);
    double nm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) nm[i] = ns[m0 + acc_m(i)];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gj = n0 + acc_n(j, r);
            const double nj = ns[gj];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int gi = m0 + acc_m(i);
                double q = nm[i] + nj - 2.0 * acc.v[i][j][r];
                q = (q < 0.0 || gi == gj) ? 0.0 : q;
                double k, c;
                kernel_kc(MATERN ? SLS_KERNEL_ARD_MATERN52 : SLS_KERNEL_ARD_SQUARED_EXPONENTIAL, a, q, k, c);
                acc.v[i][j][r] = -k;
            }
        }
    gemm_tile_mc(acc, V + m0, ldv, V2 + n0, ldv, 0, Kv, lds);   // V2 == V: V V^T; a Laplace handle: V (V T)^T
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = m0 + acc_m(i), gj = n0 + acc_n(j, r);
                double v = -acc.v[i][j][r];
                if (gi >= M || gj >= M) v = gi == gj ? 1.0 : 0.0;   // padding candidates (0.5 upstream): identity, for potrf on Mp
                if (gi < gj) continue;                              // upper half of a diagonal tile: written as the mirror below
                C[(long)gi + (long)gj * Mp] = v;
                if (gi != gj) C[(long)gj + (long)gi * Mp] = v;
            }
}

void launch_post_cov(hipStream_t s, const double* XsT, long ldx, int Dp, const double* ns, const double* V, long ldv, int Kv, int Mp,
                     int M, KernelSpec ks, double* C, const double* V2) {
    if (!V2) V2 = V;
    ensure_dyn_lds((const void*)post_cov_kernel<false>, GEMM_LDS_BYTES);
    ensure_dyn_lds((const void*)post_cov_kernel<true>, GEMM_LDS_BYTES);
    const int nt = Mp / GEMM_BM;
    const dim3 grid(nt * (nt + 1) / 2);
    if (ks.kernel == SLS_KERNEL_ARD_MATERN52)
        hipLaunchKernelGGL(post_cov_kernel<true>, grid, dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, XsT, ldx, Dp, ns, V, V2, ldv, Kv, Mp, M, ks.a, C);
    else
        hipLaunchKernelGGL(post_cov_kernel<false>, grid, dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, XsT, ldx, Dp, ns, V, V2, ldv, Kv, Mp, M, ks.a, C);
}

// The same Sigma with the prior term from the raw coordinate differences (gram_direct_form, kernels.hpp): thread = entry (i, j) of the
// lower triangle, written with its mirror.  Xs[d + i*D]: the M raw query points.
__global__ __launch_bounds__(256) void post_cov_direct_kernel(const double* __restrict__ Xs, int D, const double* __restrict__ inv_ell,
                                                              const double* __restrict__ V, const double* __restrict__ V2, long ldv,
                                                              int Kv, int Mp, int M, int kernel, double a, double* __restrict__ C) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= Mp || i < j) return;
    double v;
    if (i >= M || j >= M) {
        v = i == j ? 1.0 : 0.0;
    } else {
        double q = 0.0;
        if (i != j)
            for (int d = 0; d < D; ++d) {
                const double t = (Xs[d + (long)i * D] - Xs[d + (long)j * D]) * inv_ell[d];
                q = fma(t, t, q);
            }
        double k, c;
        kernel_kc(kernel, a, q, k, c);
        double vv = 0.0;
        for (int kk = 0; kk < Kv; ++kk) vv = fma(V[i + (long)kk * ldv], V2[j + (long)kk * ldv], vv);
        v = k - vv;
    }
    C[(long)i + (long)j * Mp] = v;
    if (i != j) C[(long)j + (long)i * Mp] = v;
}
void launch_post_cov_direct(hipStream_t s, const double* Xs, int D, const double* inv_ell, const double* V, long ldv, int Kv, int Mp,
                            int M, KernelSpec ks, double* C, const double* V2) {
    if (!V2) V2 = V;
    hipLaunchKernelGGL(post_cov_direct_kernel, dim3((Mp + 255) / 256, Mp), dim3(256), 0, s, Xs, D, inv_ell, V, V2, ldv, Kv, Mp, M, ks.kernel,
                       ks.a, C);
}

// ---- Philox4x64-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) ----
__device__ __forceinline__ void philox4x64_10(unsigned long long (&x)[4], unsigned long long k0, unsigned long long k1) {
    constexpr unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    constexpr unsigned long long W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += W0;
            k1 += W1;
        }
        const unsigned long long hi0 = __umul64hi(M0, x[0]), lo0 = M0 * x[0];
        const unsigned long long hi1 = __umul64hi(M1, x[2]), lo1 = M1 * x[2];
        const unsigned long long y0 = hi1 ^ x[1] ^ k0, y2 = hi0 ^ x[3] ^ k1;
        x[0] = y0;
        x[1] = lo1;
        x[2] = y2;
        x[3] = lo0;
    }
}

// normal number t of stream `seed` (kernels.hpp: launch_normal_fill)
__device__ __forceinline__ double philox_normal(unsigned long long seed, unsigned long long t) {
    unsigned long long x[4] = {t >> 2, 0ull, 0ull, 0ull};
    philox4x64_10(x, seed, 0ull);
    const int pair = (int)(t >> 1) & 1;
    const unsigned long long x0 = pair ? x[2] : x[0], x1 = pair ? x[3] : x[1];
    const double u0 = ((double)(x0 >> 11) + 0.5) * 0x1p-53;
    const double u1 = ((double)(x1 >> 11) + 0.5) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u0));
    const double th = 6.283185307179586 * u1;   // 2 pi, rounded as numpy's 2 * np.pi
    return (t & 1) ? r * sin(th) : r * cos(th);
}

// one thread per element of Zt, samples fastest (coalesced stores); each thread runs the Philox block of its own number
__global__ __launch_bounds__(256) void normal_fill_kernel(unsigned long long seed, long s0, int sc, int Scp, int M, int Mp,
                                                          double* __restrict__ Zt, long ldz) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)Scp * Mp) return;
    const int sl = (int)(idx % Scp), j = (int)(idx / Scp);
    double z = 0.0;
    if (sl < sc && j < M) z = philox_normal(seed, (unsigned long long)(s0 + sl) * (unsigned long long)M + (unsigned long long)j);
    Zt[sl + (long)j * ldz] = z;
}
void launch_normal_fill(hipStream_t s, unsigned long long seed, long s0, int sc, int Scp, int M, int Mp, double* Zt, long ldz) {
    const long n = (long)Scp * Mp;
    hipLaunchKernelGGL(normal_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, s0, sc, Scp, M, Mp, Zt, ldz);
}

__global__ __launch_bounds__(256) void random_normal_kernel(unsigned long long seed, long offset, long n, double* __restrict__ out) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    out[i] = philox_normal(seed, (unsigned long long)(offset + i));
}
void launch_random_normal(hipStream_t s, unsigned long long seed, long offset, long n, double* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(random_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, offset, n, out);
}

__global__ __launch_bounds__(256) void add_diag_kernel(double* __restrict__ A, int Mp, int M, double v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) A[(long)i * (Mp + 1)] += v;
}
void launch_add_diag(hipStream_t s, double* A, int Mp, int M, double v) {
    if (M <= 0) return;
    hipLaunchKernelGGL(add_diag_kernel, dim3((M + 255) / 256), dim3(256), 0, s, A, Mp, M, v);
}

// One workgroup: flag[0] = 1 + the first i < M with L_ii^2 <= thr (or not a number), else 0.
__global__ __launch_bounds__(256) void pivot_check_kernel(const double* __restrict__ L, int Mp, int M, double thr, int* __restrict__ flag) {
    __shared__ int first;
    if (threadIdx.x == 0) first = 0x7fffffff;
    __syncthreads();
    int mine = 0x7fffffff;
    for (int i = threadIdx.x; i < M; i += 256) {
        const double d = L[(long)i * (Mp + 1)];
        if (!(d * d > thr)) {
            mine = i;
            break;
        }
    }
    if (mine != 0x7fffffff) atomicMin(&first, mine);
    __syncthreads();
    if (threadIdx.x == 0) flag[0] = first == 0x7fffffff ? 0 : first + 1;
}
void launch_pivot_check(hipStream_t s, const double* L, int Mp, int M, double thr, int* flag) {
    hipLaunchKernelGGL(pivot_check_kernel, dim3(1), dim3(256), 0, s, L, Mp, M, thr, flag);
}

// one workgroup per diagonal block; thread = row, column by column (coalesced)
__global__ __launch_bounds__(128) void zero_diag_upper_kernel(double* __restrict__ A, int Mp) {
    const int b = blockIdx.x, r = threadIdx.x;
    double* blk = A + (long)b * NB * (Mp + 1);
    for (int c = 1; c < NB; ++c)
        if (r < c) blk[r + (long)c * Mp] = 0.0;
}
void launch_zero_diag_upper(hipStream_t s, double* A, int Mp) {
    hipLaunchKernelGGL(zero_diag_upper_kernel, dim3(Mp / NB), dim3(NB), 0, s, A, Mp);
}

__global__ __launch_bounds__(256) void bcast_cols_kernel(const double* __restrict__ mu, int Mp, double* __restrict__ C, long ldc) {
    const int m = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (m < Mp) C[m + (long)n * ldc] = mu[m];
}
void launch_bcast_cols(hipStream_t s, const double* mu, int Mp, double* C, long ldc, int ncols) {
    if (ncols <= 0) return;
    hipLaunchKernelGGL(bcast_cols_kernel, dim3((Mp + 255) / 256, ncols), dim3(256), 0, s, mu, Mp, C, ldc);
}

}  // namespace slsk
