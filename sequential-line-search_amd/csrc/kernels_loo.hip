// Leave-one-out cross-validation of a GP (Rasmussen & Williams, GPML 5.4.2) from what a fit holds anyway: Kinv = K_y^-1 and
// alpha = Kinv y.  With d_i = Kinv_ii:
//     mu_-i = y_i - alpha_i / d_i,  var_-i = 1 / d_i,  logp_i = 1/2 log d_i - alpha_i^2 / (2 d_i) - 1/2 log 2 pi,  L = sum_i logp_i
// and the gradient of L is a weight matrix contracted against dK/dtheta_p, like the marginal likelihood's (kernels_map.hip):
//     u = Kinv (alpha ./ d),  c_i = 1/2 (1 + alpha_i^2 / d_i) / d_i,  M = Kinv diag(c) Kinv,  W = 1/2 (u alpha^T + alpha u^T) - M
//     dL/dtheta_p = sum_ij W_ij dK_ij/dtheta_p,   dL/db = sum_i (u_i alpha_i - M_ii).
// W enters where nll_weight_kernel's w = 1/2 (alpha_i alpha_j - Kinv_ij) does (no further 1/2): G = W .* c_kernel, the per-tile sums
// of W .* k and the row sums of G are left exactly as that kernel leaves them, so Y = G X~, sum_chunks and lengthscale_grad serve
// both criteria.  The one new N^3 stage is M, a symmetric product on the fp64 matrix cores (loo_syrk_kernel).
#include "gemm_f64.hpp"
#include "kernels.hpp"
#include "../../include/sls_hip.h"

namespace slsk {

__device__ __forceinline__ double loo_block_sum_256(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// d_i = sum_{k = i}^{N-1} (L^-1)_ki^2 = (K_y^-1)_ii from the factor's inverse alone (a handle in the Cholesky-solve sigma mode): one
// wave per column (contiguous), lane-strided partial sums in increasing k, then the shuffle tree.
__global__ __launch_bounds__(256) void loo_diag_linv_kernel(const double* __restrict__ Linv, int Np, int N, double* __restrict__ d) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double* col = Linv + (long)i * Np;
    double s = 0.0;
    for (int k = i + lane; k < N; k += 64) s = fma(col[k], col[k], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) d[i] = s;
}
void launch_loo_diag_linv(hipStream_t s, const double* Linv, int Np, int N, double* d) {
    hipLaunchKernelGGL(loo_diag_linv_kernel, dim3((N + 3) / 4), dim3(256), 0, s, Linv, Np, N, d);
}

// The per-point terms by ONE workgroup.  dvec[i * dstride]: d_i (Kinv with stride Np + 1, or a vector).  Every padded entry
// N <= i < Np of the five vectors is exactly 0.  Lsum[0] = L: 256 partial sums over i mod 256 in increasing i, then the binary tree
// (the order nll_scalars_block uses for log|K_y|).
__global__ __launch_bounds__(256) void loo_terms_kernel(const double* __restrict__ dvec, long dstride, const double* __restrict__ alpha,
                                                        const double* __restrict__ y, int Np, int N, double* __restrict__ mu,
                                                        double* __restrict__ var, double* __restrict__ logp, double* __restrict__ ad,
                                                        double* __restrict__ sc, double* __restrict__ Lsum) {
    __shared__ double red256[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < Np; i += 256) {
        double m = 0.0, v = 0.0, lp = 0.0, q = 0.0, r = 0.0;
        if (i < N) {
            const double d = dvec[(long)i * dstride], a = alpha[i];
            q = a / d;
            m = y[i] - q;
            v = 1.0 / d;
            lp = 0.5 * log(d) - 0.5 * (a * q) - 0.91893853320467274178;   // 1/2 log 2 pi
            r = sqrt(0.5 * (1.0 + a * q) / d);
            s += lp;
        }
        mu[i] = m; var[i] = v; logp[i] = lp; ad[i] = q; sc[i] = r;
    }
    red256[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red256[threadIdx.x] += red256[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) Lsum[0] = red256[0];
}
void launch_loo_terms(hipStream_t s, const double* dvec, long dstride, const double* alpha, const double* y, int Np, int N, double* mu,
                      double* var, double* logp, double* ad, double* sc, double* Lsum) {
    hipLaunchKernelGGL(loo_terms_kernel, dim3(1), dim3(256), 0, s, dvec, dstride, alpha, y, Np, N, mu, var, logp, ad, sc, Lsum);
}

// R[i + k*Np] = Kinv[i + k*Np] sc[k]: Kinv diag(sqrt c), the transpose of diag(sqrt c) Kinv (Kinv is symmetric), so that both
// operands of M = R R^T are M-contiguous and go straight from global memory into LDS.  One N^2 pass; the scale cannot be applied
// inside the LDS-direct load.  sc is 0 in the padding: the padded columns of R are exactly zero.
__global__ __launch_bounds__(256) void loo_scale_kernel(const double* __restrict__ Kinv, const double* __restrict__ sc, int Np,
                                                        double* __restrict__ R) {
    const long n2 = (long)Np * Np / 2;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n2; e += (long)gridDim.x * 256L) {
        const long off = 2 * e;
        const double f = sc[off / Np];   // Np is even: both elements sit in one column
        d2_t v = *reinterpret_cast<const d2_t*>(Kinv + off);
        v[0] *= f; v[1] *= f;
        *reinterpret_cast<d2_t*>(R + off) = v;
    }
}

// M = R R^T (= Kinv diag(c) Kinv) on v_mfma_f64_16x16x4_f64, the nt (nt + 1) / 2 tiles with tm >= tn only: N^3 flop.  One workgroup
// per 128 x 128 tile through the LDS-direct tile loop, Np deep (an even number of slabs).  Tiles above the diagonal are not written.
__global__ __launch_bounds__(256) void loo_syrk_kernel(const double* __restrict__ R, int Np, double* __restrict__ M) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    const int nt = Np / GEMM_BM;
    int tn = 0, rem = blockIdx.x;
    while (rem >= nt - tn) {
        rem -= nt - tn;
        ++tn;
    }
    const int tm = tn + rem;
    const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
    Acc acc;
    acc.zero();
    gemm_tile_mc<4, true>(acc, R + m0, Np, R + n0, Np, 0, Np, lds);
    acc_tile_by_columns(acc, lds, [&](int col, int row, d2_t v) {
        *reinterpret_cast<d2_t*>(M + (long)(m0 + row) + (long)(n0 + col) * Np) = v;
    });
}
void launch_loo_syrk(hipStream_t s, const double* Kinv, const double* sc, int Np, double* R, double* M) {
    ensure_dyn_lds((const void*)loo_syrk_kernel, GEMM_LDS_BYTES);
    const int nt = Np / GEMM_BM;
    const long n2 = (long)Np * Np / 2;
    const int nb = (int)((n2 + 255) / 256 < 4096 ? (n2 + 255) / 256 : 4096);
    hipLaunchKernelGGL(loo_scale_kernel, dim3(nb), dim3(256), 0, s, Kinv, sc, Np, R);
    if (!tune_on(TUNE_LOO_SYRK)) {   // SLS_LOO_SYRK=0 (A/B, tools/time_loo.py): the full product, every tile, by the generic GEMM
        launch_gemm_plain(s, R, Np, false, R, Np, false, M, Np, nt, nt, Np, 1.0, 0.0);
        return;
    }
    hipLaunchKernelGGL(loo_syrk_kernel, dim3(nt * (nt + 1) / 2), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, R, Np, M);
}

// M_ij from the lower triangle: entry (i, j) with i < j reads M_ji
__device__ __forceinline__ double loo_m_lower(const double* __restrict__ M, int Np, int gi, int gj) {
    return gi >= gj ? M[(long)gi + (long)gj * Np] : M[(long)gj + (long)gi * Np];
}

// nll_weight_kernel with w = 1/2 (u_i alpha_j + alpha_i u_j) - M_ij: the same kernel-tile rebuild, the same outputs G, wk_part,
// row_part in the same orders.
template <bool MATERN>
__global__ __launch_bounds__(256) void loo_weight_kernel(const double* __restrict__ XT, long ld, int Dp, const double* __restrict__ nx,
                                                         int Np, int N, double a, const double* __restrict__ alpha,
                                                         const double* __restrict__ u, const double* __restrict__ M,
                                                         double* __restrict__ G, double* __restrict__ wk_part,
                                                         double* __restrict__ row_part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    const int nt = Np / GEMM_BM;
    const int tm = blockIdx.x % nt, tn = blockIdx.x / nt;
    const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
    Acc acc;
    acc.zero();
    gemm_tile<false, false>(acc, XT + m0, ld, XT + n0, ld, 0, Dp, lds);
    double part = 0.0;
    d2_t rs = {0.0, 0.0};
    acc_tile_by_columns<true>(acc, lds, [&](int col, int row, d2_t dot) {
        const int gj = n0 + col;
        const double nj = nx[gj], aj = alpha[gj], uj = u[gj];
        const d2_t ni = *reinterpret_cast<const d2_t*>(nx + m0 + row);
        const d2_t ai = *reinterpret_cast<const d2_t*>(alpha + m0 + row);
        const d2_t ui = *reinterpret_cast<const d2_t*>(u + m0 + row);
        const long off = (long)(m0 + row) + (long)gj * Np;
        d2_t mm;
        if (tm > tn) {
            mm = *reinterpret_cast<const d2_t*>(M + off);
        } else {
            mm[0] = loo_m_lower(M, Np, m0 + row, gj);
            mm[1] = loo_m_lower(M, Np, m0 + row + 1, gj);
        }
        d2_t g;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gi = m0 + row + e;
            double q = ni[e] + nj - 2.0 * dot[e];
            q = (q < 0.0 || gi == gj) ? 0.0 : q;
            double k, c;
            if (!MATERN) {
                k = a * exp(-0.5 * q);
                c = k;
            } else {
                const double s = sqrt(5.0 * q), ex = exp(-s);
                k = a * (1.0 + s + (5.0 / 3.0) * q) * ex;
                c = a * (5.0 / 3.0) * (1.0 + s) * ex;
            }
            double w = 0.5 * (ui[e] * aj + ai[e] * uj) - mm[e];
            if (gi >= N || gj >= N) w = 0.0;
            g[e] = w * c;
            part += w * k;
        }
        rs += g;
        *reinterpret_cast<d2_t*>(G + off) = g;
    });
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = part;
    *reinterpret_cast<d2_t*>(lds + 8 + 128 * (threadIdx.x >> 6) + 2 * (threadIdx.x & 63)) = rs;
    __syncthreads();
    if (threadIdx.x == 0) wk_part[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    if (row_part && threadIdx.x < 128) {
        const double* r = lds + 8 + threadIdx.x;
        row_part[(long)tn * Np + m0 + threadIdx.x] = (r[0] + r[128]) + (r[256] + r[384]);
    }
}

void launch_loo_weight(hipStream_t s, const double* XT, long ld, int Dp, const double* nx, int Np, int N, KernelSpec ks,
                       const double* alpha, const double* u, const double* M, double* G, double* wk_part, double* row_part) {
    ensure_dyn_lds((const void*)loo_weight_kernel<false>, GEMM_LDS_BYTES);
    ensure_dyn_lds((const void*)loo_weight_kernel<true>, GEMM_LDS_BYTES);
    const int nt = Np / GEMM_BM;
    if (ks.kernel == SLS_KERNEL_ARD_MATERN52)
        hipLaunchKernelGGL(loo_weight_kernel<true>, dim3(nt * nt), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, XT, ld, Dp, nx, Np, N, ks.a,
                           alpha, u, M, G, wk_part, row_part);
    else
        hipLaunchKernelGGL(loo_weight_kernel<false>, dim3(nt * nt), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, XT, ld, Dp, nx, Np, N, ks.a,
                           alpha, u, M, G, wk_part, row_part);
}

// nll_weight_direct_kernel with the LOO weights (gram_direct_form): q from the raw coordinate differences
template <bool MATERN>
__global__ __launch_bounds__(256) void loo_weight_direct_kernel(const double* __restrict__ X, int D, const double* __restrict__ inv_ell,
                                                                int Np, int N, double a, const double* __restrict__ alpha,
                                                                const double* __restrict__ u, const double* __restrict__ M,
                                                                double* __restrict__ G, double* __restrict__ wk_part) {
    __shared__ double red[4];
    extern __shared__ double ils[];
    for (int d = threadIdx.x; d < D; d += 256) ils[d] = inv_ell[d];
    __syncthreads();
    const int nt = Np / 128;
    const int m0 = (blockIdx.x % nt) * 128, n0 = (blockIdx.x / nt) * 128;
    const int gi = m0 + (threadIdx.x & 127), c0 = n0 + 64 * (threadIdx.x >> 7);
    const double ai = alpha[gi], ui = u[gi];
    double part = 0.0;
    for (int gj = c0; gj < c0 + 64; ++gj) {
        const long off = (long)gi + (long)gj * Np;
        double g = 0.0;
        if (gi < N && gj < N) {
            double q = 0.0;
            if (gi != gj)
                for (int d = 0; d < D; ++d) {
                    const double t = (X[d + (long)gi * D] - X[d + (long)gj * D]) * ils[d];
                    q = fma(t, t, q);
                }
            double k, c;
            if (!MATERN) {
                k = a * exp(-0.5 * q);
                c = k;
            } else {
                const double s = sqrt(5.0 * q), ex = exp(-s);
                k = a * (1.0 + s + (5.0 / 3.0) * q) * ex;
                c = a * (5.0 / 3.0) * (1.0 + s) * ex;
            }
            const double w = 0.5 * (ui * alpha[gj] + ai * u[gj]) - loo_m_lower(M, Np, gi, gj);
            g = w * c;
            part += w * k;
        }
        G[off] = g;
    }
    const double t = loo_block_sum_256(part, red);
    if (threadIdx.x == 0) wk_part[blockIdx.x] = t;
}

void launch_loo_weight_direct(hipStream_t s, const double* X, int D, const double* inv_ell, int Np, int N, KernelSpec ks,
                              const double* alpha, const double* u, const double* M, double* G, double* wk_part) {
    const int nt = Np / 128;
    if (ks.kernel == SLS_KERNEL_ARD_MATERN52)
        hipLaunchKernelGGL(loo_weight_direct_kernel<true>, dim3(nt * nt), dim3(256), (size_t)D * 8, s, X, D, inv_ell, Np, N, ks.a, alpha, u,
                           M, G, wk_part);
    else
        hipLaunchKernelGGL(loo_weight_direct_kernel<false>, dim3(nt * nt), dim3(256), (size_t)D * 8, s, X, D, inv_ell, Np, N, ks.a, alpha,
                           u, M, G, wk_part);
}

// The sums of a LOO gradient by ONE workgroup, in nll_scalars_block's orders (strided by 256, then the wave tree and the four waves):
// out[0] = sum_t part[t] (= sum_ij W_ij K_f,ij),  out[1] = dL/db = sum_{i < N} (u_i alpha_i - M_ii).
__global__ __launch_bounds__(256) void loo_scalars_kernel(const double* __restrict__ part, int nparts, const double* __restrict__ alpha,
                                                          const double* __restrict__ u, const double* __restrict__ M, int Np, int N,
                                                          double* __restrict__ out) {
    __shared__ double red[4];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < nparts; i += 256) s0 += part[i];
#pragma unroll 8
    for (int i = threadIdx.x; i < N; i += 256) s1 += u[i] * alpha[i] - M[(long)i * (Np + 1)];
    const double t0 = loo_block_sum_256(s0, red);
    const double t1 = loo_block_sum_256(s1, red);
    if (threadIdx.x == 0) {
        out[0] = t0;
        out[1] = t1;
    }
}
void launch_loo_scalars(hipStream_t s, const double* part, int nparts, const double* alpha, const double* u, const double* M, int Np,
                        int N, double* out) {
    hipLaunchKernelGGL(loo_scalars_kernel, dim3(1), dim3(256), 0, s, part, nparts, alpha, u, M, Np, N, out);
}

}  // namespace slsk
