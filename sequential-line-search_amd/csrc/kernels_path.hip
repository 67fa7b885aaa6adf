// Pathwise posterior function draws (sls_path_*, capi_path.hip; Wilson et al. 2020):
//   f_s(x) = sum_l [ W[l, s] cos(om_l . x~) + W[Fp + l, s] sin(om_l . x~) ]  +  sum_i V[i, s] k(x, x_i)
// with W already scaled by sqrt(a / F).  The random-feature prior is path_feat_kernel (MFMA contraction + sincos epilogue, the hot
// path of a maximisation round) and the tile GEMM of kernels_tri.hip; the data term runs on cross_gram's K* / C* (kernels_gram.hip)
// through path_data_kernel and the same tile GEMM.
//
// Every candidate is evaluated by arithmetic of its own, in an order fixed by (N, F, D) alone: its bits do not depend on the
// column it occupies, on the chunk it falls in, or on which candidates (of which draws) share its wave or workgroup.  The
// maximiser's compaction and the prefix property over draws rely on this.
#include "gemm_f64.hpp"
#include "kernels.hpp"

namespace slsk {

// Om[l + d*Fp] = z_{l D + d} * r_l for l < F, d < D (0 elsewhere, l < Fp, d < Dp); r_l = 1 (SE) or sqrt(5 / u_l) with
// u_l = sum_{j<5} z_{F D + 5 l + j}^2 (Matern 5/2: the multivariate t with 5 degrees of freedom).  Z = the B0 numbers of the block.
__global__ __launch_bounds__(256) void path_omega_kernel(const double* __restrict__ Z, int F, int Fp, int D, int Dp, int matern,
                                                         double* __restrict__ Om) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)Fp * Dp) return;
    const int l = (int)(idx % Fp), d = (int)(idx / Fp);
    double v = 0.0;
    if (l < F && d < D) {
        double r = 1.0;
        if (matern) {
            const double* u = Z + (long)F * D + 5L * l;
            const double uu = (((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]) + u[4] * u[4];
            r = sqrt(5.0 / uu);
        }
        v = Z[(long)l * D + d] * r;
    }
    Om[idx] = v;
}
void launch_path_omega(hipStream_t s, const double* Z, int F, int Fp, int D, int Dp, int matern, double* Om) {
    const long n = (long)Fp * Dp;
    hipLaunchKernelGGL(path_omega_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Z, F, Fp, D, Dp, matern, Om);
}

// W[l + s*2Fp] = scale E[s (2F + N) + l], W[Fp + l + s*2Fp] = scale E[s (2F + N) + F + l] (l < F, s < n_draws); 0 for F <= l < Fp
// and for n_draws <= s < Rp (the tile GEMM of the every-draw form reads whole 128-column tiles)
__global__ __launch_bounds__(256) void path_weights_kernel(const double* __restrict__ E, int F, int Fp, int N, int n_draws, int Rp,
                                                           double scale, double* __restrict__ W) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= 2L * Fp * Rp) return;
    const int r = (int)(idx % (2L * Fp)), s = (int)(idx / (2L * Fp));
    const int half = r >= Fp, l = r - half * Fp;
    W[idx] = (l < F && s < n_draws) ? scale * E[(long)s * (2L * F + N) + (long)half * F + l] : 0.0;
}
void launch_path_weights(hipStream_t s, const double* E, int F, int Fp, int N, int n_draws, int Rp, double scale, double* W) {
    const long n = 2L * Fp * Rp;
    hipLaunchKernelGGL(path_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, E, F, Fp, N, n_draws, Rp, scale, W);
}

// R[i + s*Np] <- y_i - sqrt(b) E[s (2F + N) + 2F + i] - R[i + s*Np] for i < N, s < n_draws; 0 elsewhere (i < Np, s < Rp)
__global__ __launch_bounds__(256) void path_rhs_kernel(const double* __restrict__ y, const double* __restrict__ E, int F, int N, int Np,
                                                       int n_draws, int Rp, double sqrt_b, double* __restrict__ R,
                                                       const double* __restrict__ Q) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)Np * Rp) return;
    const int i = (int)(idx % Np), s = (int)(idx / Np);
    double v = 0.0;
    if (i < N && s < n_draws) {
        if (Q) v = ((y[i] + Q[idx]) - sqrt_b * E[(long)s * (2L * F + 2L * N) + 2L * F + i]) - R[idx];   // a Laplace handle's draw layout
        else v = (y[i] - sqrt_b * E[(long)s * (2L * F + N) + 2L * F + i]) - R[idx];
    }
    R[idx] = v;
}
void launch_path_rhs(hipStream_t s, const double* y, const double* E, int F, int N, int Np, int n_draws, int Rp, double sqrt_b,
                     double* R, const double* Q) {
    const long n = (long)Np * Rp;
    hipLaunchKernelGGL(path_rhs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, E, F, N, Np, n_draws, Rp, sqrt_b, R, Q);
}

__global__ __launch_bounds__(256) void path_laplace_z_kernel(const double* __restrict__ E, int F, int N, int Np, int n_draws, int Rp,
                                                             double* __restrict__ Z) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)Np * Rp) return;
    const int i = (int)(idx % Np), s = (int)(idx / Np);
    Z[idx] = (i < N && s < n_draws) ? E[(long)s * (2L * F + 2L * N) + 2L * F + N + i] : 0.0;
}
void launch_path_laplace_z(hipStream_t s, const double* E, int F, int N, int Np, int n_draws, int Rp, double* Z) {
    const long n = (long)Np * Rp;
    hipLaunchKernelGGL(path_laplace_z_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, E, F, N, Np, n_draws, Rp, Z);
}

// (point, draw) of pair p: the gathered form (draw != nullptr) evaluates point p under draw[p]; the every-draw form point p % npts
// under draw p / npts.  Outputs go to out[p] (gathered) or out[point + draw * ldo] (every draw).
struct PairMap {
    const int* draw;
    int npts;
    long ldo;
    __device__ __forceinline__ void at(int p, int& pt, int& dr, long& o) const {
        if (draw) {
            pt = p;
            dr = draw[p];
            o = p;
        } else {
            pt = p % npts;
            dr = p / npts;
            o = pt + (long)dr * ldo;
        }
    }
};

// Random-feature prior on the matrix cores, one workgroup per (128-candidate tile, 128-frequency chunk):
//   Theta = X~_tile Om_chunk^T   (Dp deep, v_mfma_f64_16x16x4_f64 through gemm_tile_mc, accumulators in VGPRs)
// then an epilogue on the accumulator registers, one sincos per element:
//   gathered form (draw != nullptr): the candidate's own draw weights (W column draw[m]) give the chunk's value partial
//     vpart[chunk * ldv + m] (the thread's 16 columns in (j, r) order, then the 8 threads of a row in slot order through LDS) and the
//     gradient weights g = W_s cos - W_c sin, stored to G[m + l*ldg]; the second contraction G Om (Fp deep) runs on the tile GEMM
//     (launch_gemm_plain) and path_vsum_kernel adds the chunk partials in chunk order;
//   every-draw form (draw == nullptr): Phi[m + l*ldg] = cos, Phi[m + (Fp + l)*ldg] = sin, and Phi^T W runs on the tile GEMM.
// Om must hold Dp columns (zero beyond D), XsT Dp columns (zero beyond D); Fp is a multiple of 128.
__global__ __launch_bounds__(256, 2) void path_feat_kernel(const double* __restrict__ XsT, long ldx, int Dp, const double* __restrict__ Om,
                                                           int Fp, const double* __restrict__ W, long ldw, const int* __restrict__ draw,
                                                           int nvalid, double* __restrict__ G, long ldg, double* __restrict__ vpart,
                                                           long ldv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    const int nchunk = Fp / GEMM_BN;
    const int tm = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int m0 = tm * GEMM_BM, l0 = ch * GEMM_BN;
    Acc acc;
    acc.zero();
    gemm_tile_mc(acc, XsT + m0, ldx, Om + l0, Fp, 0, Dp, lds);
    if (!draw) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long m = m0 + acc_m(i), l = l0 + acc_n(j, r);
                    double sn, cs;
                    sincos(acc.v[i][j][r], &sn, &cs);
                    G[m + l * ldg] = cs;
                    G[m + (Fp + l) * ldg] = sn;
                }
        return;
    }
    double vp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + acc_m(i);
        const double* w = W + (long)(m < nvalid ? draw[m] : 0) * ldw;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int l = l0 + acc_n(j, r);
                double sn, cs;
                sincos(acc.v[i][j][r], &sn, &cs);
                const double a = w[l], b = w[Fp + l];
                v = fma(b, sn, fma(a, cs, v));
                G[(long)m + (long)l * ldg] = b * cs - a * sn;
            }
        vp[i] = v;
    }
    // the 8 partials of a row: slot = 4 (wave >> 1) + (lane >> 4), added in slot order (gemm_tile_mc left the LDS block free)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = 4 * (wave >> 1) + (lane >> 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) lds[acc_m(i) * 8 + slot] = vp[i];
    __syncthreads();
    if (threadIdx.x < GEMM_BM) {
        const double* q = lds + threadIdx.x * 8;
        vpart[(long)ch * ldv + m0 + threadIdx.x] = ((((((q[0] + q[1]) + q[2]) + q[3]) + q[4]) + q[5]) + q[6]) + q[7];
    }
}
void launch_path_feat(hipStream_t s, const double* XsT, long ldx, int Dp, int Mp, const double* Om, int Fp, const double* W, long ldw,
                      const int* draw, int nvalid, double* G, long ldg, double* vpart, long ldv) {
    ensure_dyn_lds((const void*)path_feat_kernel, GEMM_LDS_BYTES);
    const unsigned grid = (unsigned)((Mp / GEMM_BM) * (Fp / GEMM_BN));
    hipLaunchKernelGGL(path_feat_kernel, dim3(grid), dim3(GEMM_THREADS), GEMM_LDS_BYTES, s, XsT, ldx, Dp, Om, Fp, W, ldw, draw, nvalid, G,
                       ldg, vpart, ldv);
}

// val[n] = sum over the chunks c (in order) of vpart[c * ldv + n], n < S
__global__ __launch_bounds__(256) void path_vsum_kernel(const double* __restrict__ vpart, long ldv, int nchunk, int S,
                                                        double* __restrict__ val) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= S) return;
    double t = 0.0;
    for (int c = 0; c < nchunk; ++c) t += vpart[(long)c * ldv + n];
    val[n] = t;
}
void launch_path_vsum(hipStream_t s, const double* vpart, long ldv, int nchunk, int S, double* val) {
    if (S <= 0) return;
    hipLaunchKernelGGL(path_vsum_kernel, dim3((S + 255) / 256), dim3(256), 0, s, vpart, ldv, nchunk, S, val);
}

// Data term on K* / C* (candidate-major, [pt + i*ldk]): val[o] += sum_{i<N} K*[pt, i] V[i, dr], summed as four fixed quarters of
// i (((q0 + q1) + q2) + q3), each accumulated from zero in increasing i.  GRAD (gathered form only): Pm[pt + i*ldk] = C*[pt, i]
// V[i, dr] and csum[pt] = sum_i Pm (the same quarter order).  Workgroup = 64 pairs x 4 quarters.
template <bool GRAD>
__global__ __launch_bounds__(256) void path_data_kernel(const double* __restrict__ Ks, const double* __restrict__ Cs, long ldk, int N, int Np,
                                                        const double* __restrict__ V, long ldv, PairMap pm, int P, double* __restrict__ val,
                                                        double* __restrict__ Pm, double* __restrict__ csum) {
    __shared__ double part[2][4][64];
    const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + j;
    const int nq = (N + 3) / 4;
    const int i0 = q * nq, i1 = min(N, i0 + nq);
    double sv = 0.0, sc = 0.0;
    int pt = 0, dr = 0;
    long o = 0;
    if (p < P) {
        pm.at(p, pt, dr, o);
        const double* vv = V + (long)dr * ldv;
        for (int i = i0; i < i1; ++i) {
            const long e = pt + (long)i * ldk;
            const double vi = vv[i];
            sv = fma(Ks[e], vi, sv);
            if (GRAD) {
                const double pc = Cs[e] * vi;
                Pm[e] = pc;
                sc += pc;
            }
        }
        if (GRAD && q == 3)   // grad_gemm contracts all Np rows: the padding rows of Pm must be zero, not whatever the block held
            for (int i = N; i < Np; ++i) Pm[pt + (long)i * ldk] = 0.0;
    }
    part[0][q][j] = sv;
    part[1][q][j] = sc;
    __syncthreads();
    if (q == 0 && p < P) {
        const double dv = ((part[0][0][j] + part[0][1][j]) + part[0][2][j]) + part[0][3][j];
        val[o] = val[o] + dv;
        if (GRAD) csum[pt] = ((part[1][0][j] + part[1][1][j]) + part[1][2][j]) + part[1][3][j];
    }
}
void launch_path_data(hipStream_t s, const double* Ks, const double* Cs, long ldk, int N, int Np, const double* V, long ldv, const int* draw,
                      int npts, long ldo, int P, double* val, double* Pm, double* csum) {
    if (P <= 0) return;
    PairMap pm{draw, npts, ldo};
    const unsigned nb = (unsigned)((P + 63) / 64);
    if (Pm)
        hipLaunchKernelGGL(path_data_kernel<true>, dim3(nb), dim3(256), 0, s, Ks, Cs, ldk, N, Np, V, ldv, pm, P, val, Pm, csum);
    else
        hipLaunchKernelGGL(path_data_kernel<false>, dim3(nb), dim3(256), 0, s, Ks, Cs, ldk, N, Np, V, ldv, pm, P, val, Pm, csum);
}

// grad[n + d*ldo] = inv_ell_d (Gt[n + d*ldk] - XsT[n + d*ldk] csum[n])  for n < S, d < D, where Gt = G Om + Pm X~ (the prior's
// gradient in scaled coordinates plus X~^T c of the data term, c = C* o v): the data term is -inv_ell o (x~ sum_i c_i - X~^T c)
__global__ __launch_bounds__(256) void path_grad_kernel(int S, int D, long ldk, const double* __restrict__ Gt, const double* __restrict__ XsT,
                                                        const double* __restrict__ csum, const double* __restrict__ inv_ell,
                                                        double* __restrict__ grad, long ldo) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)S * D) return;
    const int n = (int)(idx % S), d = (int)(idx / S);
    const long e = n + (long)d * ldk;
    grad[n + (long)d * ldo] = inv_ell[d] * (Gt[e] - XsT[e] * csum[n]);
}
void launch_path_grad(hipStream_t s, int S, int D, long ldk, const double* Gt, const double* XsT, const double* csum, const double* inv_ell,
                      double* grad, long ldo) {
    const long n = (long)S * D;
    if (n <= 0) return;
    hipLaunchKernelGGL(path_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S, D, ldk, Gt, XsT, csum, inv_ell, grad, ldo);
}

// grad[n + d*ldo] = inv_ell_d (Gt[n + d*ldk] + Gd[n + d*ldk])  for n < S, d < D: the prior's gradient in scaled coordinates (Gt = G Om) plus
// the data term's contraction over raw coordinate differences (grad_direct: Gd = sum_i c_i (x_id - x_d) / l_d), beyond the guard
__global__ __launch_bounds__(256) void path_grad_direct_kernel(int S, int D, long ldk, const double* __restrict__ Gt, const double* __restrict__ Gd,
                                                               const double* __restrict__ inv_ell, double* __restrict__ grad, long ldo) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)S * D) return;
    const int n = (int)(idx % S), d = (int)(idx / S);
    const long e = n + (long)d * ldk;
    grad[n + (long)d * ldo] = inv_ell[d] * (Gt[e] + Gd[e]);
}
void launch_path_grad_direct(hipStream_t s, int S, int D, long ldk, const double* Gt, const double* Gd, const double* inv_ell, double* grad,
                             long ldo) {
    const long n = (long)S * D;
    if (n <= 0) return;
    hipLaunchKernelGGL(path_grad_direct_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S, D, ldk, Gt, Gd, inv_ell, grad, ldo);
}

// draw[j] = (live ? live[j] : j) / S  for j < n
__global__ __launch_bounds__(256) void path_draw_of_live_kernel(const int* __restrict__ live, int n, int S, int* __restrict__ draw) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) draw[j] = (live ? live[j] : j) / S;
}
void launch_path_draw_of_live(hipStream_t s, const int* live, int n, int S, int* draw) {
    if (n <= 0) return;
    hipLaunchKernelGGL(path_draw_of_live_kernel, dim3((n + 255) / 256), dim3(256), 0, s, live, n, S, draw);
}

// Segmented first maximum: draw s owns starts [s S, (s + 1) S); y = -f.  out[s * (D + 2)] = max, [+1] = index within the draw,
// [+2 .. +2+D) = x[n + d*ldx] of the winner.  A start whose value is not a number never wins over a number; the first start wins ties.
__global__ __launch_bounds__(64) void path_argmax_kernel(const double* __restrict__ f, int S, int n_draws, const double* __restrict__ x,
                                                         long ldx, int D, double* __restrict__ out) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_draws) return;
    const long base = (long)s * S;
    int bi = 0;
    double best = -f[base];
    for (int n = 1; n < S; ++n) {
        const double y = -f[base + n];
        if (y > best || (best != best && y == y)) {
            best = y;
            bi = n;
        }
    }
    double* o = out + (long)s * (D + 2);
    o[0] = best;
    o[1] = (double)bi;
    for (int d = 0; d < D; ++d) o[2 + d] = x[base + bi + (long)d * ldx];
}
void launch_path_argmax(hipStream_t s, const double* f, int S, int n_draws, const double* x, long ldx, int D, double* out) {
    hipLaunchKernelGGL(path_argmax_kernel, dim3((n_draws + 63) / 64), dim3(64), 0, s, f, S, n_draws, x, ldx, D, out);
}

}  // namespace slsk
