// Joint entropy search on the optima of posterior draws (include/sls_hip.h "joint entropy search"): the scalar terms tau, tau' of the
// truncated normal, the candidate-optima kernel stage, the combiner that turns mu, sigma and the K posterior covariances c_k(x) into
// the acquisition, its weights A_mu, A_sigma and H, and the kernels that fold the weights into the gradient.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// tau(t) = 1 - r (t + r), tau'(t) = r [(t + r)(t + 2 r) - 1], r = phi / Phi, without Phi underflowing.
//   t <  0: r from erfcx as mes_g forms it; w = r + t (LogEI) and c = 1 + t w (MES): tau = c - w^2, tau' = r (w^2 - tau).  The direct
//           forms cancel to ~1 / t^2: from t < -30 on c comes from mes_g's series in u = 1 / t^2 and w = (c - 1) / t.
//   t >= 0: Phi = erfc(-t / sqrt 2) / 2 has no cancellation; tau = 1 - r w stays near 1.
__device__ __forceinline__ void jes_tau(double t, double& tau, double& dtau) {
    constexpr double RSQRT2 = 0.70710678118654752440, SQRT_2_OVER_PI = 0.79788456080286535588, RSQRT_2PI = 0.39894228040143267794;
    double r, w;
    if (t < 0.0) {
        r = SQRT_2_OVER_PI / erfcx(-t * RSQRT2);
        w = r + t;
        double c = 1.0 + t * w;
        if (t < -30.0) {
            const double u = 1.0 / (t * t);
            c = u * (2.0 + u * (-10.0 + u * (74.0 + u * (-706.0 + u * 8162.0))));
            w = (c - 1.0) / t;
        }
        tau = c - w * w;
    } else {
        r = exp(-0.5 * t * t) * RSQRT_2PI / (0.5 * erfc(-t * RSQRT2));
        w = r + t;
        tau = 1.0 - r * w;
    }
    dtau = r * (w * w - tau);
}

__global__ __launch_bounds__(256) void jes_terms_kernel(const double* __restrict__ t, long n, double* __restrict__ tau,
                                                       double* __restrict__ dtau) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a, b;
    jes_tau(t[i], a, b);
    if (tau) tau[i] = a;
    if (dtau) dtau[i] = b;
}
void launch_jes_terms(hipStream_t s, const double* t, long n, double* tau, double* dtau) {
    if (n <= 0) return;
    hipLaunchKernelGGL(jes_terms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, n, tau, dtau);
}

// Per optimum k < K: v = sigma*^2 + star_noise (sigma* >= 0 comes from the tiled evaluation, so sigma*^2 is max(sigma^2, 0) squared
// back), d = f* - mu*, and the reciprocal 1 / v every candidate multiplies by: 0 below the floor (the uninformative optimum).
__global__ __launch_bounds__(256) void jes_optima_kernel(int K, const double* __restrict__ mu_star, const double* __restrict__ sg_star,
                                                        const double* __restrict__ f_star, double star_noise, double* __restrict__ v,
                                                        double* __restrict__ dd, double* __restrict__ inv_v) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double vv;
    {
#pragma clang fp contract(off)   // the square is rounded on its own (never fused into the sum): v has the bits of the host's sigma * sigma + star_noise
        const double sq = sg_star[k] * sg_star[k];
        vv = sq + star_noise;
    }
    v[k] = vv;
    dd[k] = f_star[k] - mu_star[k];
    inv_v[k] = vv < 1e-20 ? 0.0 : 1.0 / vv;
}
void launch_jes_optima(hipStream_t s, int K, const double* mu_star, const double* sg_star, const double* f_star, double star_noise,
                       double* v, double* dd, double* inv_v) {
    hipLaunchKernelGGL(jes_optima_kernel, dim3((K + 255) / 256), dim3(256), 0, s, K, mu_star, sg_star, f_star, star_noise, v, dd, inv_v);
}

// The candidate-optima stage: kx[m + k*ld] = k(x_m, x*_k) and cx[m + k*ld] = its derivative weight (kernel_kc) for m < M, k < K, from
// the differences of the RAW coordinates in dimension order (q keeps a relative error of (D + O(1)) eps at any length scale, so one
// form serves the handles on both sides of the Gram guard); exactly 0 for the padding m in [M, Mp) and k in [K, Kp).
// One lane per candidate and JES_KT optima: the candidate's coordinate is read once per JES_KT optima, the optimum's coordinate is
// uniform over the wave.  grid (Mp / 256 rounded up, Kp / JES_KT).  x[m*sn + d*sd]; xs[d + k*D].
constexpr int JES_KT = 4;
__global__ __launch_bounds__(256) void jes_cross_kernel(const double* __restrict__ x, long sn, long sd, int M, int Mp,
                                                       const double* __restrict__ xs, int D, int K,
                                                       const double* __restrict__ inv_ell, int kernel, double a,
                                                       double* __restrict__ kx, double* __restrict__ cx, long ld) {
    const int m = blockIdx.x * 256 + threadIdx.x, k0 = blockIdx.y * JES_KT;
    if (m >= Mp) return;
    double q[JES_KT];
#pragma unroll
    for (int j = 0; j < JES_KT; ++j) q[j] = 0.0;
    if (m < M && k0 < K) {
        for (int d = 0; d < D; ++d) {
            const double xv = x[(long)m * sn + (long)d * sd], il = inv_ell[d];
#pragma unroll
            for (int j = 0; j < JES_KT; ++j) {
                const int k = min(k0 + j, K - 1);
                const double t = (xv - xs[d + (long)k * D]) * il;
                q[j] = fma(t, t, q[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < JES_KT; ++j) {
        const int k = k0 + j;
        double kv = 0.0, cv = 0.0;
        if (m < M && k < K) kernel_kc(kernel, a, q[j], kv, cv);
        kx[(long)m + (long)k * ld] = kv;
        if (cx) cx[(long)m + (long)k * ld] = cv;
    }
}
void launch_jes_cross(hipStream_t s, const double* x, long sn, long sd, int M, int Mp, const double* xs, int D, int K, int Kp,
                      const double* inv_ell, KernelSpec ks, double* kx, double* cx, long ld) {
    hipLaunchKernelGGL(jes_cross_kernel, dim3((Mp + 255) / 256, Kp / JES_KT), dim3(256), 0, s, x, sn, sd, M, Mp, xs, D, K, inv_ell,
                       ks.kernel, ks.a, kx, cx, ld);
}

// ONE lane per candidate, whatever the grid: a candidate's sums over k run in increasing k in its own lane, so its bits depend on
// neither its column, the other candidates nor the launch shape.  The per-optimum constants f*, d, 1 / v are uniform over the
// workgroup: staged through LDS a tile at a time.  cov and H are candidate-major ([m + k*ld]: consecutive lanes, consecutive
// addresses).  H may be NULL (value only); padding candidates m in [S, Sp) get H = 0.
constexpr int JES_TILE = 256;
__global__ __launch_bounds__(JES_TILE) void jes_combine_kernel(int S, int Sp, long ld, const double* __restrict__ mu,
                                                              const double* __restrict__ sigma, const double* __restrict__ cov,
                                                              const double* __restrict__ f_star, const double* __restrict__ dd,
                                                              const double* __restrict__ inv_v, int K, double noise_var,
                                                              double* __restrict__ val, double* __restrict__ a_mu,
                                                              double* __restrict__ a_sg, double* __restrict__ H) {
    __shared__ double fs[JES_TILE], ds[JES_TILE], ivs[JES_TILE];
    const int n = blockIdx.x * JES_TILE + threadIdx.x;
    const bool mine = n < S, row = n < Sp;
    const double m = mine ? mu[n] : 0.0, sg = mine ? sigma[n] : 1.0;
    const double s2 = sg * sg;
    const double hk = -0.5 / (double)K;
    double S0 = 0.0, Sm = 0.0, Ss = 0.0;
    for (int k0 = 0; k0 < K; k0 += JES_TILE) {
        const int kc = min(JES_TILE, K - k0);
        __syncthreads();                       // the previous tile has been read by every lane
        if ((int)threadIdx.x < kc) {
            fs[threadIdx.x] = f_star[k0 + threadIdx.x];
            ds[threadIdx.x] = dd[k0 + threadIdx.x];
            ivs[threadIdx.x] = inv_v[k0 + threadIdx.x];
        }
        __syncthreads();
        if (!row) continue;
        for (int k = 0; k < kc; ++k) {
            const long at = (long)n + (long)(k0 + k) * ld;
            double h = 0.0;
            if (mine) {
                const double c = cov[at];
                const double ratio = c * ivs[k];
                const double mk = m + ratio * ds[k];
                const double sk2 = s2 - c * ratio;
                if (sk2 < 1e-20) {
                    S0 += log(noise_var);      // collapsed conditional: nothing left to learn about this optimum here
                } else {
                    const double sk = sqrt(sk2);
                    const double gam = (fs[k] - mk) / sk;
                    double tau, dtau;
                    jes_tau(gam, tau, dtau);
                    const double q = noise_var + sk2 * tau;
                    const double inv_q = 1.0 / q;
                    S0 += log(q);
                    Sm += (-sk * dtau) * inv_q;
                    Ss += (2.0 * sg * tau - gam * sg * dtau) * inv_q;
                    h = hk * ((-2.0 * ratio * tau + dtau * (gam * ratio - sk * ds[k] * ivs[k])) * inv_q);
                }
            }
            if (H) H[at] = h;
        }
    }
    if (!mine) return;
    const double tot = s2 + noise_var;
    val[n] = 0.5 * log(tot) + hk * S0;
    if (a_mu) {
        a_mu[n] = hk * Sm;
        a_sg[n] = sg / tot + hk * Ss;
    }
}
void launch_jes_combine(hipStream_t s, int S, int Sp, long ld, const double* mu, const double* sigma, const double* cov,
                        const double* f_star, const double* dd, const double* inv_v, int K, double noise_var, double* val, double* a_mu,
                        double* a_sg, double* H) {
    if (S <= 0) return;
    hipLaunchKernelGGL(jes_combine_kernel, dim3((Sp + JES_TILE - 1) / JES_TILE), dim3(JES_TILE), 0, s, S, Sp, ld, mu, sigma, cov, f_star,
                       dd, inv_v, K, noise_var, val, a_mu, a_sg, H);
}

// P[m + i*ld] = C*[m + i*ld] U[m + i*ld] in place in U, and csum[m] = sum_i P[m + i*ld] over i < Np as four fixed quarters of i
// (((q0 + q1) + q2) + q3), each accumulated from zero in increasing i: the form of path_data_kernel.  Workgroup = 64 candidates x 4
// quarters; Np is a multiple of 128, so a quarter is a multiple of 32 rows and runs four rows at a time (the four loads ahead of the
// four stores).  C* is exactly 0 for N <= i < Np, so the padding rows of P come out 0 and add zeros.  grid Sp / 64.
__global__ __launch_bounds__(256) void jes_weight_kernel(int Sp, int Np, long ld, const double* __restrict__ Cs, double* __restrict__ U,
                                                        double* __restrict__ csum) {
    __shared__ double part[4][64];
    const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + j;
    const int nq = Np / 4;
    double acc = 0.0;
    if (m < Sp) {
        for (int i = q * nq; i < (q + 1) * nq; i += 4) {
            const long at = (long)m + (long)i * ld;
            const double p0 = Cs[at] * U[at], p1 = Cs[at + ld] * U[at + ld], p2 = Cs[at + 2 * ld] * U[at + 2 * ld],
                         p3 = Cs[at + 3 * ld] * U[at + 3 * ld];
            U[at] = p0; U[at + ld] = p1; U[at + 2 * ld] = p2; U[at + 3 * ld] = p3;
            acc += p0; acc += p1; acc += p2; acc += p3;
        }
    }
    part[q][j] = acc;
    __syncthreads();
    if (q == 0 && m < Sp) csum[m] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
}
void launch_jes_weight(hipStream_t s, int Sp, int Np, long ld, const double* Cs, double* U, double* csum) {
    hipLaunchKernelGGL(jes_weight_kernel, dim3((Sp + 63) / 64), dim3(256), 0, s, Sp, Np, ld, Cs, U, csum);
}

// The optima term of the gradient: Go[m + d*ld] = sum_k H[m + k*ld] cx[m + k*ld] (x*_kd - x_md) / l_d in increasing k < K, m < M
// (d/dx_d k(x, x*) = cx (x*_d - x_d) / l_d^2; the second 1 / l_d is jes_finish_kernel's).  One lane per candidate and JES_DT dimensions:
// the weight H cx is read once per JES_DT dimensions.  grid (Mp / 256 rounded up, ceil(D / JES_DT)).
constexpr int JES_DT = 8;
__global__ __launch_bounds__(256) void jes_optima_grad_kernel(const double* __restrict__ x, long sn, long sd, int M,
                                                             const double* __restrict__ xs, int D, int K,
                                                             const double* __restrict__ inv_ell, const double* __restrict__ H,
                                                             const double* __restrict__ cx, long ld, double* __restrict__ Go) {
    const int m = blockIdx.x * 256 + threadIdx.x, d0 = blockIdx.y * JES_DT;
    if (m >= M) return;
    double xv[JES_DT], acc[JES_DT];
#pragma unroll
    for (int j = 0; j < JES_DT; ++j) {
        const int d = min(d0 + j, D - 1);
        xv[j] = x[(long)m * sn + (long)d * sd];
        acc[j] = 0.0;
    }
    for (int k = 0; k < K; ++k) {
        const long at = (long)m + (long)k * ld;
        const double wgt = H[at] * cx[at];
#pragma unroll
        for (int j = 0; j < JES_DT; ++j) {
            const int d = min(d0 + j, D - 1);
            acc[j] = fma(wgt, xs[d + (long)k * D] - xv[j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < JES_DT; ++j)
        if (d0 + j < D) Go[(long)m + (long)(d0 + j) * ld] = acc[j] * inv_ell[d0 + j];
}
void launch_jes_optima_grad(hipStream_t s, const double* x, long sn, long sd, int M, const double* xs, int D, int K,
                            const double* inv_ell, const double* H, const double* cx, long ld, double* Go) {
    if (M <= 0) return;
    hipLaunchKernelGGL(jes_optima_grad_kernel, dim3((M + 255) / 256, (D + JES_DT - 1) / JES_DT), dim3(256), 0, s, x, sn, sd, M, xs, D, K,
                       inv_ell, H, cx, ld, Go);
}

// The gradient and the guard, one lane per candidate:
//   grad_d = A_mu dmu_d + A_sigma dsigma_d + (Gd_d - x~_d csum + Go_d) / l_d          (XsT != nullptr: the tiled contraction Gd = P X~)
//   grad_d = A_mu dmu_d + A_sigma dsigma_d + (Gd_d + Go_d) / l_d                      (XsT == nullptr: Gd over raw differences)
// Guard of the EI combiner: sigma < 1e-10 or a NaN in the value or any gradient component -> value 0, gradient 0; ONE scan over d
// before the writes.  grad == nullptr: the guard on the value alone.  dmu / dsigma / grad have leading dimension ldo, the chunk's
// blocks Gd / Go / XsT ldk.
__global__ __launch_bounds__(256) void jes_finish_kernel(int S, int D, long ldo, long ldk, const double* __restrict__ sigma,
                                                        const double* __restrict__ dmu, const double* __restrict__ dsigma,
                                                        const double* __restrict__ a_mu, const double* __restrict__ a_sg,
                                                        const double* __restrict__ Gd, const double* __restrict__ Go,
                                                        const double* __restrict__ XsT, const double* __restrict__ csum,
                                                        const double* __restrict__ inv_ell, double* __restrict__ val,
                                                        double* __restrict__ grad) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= S) return;
    bool bad = (sigma[n] < 1e-10) || isnan(val[n]);
    if (grad) {
        const double am = a_mu[n], as = a_sg[n], cs = XsT ? csum[n] : 0.0;
        auto comp = [&](int d) {
            double data = Gd[n + d * ldk];
            if (XsT) data -= XsT[n + d * ldk] * cs;
            return (am * dmu[n + d * ldo] + as * dsigma[n + d * ldo]) + (data + Go[n + d * ldk]) * inv_ell[d];
        };
        for (int d = 0; d < D && !bad; ++d)
            if (isnan(comp(d))) bad = true;
        for (int d = 0; d < D; ++d) grad[n + d * ldo] = bad ? 0.0 : comp(d);
    }
    if (bad) val[n] = 0.0;
}
void launch_jes_finish(hipStream_t s, int S, int D, long ldo, long ldk, const double* sigma, const double* dmu, const double* dsigma,
                       const double* a_mu, const double* a_sg, const double* Gd, const double* Go, const double* XsT, const double* csum,
                       const double* inv_ell, double* val, double* grad) {
    if (S <= 0) return;
    hipLaunchKernelGGL(jes_finish_kernel, dim3((S + 255) / 256), dim3(256), 0, s, S, D, ldo, ldk, sigma, dmu, dsigma, a_mu, a_sg, Gd, Go,
                       XsT, csum, inv_ell, val, grad);
}

}  // namespace slsk
