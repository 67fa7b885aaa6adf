// Max-value entropy search (Wang & Jegelka 2017; include/sls_hip.h "max-value entropy search"): the combiner that turns separately
// predicted mu, sigma, dmu, dsigma and K samples y* of the maximum value into the acquisition and its gradient, and the scalar
// terms g, g' behind it.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// g(t) = 1/2 t r(t) - log Phi(t), g'(t) = -1/2 r(t) (1 + t (t + r(t))), r = phi / Phi, without Phi underflowing.
//   t <  0: e = erfcx(-t / sqrt 2): r = sqrt(2 / pi) / e, log Phi = log(e / 2) - t^2 / 2;
//   t >= 0: Phi = erfc(-t / sqrt 2) / 2 (no cancellation), log Phi = log1p(-erfc(t / sqrt 2) / 2).
// c = 1 + t (t + r) cancels to ~2 / t^2 for large negative t and the direct form loses ~t^4 eps / 2 of it: from t < -30 on the
// asymptotic series in u = 1 / t^2 (its first omitted term is 1.1e5 u^6 = 1.5e-13 relative to 2 u at t = -30).
__device__ __forceinline__ void mes_g(double t, double& g, double& dg) {
    constexpr double RSQRT2 = 0.70710678118654752440, SQRT_2_OVER_PI = 0.79788456080286535588, RSQRT_2PI = 0.39894228040143267794;
    double r, log_Phi;
    if (t < 0.0) {
        const double e = erfcx(-t * RSQRT2);
        r = SQRT_2_OVER_PI / e;
        log_Phi = log(0.5 * e) - 0.5 * t * t;
    } else {
        r = exp(-0.5 * t * t) * RSQRT_2PI / (0.5 * erfc(-t * RSQRT2));
        log_Phi = log1p(-0.5 * erfc(t * RSQRT2));
    }
    double c = 1.0 + t * (t + r);
    if (t < -30.0) {
        const double u = 1.0 / (t * t);
        c = u * (2.0 + u * (-10.0 + u * (74.0 + u * (-706.0 + u * 8162.0))));
    }
    g = 0.5 * t * r - log_Phi;
    dg = -0.5 * r * c;
}

__global__ __launch_bounds__(256) void mes_terms_kernel(const double* __restrict__ t, long n, double* __restrict__ g,
                                                       double* __restrict__ dg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double gv, dv;
    mes_g(t[i], gv, dv);
    if (g) g[i] = gv;
    if (dg) dg[i] = dv;
}
void launch_mes_terms(hipStream_t s, const double* t, long n, double* g, double* dg) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mes_terms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, n, g, dg);
}

// ONE lane per candidate, whatever the grid: a candidate's sums over k run in increasing k in its own lane, so its bits depend on
// neither its column, the other candidates nor the launch shape.  y* is uniform over the workgroup: staged through LDS a tile at a
// time.  The K loop carries A0, A1, A2; the D loop behind it reads dmu / dsigma candidate-major (consecutive lanes, consecutive
// addresses).  Guard of the EI combiner (combine_kernel): sigma < 1e-10 or a NaN in the value or any gradient component -> value 0,
// gradient 0.
constexpr int MES_TILE = 256;
__global__ __launch_bounds__(MES_TILE) void mes_combine_kernel(int S, int D, long ld, const double* __restrict__ mu,
                                                              const double* __restrict__ sigma, const double* __restrict__ dmu,
                                                              const double* __restrict__ dsigma, const double* __restrict__ y_star,
                                                              int K, double* __restrict__ val, double* __restrict__ grad) {
    __shared__ double ys[MES_TILE];
    const int n = blockIdx.x * MES_TILE + threadIdx.x;
    const bool mine = n < S;
    const double m = mine ? mu[n] : 0.0, sg = mine ? sigma[n] : 1.0;
    const double inv_sg = 1.0 / sg;
    double A0 = 0.0, A1 = 0.0, A2 = 0.0;
    for (int k0 = 0; k0 < K; k0 += MES_TILE) {
        const int kc = min(MES_TILE, K - k0);
        __syncthreads();                       // the previous tile has been read by every lane
        if ((int)threadIdx.x < kc) ys[threadIdx.x] = y_star[k0 + threadIdx.x];
        __syncthreads();
        if (mine)
            for (int k = 0; k < kc; ++k) {
                const double gam = (ys[k] - m) / sg;
                double gv, dv;
                mes_g(gam, gv, dv);
                A0 += gv;
                A1 += dv;
                A2 += gam * dv;
            }
    }
    if (!mine) return;
    const double inv_K = 1.0 / (double)K;
    A0 *= inv_K; A1 *= inv_K; A2 *= inv_K;
    bool bad = (sg < 1e-10) || isnan(A0);
    if (grad) {
        for (int d = 0; d < D && !bad; ++d)
            if (isnan(-inv_sg * (A1 * dmu[n + d * ld] + A2 * dsigma[n + d * ld]))) bad = true;
        for (int d = 0; d < D; ++d) grad[n + d * ld] = bad ? 0.0 : -inv_sg * (A1 * dmu[n + d * ld] + A2 * dsigma[n + d * ld]);
    }
    val[n] = bad ? 0.0 : A0;
}
void launch_mes_combine(hipStream_t s, int S, int D, long ld, const double* mu, const double* sigma, const double* dmu,
                        const double* dsigma, const double* y_star, int K, double* val, double* grad) {
    if (S <= 0) return;
    hipLaunchKernelGGL(mes_combine_kernel, dim3((S + MES_TILE - 1) / MES_TILE), dim3(MES_TILE), 0, s, S, D, ld, mu, sigma, dmu, dsigma,
                       y_star, K, val, grad);
}

}  // namespace slsk
