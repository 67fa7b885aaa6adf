// Log-space expected improvement (include/sls_hip.h "log expected improvement"): the scalar terms log h, B1 = Phi / h, B2 = phi / h
// of h(u) = phi(u) + u Phi(u), and the combiner that turns separately predicted mu, sigma, dmu, dsigma into LogEI and its gradient.
// Phi is never formed for u < 0, so nothing underflows however far below the incumbent a point lies.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// r = phi / Phi and log Phi as mes_g forms them (kernels_mes.hip):
//   u <  0: e = erfcx(-u / sqrt 2): r = sqrt(2 / pi) / e, log Phi = log(e / 2) - u^2 / 2;
//   u >= 0: Phi = erfc(-u / sqrt 2) / 2 (no cancellation), r = phi / Phi.
// w = h / Phi = r + u cancels to ~1 / |u| for large negative u and the direct form loses ~u^2 eps of it: from u < -30 on
// w = (c - 1) / u with c = 1 + u (u + r) from mes_g's asymptotic series in t = 1 / u^2 (its first omitted term is 1.1e5 t^6 = 2e-13
// at u = -30, against c - 1 ~ -1: 2e-13 relative in w, B1 and B2, 2e-13 absolute in log w).
//   log h = log Phi + log w (u < 0);  log(phi + u Phi) (u >= 0, both terms positive);  B1 = 1 / w,  B2 = r / w.
__device__ __forceinline__ void logei_terms(double u, double& log_h, double& b1, double& b2) {
    constexpr double RSQRT2 = 0.70710678118654752440, SQRT_2_OVER_PI = 0.79788456080286535588, RSQRT_2PI = 0.39894228040143267794;
    double r, w;
    if (u < 0.0) {
        const double e = erfcx(-u * RSQRT2);
        r = SQRT_2_OVER_PI / e;
        w = r + u;
        if (u < -30.0) {
            const double t = 1.0 / (u * u);
            const double c = t * (2.0 + t * (-10.0 + t * (74.0 + t * (-706.0 + t * 8162.0))));
            w = (c - 1.0) / u;
        }
        log_h = (log(0.5 * e) - 0.5 * u * u) + log(w);
    } else {
        const double phi = exp(-0.5 * u * u) * RSQRT_2PI, Phi = 0.5 * erfc(-u * RSQRT2);
        r = phi / Phi;
        w = r + u;
        log_h = log(phi + u * Phi);
    }
    b1 = 1.0 / w;
    b2 = r / w;
}

__global__ __launch_bounds__(256) void logei_terms_kernel(const double* __restrict__ u, long n, double* __restrict__ log_h,
                                                         double* __restrict__ b1, double* __restrict__ b2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double lh, v1, v2;
    logei_terms(u[i], lh, v1, v2);
    if (log_h) log_h[i] = lh;
    if (b1) b1[i] = v1;
    if (b2) b2[i] = v2;
}
void launch_logei_terms(hipStream_t s, const double* u, long n, double* log_h, double* b1, double* b2) {
    if (n <= 0) return;
    hipLaunchKernelGGL(logei_terms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, u, n, log_h, b1, b2);
}

// ONE lane per candidate, whatever the grid, and one fixed operation order: a candidate's bits depend on neither its column, the other
// candidates nor the launch shape.  dmu / dsigma are read and grad written candidate-major (consecutive lanes, consecutive addresses).
// Guard with the conditions of the EI combiner (combine_kernel): sigma < 1e-10 or a NaN in the value or any gradient component ->
// value SLS_LOG_EI_FLOOR, gradient 0.
constexpr int LOGEI_TILE = 256;
__global__ __launch_bounds__(LOGEI_TILE) void logei_combine_kernel(int S, int D, long ld, const double* __restrict__ mu,
                                                                  const double* __restrict__ sigma, const double* __restrict__ dmu,
                                                                  const double* __restrict__ dsigma, double mu_best,
                                                                  double* __restrict__ val, double* __restrict__ grad) {
    const int n = blockIdx.x * LOGEI_TILE + threadIdx.x;
    if (n >= S) return;
    const double sg = sigma[n];
    const double inv_sg = 1.0 / sg;
    double log_h, b1, b2;
    logei_terms((mu[n] - mu_best) / sg, log_h, b1, b2);
    const double v = log(sg) + log_h;
    bool bad = (sg < 1e-10) || isnan(v);
    if (grad) {
        for (int d = 0; d < D && !bad; ++d)
            if (isnan(inv_sg * (b1 * dmu[n + d * ld] + b2 * dsigma[n + d * ld]))) bad = true;
        for (int d = 0; d < D; ++d) grad[n + d * ld] = bad ? 0.0 : inv_sg * (b1 * dmu[n + d * ld] + b2 * dsigma[n + d * ld]);
    }
    val[n] = bad ? SLS_LOG_EI_FLOOR : v;
}
void launch_logei_combine(hipStream_t s, int S, int D, long ld, const double* mu, const double* sigma, const double* dmu,
                          const double* dsigma, double mu_best, double* val, double* grad) {
    if (S <= 0) return;
    hipLaunchKernelGGL(logei_combine_kernel, dim3((S + LOGEI_TILE - 1) / LOGEI_TILE), dim3(LOGEI_TILE), 0, s, S, D, ld, mu, sigma, dmu,
                       dsigma, mu_best, val, grad);
}

}  // namespace slsk
