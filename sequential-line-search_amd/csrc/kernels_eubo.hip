// Expected utility of the best option for a query PAIR (q = 2 case of qEUBO, Astudillo et al. 2023; include/sls_hip.h "expected
// utility of the best option"): the two kernels the pair objective adds to the tiled evaluation.  Everything between them -- the
// cross covariances of the two options, the contraction of d = k_x - k_x' with K_y^-1 and the gradient products -- is the
// evaluation's own kernels, unchanged (capi.hip: eval_pairs).
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// Kd = Ka - Kb over the whole padded block (n doubles, a multiple of 128 x 128): the padding rows of both operands are 0 and stay 0
__global__ __launch_bounds__(256) void pair_diff_kernel(const double* __restrict__ Ka, const double* __restrict__ Kb, long n,
                                                       double* __restrict__ Kd) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i >= n) return;
    const double2 a = *reinterpret_cast<const double2*>(Ka + i);
    const double2 b = *reinterpret_cast<const double2*>(Kb + i);
    double2 d;
    d.x = a.x - b.x;
    d.y = a.y - b.y;
    *reinterpret_cast<double2*>(Kd + i) = d;
}
void launch_pair_diff(hipStream_t s, const double* Ka, const double* Kb, long ldk, int Np, double* Kd) {
    const long n = ldk * Np;
    if (n <= 0) return;
    hipLaunchKernelGGL(pair_diff_kernel, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, s, Ka, Kb, n, Kd);
}

// mu Phi + mu' Phi' + s phi as three products and two sums, none of them contracted into a multiply-add: which product would be
// fused depends on the order of the operands, and (x, x') and (x', x) must not differ by more than the rounding of the sum
__device__ __forceinline__ double eubo_value(double mu0, double Phi0, double mu1, double Phi1, double s, double phi) {
#pragma clang fp contract(off)
    const double t0 = mu0 * Phi0;
    const double t1 = mu1 * Phi1;
    const double t2 = s * phi;
    return (t0 + t1) + t2;
}

// ONE lane per pair, whatever the grid: the partial sums of both options are added in increasing t in the pair's own lane, so its
// bits depend on neither its column, the other pairs nor the launch shape.  Option 0 is x, option 1 is x'.
// RAW (a handle beyond the guard of the norm expansion): the pair's own scaled difference (x_d - x'_d) / l_d is taken from the raw
// coordinates, differenced first -- a near-duplicate pair's difference is then exact, where x~_d - x~'_d carries eps |x~| = eps / (2 l)
// absolute (at l = 1e-8: 5e-9 in a difference of 0.3, 3e-9 a in k(x, x') and so in s^2).  RAW = false is the kernel as it was.
template <bool RAW>
__global__ __launch_bounds__(256) void eubo_finalize_kernel(EuboFinalizeArgs p) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.S) return;
    constexpr double RSQRT2 = 0.70710678118654752440, RSQRT_2PI = 0.39894228040143267794;
    double mu[2] = {0.0, 0.0}, ca[2] = {0.0, 0.0}, cw[2] = {0.0, 0.0}, kw = 0.0;
    const int tm_ = n >> 7, grp_ = tm_ >> 3;
    const int gm_ = min(8, p.ntm - 8 * grp_);
    const int tile_base = grp_ * 8 * p.nbt + (tm_ - 8 * grp_);       // tile index = tile_base + t * gm_ (acq_tile's order)
    for (int t = 0; t < p.nbt; ++t) {
        // tile (tm, t) in acq_gemm's grouped order; the tiles from split_first on ran as two halves (one slot each): finalize_kernel
        const bool halves = tile_base + t * gm_ >= p.split_first;
        double kt = p.kw_part[(long)(2 * t) * p.ldk + n];
        if (halves) kt += p.kw_part[(long)(2 * t + 1) * p.ldk + n];
        kw += kt;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            mu[o] += p.mu_part[o][(long)t * p.ldk + n];
            ca[o] += p.ca_part[o][(long)t * p.ldk + n];
            double ct = p.cw_part[o][(long)(2 * t) * p.ldk + n];
            if (halves) ct += p.cw_part[o][(long)(2 * t + 1) * p.ldk + n];
            cw[o] += ct;
        }
    }
    if (p.kw_solve_part) {                            // d . LLT.solve(d) = |L^-1 d|^2: var_gemm's sums
        kw = 0.0;
        for (int t = 0; t < p.nbt; ++t) kw += p.kw_solve_part[(long)(2 * t) * p.ldk + n];
    }
    // k(x, x') and its derivative weight from the scaled coordinates of the two options
    double q = 0.0;
    for (int d = 0; d < p.D; ++d) {
        double df;
        if constexpr (RAW) df = (p.xr[0][n + (long)d * p.ldr] - p.xr[1][n + (long)d * p.ldr]) * p.inv_ell[d];
        else df = p.XsT[0][n + (long)d * p.ldk] - p.XsT[1][n + (long)d * p.ldk];
        q = fma(df, df, q);
    }
    double k12, c12;
    kernel_kc(p.kernel, p.a, q, k12, c12);
    const double s2 = (2.0 * p.a - 2.0 * k12) - kw;
    const double s = sqrt(s2);
    const double u = (mu[0] - mu[1]) / s;
    const double Phi[2] = {0.5 * erfc(-u * RSQRT2), 0.5 * erfc(u * RSQRT2)};
    const double phi = exp(-0.5 * u * u) * RSQRT_2PI;
    const double v = eubo_value(mu[0], Phi[0], mu[1], Phi[1], s, phi);
    bool bad = !(s2 > 0.0) || s < 1e-10 || isnan(v);
    const double h = phi / (2.0 * s);
    // a NaN anywhere in the gradient takes the guard too (value included): the scan comes before any write, and it runs whether or
    // not the gradient is asked for, so that a pair's value does not depend on it
    for (int o = 0; o < 2 && !bad; ++o) {
        const double sg = o == 0 ? 2.0 : -2.0;
        for (int d = 0; d < p.D && !bad; ++d) {
            const double x0 = p.XsT[0][n + (long)d * p.ldk], x1 = p.XsT[1][n + (long)d * p.ldk];
            const double xo = o == 0 ? x0 : x1;
            const double il = p.inv_ell[d];
            const double dm = -il * (xo * ca[o] - p.Gm[o][n + (long)d * p.ldk]);
            const double T = il * (xo * cw[o] - p.Gs[o][n + (long)d * p.ldk]);
            double e;
            if constexpr (RAW) e = c12 * ((p.xr[0][n + (long)d * p.ldr] - p.xr[1][n + (long)d * p.ldr]) * il) * il;
            else e = c12 * (x0 - x1) * il;
            if (isnan(Phi[o] * dm + h * (sg * (e + T)))) bad = true;
        }
    }
    if (p.val) p.val[n] = bad ? fmax(mu[0], mu[1]) : v;
    if (!p.grad) return;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const double sg = o == 0 ? 2.0 : -2.0;
        for (int d = 0; d < p.D; ++d) {
            const double x0 = p.XsT[0][n + (long)d * p.ldk], x1 = p.XsT[1][n + (long)d * p.ldk];
            const double xo = o == 0 ? x0 : x1;
            const double il = p.inv_ell[d];
            const double dm = -il * (xo * ca[o] - p.Gm[o][n + (long)d * p.ldk]);     // grad mu of this option
            const double T = il * (xo * cw[o] - p.Gs[o][n + (long)d * p.ldk]);       // T_x,d / T_x',d
            double e;                                                                // e_d
            if constexpr (RAW) e = c12 * ((p.xr[0][n + (long)d * p.ldr] - p.xr[1][n + (long)d * p.ldr]) * il) * il;
            else e = c12 * (x0 - x1) * il;
            p.grad[n + (long)(o * p.D + d) * p.ldo] = bad ? 0.0 : Phi[o] * dm + h * (sg * (e + T));
        }
    }
}
void launch_eubo_finalize(hipStream_t s, const EuboFinalizeArgs& a) {
    if (a.S <= 0) return;
    if (a.xr[0]) hipLaunchKernelGGL(eubo_finalize_kernel<true>, dim3((a.S + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(eubo_finalize_kernel<false>, dim3((a.S + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace slsk
