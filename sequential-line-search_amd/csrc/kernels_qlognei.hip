// qLogNEI, the log-space form of noisy expected improvement on posterior draws (Ament et al. 2023; include/sls_hip.h "log-space noisy
// expected improvement on posterior draws"): the selection stage of the set pass (capi_path.hip: qeubo_eval_device) in log space.
// The 0/1 mask of qEUBO / qNEI becomes the real weights c_{i,s} = d value / d v_{i,s}; everything around the selection is the pass's own.
// Points are laid out option-major inside a pass: option i of set n is point i Sp + n.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// L(a) = log softplus(a) and R(a) = L'(a), in the three branches of the header.  e = exp(-|a|) <= 1 and lp = log1p(e) in (0, ln 2]
// are shared; a < -36 returns (a, 1): the neglected term of L is below exp(-36) / 2 < eps / 8.
constexpr double QLOGNEI_CUT = -36.0;
__device__ __forceinline__ double qlognei_L(double a) {
    if (a < QLOGNEI_CUT) return a;
    const double lp = log1p(exp(-fabs(a)));
    return log(a >= 0.0 ? a + lp : lp);
}
__device__ __forceinline__ void qlognei_LR(double a, double& L, double& R) {
    if (a < QLOGNEI_CUT) {
        L = a;
        R = 1.0;
        return;
    }
    const double e = exp(-fabs(a)), lp = log1p(e);
    if (a >= 0.0) {
        const double sp = a + lp;
        L = log(sp);
        R = 1.0 / ((1.0 + e) * sp);
    } else {
        L = log(lp);
        R = e / ((1.0 + e) * lp);
    }
}

__global__ __launch_bounds__(256) void qlognei_terms_kernel(const double* __restrict__ a, long n, double* __restrict__ L,
                                                            double* __restrict__ R) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double l, r;
    qlognei_LR(a[i], l, r);
    if (L) L[i] = l;
    if (R) R[i] = r;
}
void launch_qlognei_terms(hipStream_t s, const double* a, long n, double* L, double* R) {
    if (n <= 0) return;
    hipLaunchKernelGGL(qlognei_terms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, n, L, R);
}

// The selection, parallel over sets AND draws.  The draws are cut into slices of QLOGNEI_SLICE (a constant: a set's bits depend on
// neither S's padding, the pass nor the geometry).  A workgroup is 64 set lanes x 4 slices: lane n of a wave reads V[i Sp + n + s ldv],
// contiguous in n.  The sums over the draws run in one fixed order: over s increasing inside a slice, over the slices increasing,
// as an ONLINE log-sum-exp (running maximum, the sum rescaled when the maximum moves).
//
// The sum over the OPTIONS of a draw does not depend on their order, so permuting a set's options permutes its weights, and with them
// its gradient blocks, bit for bit.  Mq is taken at the largest value (L is increasing; a maximum has no order), every term
// e_i = exp(min(l_i - Mq, 0) / taum) lies in [0, 1], and Zq is the sum of the e_i rounded to multiples of 2^-58, added as 64-bit
// integers: q <= 16 such terms stay below 2^62 and integer addition is associative.  The largest option contributes exactly 1, so
// Zq >= 1 and the rounding of the terms moves Zq by at most q 2^-59 < eps / 4 relative; the min only matters where rounding makes
// the computed L non-monotone by an ulp.  A draw's values are read twice in stage A (the second read hits the cache).
constexpr int QLOGNEI_SLICE = 16;
constexpr int QLOGNEI_LANES = 64;
constexpr int QLOGNEI_WAVES = 4;
constexpr double QLOGNEI_FIX = 0x1p58, QLOGNEI_UNFIX = 0x1p-58;
static_assert(SLS_QEUBO_MAX_OPTIONS <= 16, "q terms of at most 2^58 must stay below 2^63");

// e_i from L(a_i), stage A's and stage B's.  Should the two kernels ever round an l_i differently, the weights still only move by
// rounding: nothing below needs the two to agree in bits, and each kernel is deterministic.
__device__ __forceinline__ double qlognei_E(double L, double log_tau0, double Mq, double invm) {
    return exp(fmin(log_tau0 + L - Mq, 0.0) * invm);
}

// Stage A, thread = (set n, slice k), k < ceil(S / SLICE): per draw s of the slice
//   Mq = log tau0 + L((max_i v_i - t_s) / tau0);  l_i = log tau0 + L((v_i - t_s) / tau0);  Zq = the fixed-point sum of the e_i;
//   m_s = fma(taum, log Zq, Mq)
// Mq and Zq go to the Sp x Rp scratch (mq, zq)[n + s Sp]; the slice's online (max, sum exp(m_s - max)) over its draws goes to
// (pmx, psm)[n + k Sp], its NaN flag to pbad[n + k Sp], and the hard winner's count (sls_qnei_eval's scan: best = t_s, strictly
// greater, increasing i) of option i to pwin[n + (k q + i) Sp].  V is only read.
__global__ __launch_bounds__(QLOGNEI_LANES* QLOGNEI_WAVES) void qlognei_stage_a_kernel(
    int nsets, int Sp, int q, int S, int nsl, const double* __restrict__ V, long ldv, const double* __restrict__ t, double tau0, double taum,
    double* __restrict__ mq, double* __restrict__ zq, double* __restrict__ pmx, double* __restrict__ psm, int* __restrict__ pbad,
    int* __restrict__ pwin) {
    __shared__ int cnt[SLS_QEUBO_MAX_OPTIONS][QLOGNEI_LANES * QLOGNEI_WAVES];
    const int n = blockIdx.x * QLOGNEI_LANES + (threadIdx.x & (QLOGNEI_LANES - 1));
    const int k = blockIdx.y * QLOGNEI_WAVES + threadIdx.x / QLOGNEI_LANES;
    if (n >= nsets || k >= nsl) return;
    for (int i = 0; i < q; ++i) cnt[i][threadIdx.x] = 0;
    const double log_tau0 = log(tau0), inv0 = 1.0 / tau0, invm = 1.0 / taum;
    const int s1 = min(S, (k + 1) * QLOGNEI_SLICE);
    double Mx = -HUGE_VAL, Zx = 0.0;
    int nan_seen = 0;
    for (int s = k * QLOGNEI_SLICE; s < s1; ++s) {
        const double* col = V + n + (long)s * ldv;
        const double ts = t[s];
        double best = ts, vmax = -HUGE_VAL;
        int arg = -1;
        for (int i = 0; i < q; ++i) {
            const double v = col[(long)i * Sp];
            nan_seen |= v != v;
            if (v > best) {
                best = v;
                arg = i;
            }
            vmax = fmax(vmax, v);
        }
        if (arg >= 0) cnt[arg][threadIdx.x] += 1;
        const double Mq = log_tau0 + qlognei_L((vmax - ts) * inv0);
        long long acc = 0;
        for (int i = 0; i < q; ++i)
            acc += __double2ll_rn(qlognei_E(qlognei_L((col[(long)i * Sp] - ts) * inv0), log_tau0, Mq, invm) * QLOGNEI_FIX);
        const double Zq = (double)acc * QLOGNEI_UNFIX;
        mq[n + (long)s * Sp] = Mq;
        zq[n + (long)s * Sp] = Zq;
        const double m = fma(taum, log(Zq), Mq);
        if (m > Mx) {
            Zx = Zx * exp(Mx - m) + 1.0;
            Mx = m;
        } else {
            Zx += exp(m - Mx);
        }
    }
    pmx[n + (long)k * Sp] = Mx;
    psm[n + (long)k * Sp] = Zx;
    pbad[n + (long)k * Sp] = nan_seen;
    for (int i = 0; i < q; ++i) pwin[n + (long)(k * q + i) * Sp] = cnt[i][threadIdx.x];
}

// Stage B, thread = (set n, slice k), k < Rp / SLICE.  Every thread of a set combines the set's nsl partials in increasing slice order
// (the same operations on the same numbers: the same bits in every thread), the thread k = 0 writes sum[n] = value = Mx + log Z - log S,
// bad[n] and the summed win counts.  Then the slice's values are overwritten IN PLACE by
//   c_{i,s} = omega_s pi_{i,s} rho_{i,s},  omega_s = exp(m_s - Mx) / Z,  pi_{i,s} = exp((l_i - Mq_s) / taum) / Zq_s,  rho = R(a) / tau0
// with l_i recomputed from the value (stage A's operations) and (Mq_s, Zq_s) read back.  Rows S <= s < Rp, the padding lanes
// n >= nsets and every row of a set with a NaN are cleared to exactly 0: the block is the B operand of the aggregation GEMM.
__global__ __launch_bounds__(QLOGNEI_LANES* QLOGNEI_WAVES) void qlognei_stage_b_kernel(
    int nsets, int Sp, int q, int S, int Rp, int nsl, double* __restrict__ V, long ldv, const double* __restrict__ t, double tau0,
    double taum, const double* __restrict__ mq, const double* __restrict__ zq, const double* __restrict__ pmx,
    const double* __restrict__ psm, const int* __restrict__ pbad, const int* __restrict__ pwin, double* __restrict__ sum,
    int* __restrict__ wins, long ldw, int* __restrict__ bad) {
    const int n = blockIdx.x * QLOGNEI_LANES + (threadIdx.x & (QLOGNEI_LANES - 1));
    const int k = blockIdx.y * QLOGNEI_WAVES + threadIdx.x / QLOGNEI_LANES;
    if (n >= Sp || k * QLOGNEI_SLICE >= Rp) return;
    const int s0 = k * QLOGNEI_SLICE;
    double Mx = -HUGE_VAL, Z = 0.0;
    int nan_seen = 0;
    if (n < nsets) {
        for (int j = 0; j < nsl; ++j) {
            const double m = pmx[n + (long)j * Sp], z = psm[n + (long)j * Sp];
            nan_seen |= pbad[n + (long)j * Sp];
            if (m > Mx) {
                Z = Z * exp(Mx - m) + z;
                Mx = m;
            } else {
                Z += z * exp(m - Mx);
            }
        }
        if (k == 0) {
            sum[n] = Mx + log(Z) - log((double)S);
            bad[n] = nan_seen;
            if (wins)
                for (int i = 0; i < q; ++i) {
                    int w = 0;
                    for (int j = 0; j < nsl; ++j) w += pwin[n + (long)(j * q + i) * Sp];
                    wins[n + (long)i * ldw] = w;
                }
        }
    }
    const bool live = n < nsets && !nan_seen;
    const double log_tau0 = log(tau0), inv0 = 1.0 / tau0, invm = 1.0 / taum, invZ = 1.0 / Z;
    for (int s = s0; s < s0 + QLOGNEI_SLICE; ++s) {
        double* col = V + n + (long)s * ldv;
        if (!live || s >= S) {
            for (int i = 0; i < q; ++i) col[(long)i * Sp] = 0.0;
            continue;
        }
        const double ts = t[s], Mq = mq[n + (long)s * Sp], Zq = zq[n + (long)s * Sp];
        const double m = fma(taum, log(Zq), Mq);   // stage A's m_s: an explicit fma in both kernels, not left to -ffp-contract
        const double scale = exp(m - Mx) * invZ / Zq * inv0;   // omega_s / (Zq tau0)
        for (int i = 0; i < q; ++i) {
            double L, R;
            qlognei_LR((col[(long)i * Sp] - ts) * inv0, L, R);
            col[(long)i * Sp] = scale * qlognei_E(L, log_tau0, Mq, invm) * R;
        }
    }
}

void launch_qlognei_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, const double* t, double tau0,
                           double taum, double* mq, double* zq, double* pmx, double* psm, int* pbad, int* pwin, double* sum, int* wins,
                           long ldw, int* bad) {
    if (Sp <= 0) return;
    const int nsl = qlognei_slices(S);
    const dim3 block(QLOGNEI_LANES * QLOGNEI_WAVES);
    hipLaunchKernelGGL(qlognei_stage_a_kernel, dim3(Sp / QLOGNEI_LANES, (nsl + QLOGNEI_WAVES - 1) / QLOGNEI_WAVES), block, 0, s, nsets, Sp, q,
                       S, nsl, V, ldv, t, tau0, taum, mq, zq, pmx, psm, pbad, pwin);
    hipLaunchKernelGGL(qlognei_stage_b_kernel, dim3(Sp / QLOGNEI_LANES, (Rp / QLOGNEI_SLICE + QLOGNEI_WAVES - 1) / QLOGNEI_WAVES), block, 0,
                       s, nsets, Sp, q, S, Rp, nsl, V, ldv, t, tau0, taum, mq, zq, pmx, psm, pbad, pwin, sum, wins, ldw, bad);
}
int qlognei_slices(int S) { return (S + QLOGNEI_SLICE - 1) / QLOGNEI_SLICE; }

}  // namespace slsk
