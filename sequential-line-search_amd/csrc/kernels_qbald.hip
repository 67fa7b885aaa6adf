// qBALD, the information gain of a q-option choice query on posterior draws (Houlsby et al. 2011 for pairs; include/sls_hip.h
// "information gain of a choice query on posterior draws"): the selection stage of the set pass (capi_path.hip: qeubo_eval_device)
// under the BTL likelihood.  As in the log form (kernels_qlognei.hip) the 0/1 mask of qEUBO becomes the real weights
// c_{i,s} = d value / d v_{i,s}; everything around the selection is the pass's own.  Points are laid out option-major inside a pass:
// option i of set n is point i Sp + n.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// kernels_qlognei.hip's layout: the draws are cut into slices of QBALD_SLICE (a constant: a set's bits depend on neither S's
// padding, the pass nor the launch), a thread is (set n, slice k), lane n of a wave reads V[i Sp + n + s ldv], contiguous in n.  A
// workgroup is 64 set lanes x 2 slices: the kernels are bound by the latency of a thread's chain of 16 draws, not by throughput, so
// the smaller workgroup only spreads a pass over more compute units and halves the LDS a workgroup asks for.  Every sum over the
// draws runs in one fixed order: over s increasing inside a slice, over the slices increasing.
//
// The sum over the OPTIONS of a draw, Z_s, does not depend on their order: the largest value contributes exp(0) = 1 exactly, every
// term lies in [0, 1] and is rounded to a multiple of 2^-58, and the terms are added as 64-bit integers (q <= 16 of them stay below
// 2^62).  Z_s >= 1, so that rounding moves it by at most q 2^-59 < eps / 4 relative.
//
// A thread's q numbers of a draw live in LDS between the loops over the options (q is a run-time number: a register array would go
// to scratch), element i of thread t at [i T + t] -- consecutive lanes, consecutive doubles.  So a value is read from memory once and
// written once per stage, with one exponential in stage A and one logarithm in stage B.
constexpr int QBALD_SLICE = 16;
constexpr int QBALD_LANES = 64;
constexpr int QBALD_WAVES = 2;
constexpr int QBALD_THREADS = QBALD_LANES * QBALD_WAVES;
constexpr double QBALD_FIX = 0x1p58, QBALD_UNFIX = 0x1p-58;
static_assert(SLS_QEUBO_MAX_OPTIONS <= 16, "q terms of at most 2^58 must stay below 2^63");
static_assert(SLS_QEUBO_MAX_OPTIONS * QBALD_THREADS * 3 * sizeof(double) <= 64 * 1024, "the LDS of a workgroup");

extern __shared__ double qbald_lds[];

// Stage A, thread = (set n, slice k), k < ceil(S / SLICE).  Per draw s of the slice: the NaN scan and qEUBO's hard-winner scan
// (best = option 0, strictly greater, increasing i -- its `best` is the draw's largest value), then
//   e_i = exp((v_i - best) / tau),  Z = the fixed-point sum of the e_i,  p_i = e_i / Z
// and the values are overwritten IN PLACE by p_i (a thread touches only its own elements), so stage B finds p_{i,s} as formed here
// and evaluates no exponential.  The slice's sum of p_{i,s} over its draws (from zero, s increasing) goes to pp[n + (k q + i) Sp], its
// NaN flag to pbad[n + k Sp], the win count of option i to pwin[n + (k q + i) Sp].  A NaN makes the set's numbers meaningless but
// harmless: stage B clears every row of a flagged set.
// LDS: (2 doubles + 1 int) q T.
__global__ __launch_bounds__(QBALD_THREADS) void qbald_stage_a_kernel(int nsets, int Sp, int q, int S, int nsl, double* __restrict__ V,
                                                                      long ldv, double tau, double* __restrict__ pp,
                                                                      int* __restrict__ pbad, int* __restrict__ pwin) {
    constexpr int T = QBALD_THREADS;
    double* es = qbald_lds + threadIdx.x;                     // the values, then the e_i, of the draw in hand
    double* ps = es + q * T;                                  // the running sums of p_i
    int* cnt = reinterpret_cast<int*>(qbald_lds + 2 * q * T) + threadIdx.x;
    const int n = blockIdx.x * QBALD_LANES + (threadIdx.x & (QBALD_LANES - 1));
    const int k = blockIdx.y * QBALD_WAVES + threadIdx.x / QBALD_LANES;
    if (n >= nsets || k >= nsl) return;
    for (int i = 0; i < q; ++i) {
        ps[i * T] = 0.0;
        cnt[i * T] = 0;
    }
    const int s0 = k * QBALD_SLICE, s1 = min(S, s0 + QBALD_SLICE);
    int nan_seen = 0;
    for (int s = s0; s < s1; ++s) {
        double* col = V + n + (long)s * ldv;
        double best = col[0];
        nan_seen |= best != best;
        es[0] = best;
        int arg = 0;
        for (int i = 1; i < q; ++i) {
            const double v = col[(long)i * Sp];
            nan_seen |= v != v;
            es[i * T] = v;
            if (v > best) {
                best = v;
                arg = i;
            }
        }
        cnt[arg * T] += 1;
        long long acc = 0;
        for (int i = 0; i < q; ++i) {
            const double e = exp((es[i * T] - best) / tau);
            es[i * T] = e;
            acc += __double2ll_rn(e * QBALD_FIX);
        }
        const double Z = (double)acc * QBALD_UNFIX;
        for (int i = 0; i < q; ++i) {
            const double p = es[i * T] / Z;
            col[(long)i * Sp] = p;
            ps[i * T] += p;
        }
    }
    for (int i = 0; i < q; ++i) {
        pp[n + (long)(k * q + i) * Sp] = ps[i * T];
        pwin[n + (long)(k * q + i) * Sp] = cnt[i * T];
    }
    pbad[n + (long)k * Sp] = nan_seen;
}

// Stage B, thread = (set n, slice k), k < Rp / SLICE.  Every thread of a set adds the set's nsl partial sums in increasing slice
// order and divides once: pbar_i (the same operations on the same numbers: the same bits in every thread), and keeps log pbar_i.
// The thread k = 0 writes pbar[n + i Sp], bad[n] and the summed win counts.  Then the slice's p_{i,s} are overwritten IN PLACE by
//   c_{i,s} = p_{i,s} (l_{i,s} - KL_s) / (S tau),  l_{i,s} = log p_{i,s} - log pbar_i (0 where p_{i,s} = 0),  KL_s = sum_i p_{i,s} l_{i,s}
// with KL_s a signed sum in increasing i, and the slice's sum of KL_s (from zero, s increasing) goes to pkl[n + k Sp].  Rows
// S <= s < Rp, the padding lanes n >= nsets and every row of a set with a NaN are cleared to exactly 0: the block is the B operand of
// the aggregation GEMM.
// LDS: 3 doubles q T.
__global__ __launch_bounds__(QBALD_THREADS) void qbald_stage_b_kernel(int nsets, int Sp, int q, int S, int Rp, int nsl,
                                                                      double* __restrict__ V, long ldv, double tau,
                                                                      const double* __restrict__ pp, const int* __restrict__ pbad,
                                                                      const int* __restrict__ pwin, double* __restrict__ pkl,
                                                                      double* __restrict__ pbar, int* __restrict__ wins, long ldw,
                                                                      int* __restrict__ bad) {
    constexpr int T = QBALD_THREADS;
    double* lpb = qbald_lds + threadIdx.x;                    // log pbar_i
    double* pv = lpb + q * T;                                 // p_i and
    double* lv = pv + q * T;                                  // l_i of the draw in hand
    const int n = blockIdx.x * QBALD_LANES + (threadIdx.x & (QBALD_LANES - 1));
    const int k = blockIdx.y * QBALD_WAVES + threadIdx.x / QBALD_LANES;
    if (n >= Sp || k * QBALD_SLICE >= Rp) return;
    const int s0 = k * QBALD_SLICE;
    int nan_seen = 0;
    if (n < nsets) {
        for (int j = 0; j < nsl; ++j) nan_seen |= pbad[n + (long)j * Sp];
        for (int i = 0; i < q; ++i) {
            double sum = 0.0;
            int w = 0;
            for (int j = 0; j < nsl; ++j) {
                sum += pp[n + (long)(j * q + i) * Sp];
                w += pwin[n + (long)(j * q + i) * Sp];
            }
            const double pb = sum / (double)S;
            lpb[i * T] = log(pb);
            if (k == 0) {
                pbar[n + (long)i * Sp] = pb;
                if (wins) wins[n + (long)i * ldw] = w;
            }
        }
        if (k == 0) bad[n] = nan_seen;
    }
    const bool live = n < nsets && !nan_seen;
    const double inv = 1.0 / ((double)S * tau);
    double klsum = 0.0;
    for (int s = s0; s < s0 + QBALD_SLICE; ++s) {
        double* col = V + n + (long)s * ldv;
        if (!live || s >= S) {
            for (int i = 0; i < q; ++i) col[(long)i * Sp] = 0.0;
            continue;
        }
        double kl = 0.0;
        for (int i = 0; i < q; ++i) {
            const double p = col[(long)i * Sp];
            const double l = p > 0.0 ? log(p) - lpb[i * T] : 0.0;
            pv[i * T] = p;
            lv[i * T] = l;
            kl += p * l;
        }
        klsum += kl;
        for (int i = 0; i < q; ++i) col[(long)i * Sp] = pv[i * T] * (lv[i * T] - kl) * inv;
    }
    if (n < nsets && k < nsl) pkl[n + (long)k * Sp] = klsum;
}

void launch_qbald_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, double tau, double* pp, double* pkl,
                         int* pbad, int* pwin, double* pbar, int* wins, long ldw, int* bad) {
    if (Sp <= 0) return;
    const int nsl = qbald_slices(S);
    const dim3 block(QBALD_THREADS);
    const size_t lds_a = (size_t)q * QBALD_THREADS * (2 * sizeof(double) + sizeof(int));
    const size_t lds_b = (size_t)q * QBALD_THREADS * 3 * sizeof(double);
    hipLaunchKernelGGL(qbald_stage_a_kernel, dim3(Sp / QBALD_LANES, (nsl + QBALD_WAVES - 1) / QBALD_WAVES), block, lds_a, s, nsets, Sp, q,
                       S, nsl, V, ldv, tau, pp, pbad, pwin);
    hipLaunchKernelGGL(qbald_stage_b_kernel, dim3(Sp / QBALD_LANES, (Rp / QBALD_SLICE + QBALD_WAVES - 1) / QBALD_WAVES), block, lds_b, s,
                       nsets, Sp, q, S, Rp, nsl, V, ldv, tau, pp, pbad, pwin, pkl, pbar, wins, ldw, bad);
}
int qbald_slices(int S) { return (S + QBALD_SLICE - 1) / QBALD_SLICE; }

// The finish of the pass for this criterion, ONE lane per set: value = (the slices' sums of KL_s, from zero, increasing slice) / S,
// the one division; the gradient of option i = gpt[i Sp + n + d ldg] as it stands (the weights carry 1 / (S tau)), scattered to the
// candidate-major block grad[n + (i D + d) ldo]; prob[n + i ldp] = pbar[n + i Sp].  Guard, as qeubo_finish_kernel's: bad[n], or a NaN
// in the value or in any of the q D gradient components, gives `floor`, the zero gradient and a zero prob column; the scan runs
// before any write and whether or not the gradient is asked for.  val / grad / prob may be NULL.
__global__ __launch_bounds__(256) void qbald_finish_kernel(int nsets, int Sp, int q, int D, int S, int nsl, const double* __restrict__ pkl,
                                                           const int* __restrict__ bad, const double* __restrict__ gpt, long ldg,
                                                           const double* __restrict__ pbar, double floor, double* __restrict__ val,
                                                           double* __restrict__ grad, long ldo, double* __restrict__ prob, long ldp) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nsets) return;
    double sum = 0.0;
    for (int j = 0; j < nsl; ++j) sum += pkl[n + (long)j * Sp];
    const double v = sum / (double)S;
    bool guard = bad[n] != 0 || v != v;
    for (int i = 0; i < q && !guard; ++i)
        for (int d = 0; d < D; ++d) {
            const double g = gpt[(long)i * Sp + n + (long)d * ldg];
            if (g != g) {
                guard = true;
                break;
            }
        }
    if (val) val[n] = guard ? floor : v;
    if (prob)
        for (int i = 0; i < q; ++i) prob[n + (long)i * ldp] = guard ? 0.0 : pbar[n + (long)i * Sp];
    if (!grad) return;
    for (int i = 0; i < q; ++i)
        for (int d = 0; d < D; ++d) grad[n + (long)(i * D + d) * ldo] = guard ? 0.0 : gpt[(long)i * Sp + n + (long)d * ldg];
}
void launch_qbald_finish(hipStream_t s, int nsets, int Sp, int q, int D, int S, const double* pkl, const int* bad, const double* gpt,
                         long ldg, const double* pbar, double floor, double* val, double* grad, long ldo, double* prob, long ldp) {
    if (nsets <= 0) return;
    hipLaunchKernelGGL(qbald_finish_kernel, dim3((nsets + 255) / 256), dim3(256), 0, s, nsets, Sp, q, D, S, qbald_slices(S), pkl, bad, gpt,
                       ldg, pbar, floor, val, grad, ldo, prob, ldp);
}

}  // namespace slsk
