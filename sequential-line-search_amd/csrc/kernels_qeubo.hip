// qEUBO, the expected utility of the best of q options on posterior draws (Astudillo et al. 2023; include/sls_hip.h "expected
// utility of the best of q options"): the two kernels the set objective adds around the path draws' own kernels and the tile GEMM
// (capi_path.hip: qeubo_eval_device).  Points are laid out option-major inside a pass: option i of set n is point i Sp + n.
// qNEI, noisy expected improvement on the same draws (Letham et al. 2019; include/sls_hip.h "noisy expected improvement on posterior
// draws"), is the same pass with a per-draw baseline in the selection, and adds the column reduction that forms such a baseline.
#include <climits>

#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// ONE lane per set (lanes n >= nsets only clear their columns of the mask).  V[i Sp + n + s ldv] holds f_s(x_i) on entry.  Draws are
// scanned in increasing s; within a draw the options in increasing i with a strictly-greater test, so the lowest option wins a tie.
// sum[n] = the sum of the maxima (from zero, increasing s, not yet divided), wins[n + i ldw] = draws option i wins, bad[n] = 1 when any
// of the q S values is not a number.  V is overwritten IN PLACE by the 0/1 indicator of the winner (a lane touches only its own
// elements), rows S <= s < Rp and the padding lanes are cleared: the block is then the B operand of the aggregation GEMM.
// BASE (qNEI): the options compete against the draw's baseline t[s] -- best starts from t[s] with no winner, every option i = 0..q-1
// is tested strictly-greater -- and the draw adds best - t[s] (exactly +0 without a winner, whose mask column is then all zero).
constexpr int QEUBO_LANES = 128;
template <bool BASE>
__global__ __launch_bounds__(QEUBO_LANES) void qeubo_select_kernel(int nsets, int Sp, int q, int S, int Rp, double* __restrict__ V, long ldv,
                                                                   const double* __restrict__ t, double* __restrict__ sum,
                                                                   int* __restrict__ wins, long ldw, int* __restrict__ bad) {
    __shared__ int cnt[SLS_QEUBO_MAX_OPTIONS][QEUBO_LANES];
    const int n = blockIdx.x * QEUBO_LANES + threadIdx.x;
    if (n >= Sp) return;
    const bool live = n < nsets;
    for (int i = 0; i < q; ++i) cnt[i][threadIdx.x] = 0;
    double total = 0.0;
    int nan_seen = 0;
    for (int s = 0; s < Rp; ++s) {
        double* col = V + n + (long)s * ldv;
        int arg = -1;
        if (live && s < S) {
            if constexpr (BASE) {
                const double ts = t[s];
                double best = ts;
                for (int i = 0; i < q; ++i) {
                    const double v = col[(long)i * Sp];
                    nan_seen |= v != v;
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
                total += best - ts;
                if (arg >= 0) cnt[arg][threadIdx.x] += 1;
            } else {
                double best = col[0];
                nan_seen |= best != best;
                arg = 0;
                for (int i = 1; i < q; ++i) {
                    const double v = col[(long)i * Sp];
                    nan_seen |= v != v;
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
                total += best;
                cnt[arg][threadIdx.x] += 1;
            }
        }
        for (int i = 0; i < q; ++i) col[(long)i * Sp] = i == arg ? 1.0 : 0.0;
    }
    if (!live) return;
    sum[n] = total;
    bad[n] = nan_seen;
    if (wins)
        for (int i = 0; i < q; ++i) wins[n + (long)i * ldw] = cnt[i][threadIdx.x];
}
void launch_qeubo_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, const double* t, double* sum,
                         int* wins, long ldw, int* bad) {
    if (Sp <= 0) return;
    if (t)
        hipLaunchKernelGGL(qeubo_select_kernel<true>, dim3(Sp / QEUBO_LANES), dim3(QEUBO_LANES), 0, s, nsets, Sp, q, S, Rp, V, ldv, t, sum,
                           wins, ldw, bad);
    else
        hipLaunchKernelGGL(qeubo_select_kernel<false>, dim3(Sp / QEUBO_LANES), dim3(QEUBO_LANES), 0, s, nsets, Sp, q, S, Rp, V, ldv, t, sum,
                           wins, ldw, bad);
}

// ONE lane per set: value = sum / S (the one division), gradient of option i = gpt[i Sp + n + d ldg] / S scattered from point layout
// to the candidate-major block grad[n + (i D + d) ldo] the lock-step rounds read.  Guard: bad[n], or a NaN in the value or in any of
// the q D gradient components, gives `floor` (SLS_QEUBO_FLOOR; 0 for qNEI) and the zero gradient; the scan runs before any write and
// whether or not the gradient is asked for.  val / grad may be NULL.
// PRE (qLogNEI): sum[n] is the value and gpt the gradient as they stand -- nothing is divided.
template <bool PRE>
__global__ __launch_bounds__(256) void qeubo_finish_kernel(int nsets, int Sp, int q, int D, int S, const double* __restrict__ sum,
                                                           const int* __restrict__ bad, const double* __restrict__ gpt, long ldg,
                                                           double floor, double* __restrict__ val, double* __restrict__ grad, long ldo) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nsets) return;
    const double v = PRE ? sum[n] : sum[n] / (double)S;
    bool guard = bad[n] != 0 || v != v;
    for (int i = 0; i < q && !guard; ++i)
        for (int d = 0; d < D; ++d) {
            const double g = PRE ? gpt[(long)i * Sp + n + (long)d * ldg] : gpt[(long)i * Sp + n + (long)d * ldg] / (double)S;
            if (g != g) {
                guard = true;
                break;
            }
        }
    if (val) val[n] = guard ? floor : v;
    if (!grad) return;
    for (int i = 0; i < q; ++i)
        for (int d = 0; d < D; ++d)
            grad[n + (long)(i * D + d) * ldo] =
                guard ? 0.0 : (PRE ? gpt[(long)i * Sp + n + (long)d * ldg] : gpt[(long)i * Sp + n + (long)d * ldg] / (double)S);
}
void launch_qeubo_finish(hipStream_t s, int nsets, int Sp, int q, int D, int S, const double* sum, const int* bad, const double* gpt,
                         long ldg, double floor, double* val, double* grad, long ldo, bool precomputed) {
    if (nsets <= 0) return;
    if (precomputed)
        hipLaunchKernelGGL(qeubo_finish_kernel<true>, dim3((nsets + 255) / 256), dim3(256), 0, s, nsets, Sp, q, D, S, sum, bad, gpt, ldg,
                           floor, val, grad, ldo);
    else
        hipLaunchKernelGGL(qeubo_finish_kernel<false>, dim3((nsets + 255) / 256), dim3(256), 0, s, nsets, Sp, q, D, S, sum, bad, gpt, ldg,
                           floor, val, grad, ldo);
}

// Column maximum with its lowest argmax: ONE workgroup per draw s over the rows pt < rows of V[pt + s ldv] (a draw's column is
// contiguous over the pass's points).  A thread scans its stride in increasing pt with a strictly-greater test, so it keeps its lowest
// index; records combine by "greater, or equal and lower index" -- over the 64 lanes of a wave by shuffles, across the waves through
// LDS -- which depends on no order.  A NaN poisons the column.  The result merges into the running record (t[s], arg[s]) of the earlier
// passes: base = 0 writes it, a later pass (higher indices base + pt) replaces it only when strictly greater; NaN gives (NaN, -1) and
// stays.
constexpr int PATH_MAX_THREADS = 256;
__device__ __forceinline__ void max_combine(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
__global__ __launch_bounds__(PATH_MAX_THREADS) void path_colmax_kernel(const double* __restrict__ V, long ldv, int rows, int base,
                                                                       double* __restrict__ t, int* __restrict__ arg) {
    __shared__ double sv[PATH_MAX_THREADS / 64];
    __shared__ int si[PATH_MAX_THREADS / 64], sn[PATH_MAX_THREADS / 64];
    const int s = blockIdx.x;
    const double* col = V + (long)s * ldv;
    double v = -HUGE_VAL;
    int i = INT_MAX, nan_seen = 0;
    for (int pt = threadIdx.x; pt < rows; pt += PATH_MAX_THREADS) {
        const double x = col[pt];
        nan_seen |= x != x;
        if (x > v || i == INT_MAX) {
            v = x;
            i = pt;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        nan_seen |= __shfl_xor(nan_seen, o);
        max_combine(v, i, ov, oi);
    }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
        sv[wave] = v;
        si[wave] = i;
        sn[wave] = nan_seen;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < PATH_MAX_THREADS / 64; ++w) {
        max_combine(v, i, sv[w], si[w]);
        nan_seen |= sn[w];
    }
    if (nan_seen) {
        t[s] = __builtin_nan("");
        arg[s] = -1;
    } else if (base == 0 || v > t[s]) {   // a poisoned record compares false and stays
        t[s] = v;
        arg[s] = base + i;
    }
}
void launch_path_colmax(hipStream_t s, const double* V, long ldv, int rows, int n_draws, int base, double* t, int* arg) {
    if (rows <= 0 || n_draws <= 0) return;
    hipLaunchKernelGGL(path_colmax_kernel, dim3(n_draws), dim3(PATH_MAX_THREADS), 0, s, V, ldv, rows, base, t, arg);
}

}  // namespace slsk
