// qEUBO, the expected utility of the best of q options on posterior draws (Astudillo et al. 2023; include/sls_hip.h "expected
// utility of the best of q options"): the two kernels the set objective adds around the path draws' own kernels and the tile GEMM
// (capi_path.hip: qeubo_eval_device).  Points are laid out option-major inside a pass: option i of set n is point i Sp + n.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

// ONE lane per set (lanes n >= nsets only clear their columns of the mask).  V[i Sp + n + s ldv] holds f_s(x_i) on entry.  Draws are
// scanned in increasing s; within a draw the options in increasing i with a strictly-greater test, so the lowest option wins a tie.
// sum[n] = the sum of the maxima (from zero, increasing s, not yet divided), wins[n + i ldw] = draws option i wins, bad[n] = 1 when any
// of the q S values is not a number.  V is overwritten IN PLACE by the 0/1 indicator of the winner (a lane touches only its own
// elements), rows S <= s < Rp and the padding lanes are cleared: the block is then the B operand of the aggregation GEMM.
constexpr int QEUBO_LANES = 128;
__global__ __launch_bounds__(QEUBO_LANES) void qeubo_select_kernel(int nsets, int Sp, int q, int S, int Rp, double* __restrict__ V, long ldv,
                                                                   double* __restrict__ sum, int* __restrict__ wins, long ldw,
                                                                   int* __restrict__ bad) {
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
        for (int i = 0; i < q; ++i) col[(long)i * Sp] = i == arg ? 1.0 : 0.0;
    }
    if (!live) return;
    sum[n] = total;
    bad[n] = nan_seen;
    if (wins)
        for (int i = 0; i < q; ++i) wins[n + (long)i * ldw] = cnt[i][threadIdx.x];
}
void launch_qeubo_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, double* sum, int* wins, long ldw,
                         int* bad) {
    if (Sp <= 0) return;
    hipLaunchKernelGGL(qeubo_select_kernel, dim3(Sp / QEUBO_LANES), dim3(QEUBO_LANES), 0, s, nsets, Sp, q, S, Rp, V, ldv, sum, wins, ldw,
                       bad);
}

// ONE lane per set: value = sum / S (the one division), gradient of option i = gpt[i Sp + n + d ldg] / S scattered from point layout
// to the candidate-major block grad[n + (i D + d) ldo] the lock-step rounds read.  Guard: bad[n], or a NaN in the value or in any of
// the q D gradient components, gives SLS_QEUBO_FLOOR and the zero gradient; the scan runs before any write and whether or not the
// gradient is asked for.  val / grad may be NULL.
__global__ __launch_bounds__(256) void qeubo_finish_kernel(int nsets, int Sp, int q, int D, int S, const double* __restrict__ sum,
                                                           const int* __restrict__ bad, const double* __restrict__ gpt, long ldg,
                                                           double* __restrict__ val, double* __restrict__ grad, long ldo) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nsets) return;
    const double v = sum[n] / (double)S;
    bool guard = bad[n] != 0 || v != v;
    for (int i = 0; i < q && !guard; ++i)
        for (int d = 0; d < D; ++d) {
            const double g = gpt[(long)i * Sp + n + (long)d * ldg] / (double)S;
            if (g != g) {
                guard = true;
                break;
            }
        }
    if (val) val[n] = guard ? SLS_QEUBO_FLOOR : v;
    if (!grad) return;
    for (int i = 0; i < q; ++i)
        for (int d = 0; d < D; ++d)
            grad[n + (long)(i * D + d) * ldo] = guard ? 0.0 : gpt[(long)i * Sp + n + (long)d * ldg] / (double)S;
}
void launch_qeubo_finish(hipStream_t s, int nsets, int Sp, int q, int D, int S, const double* sum, const int* bad, const double* gpt,
                         long ldg, double* val, double* grad, long ldo) {
    if (nsets <= 0) return;
    hipLaunchKernelGGL(qeubo_finish_kernel, dim3((nsets + 255) / 256), dim3(256), 0, s, nsets, Sp, q, D, S, sum, bad, gpt, ldg, val, grad,
                       ldo);
}

}  // namespace slsk
