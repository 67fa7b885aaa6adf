// Laplace posterior of the goodness values of a preference model (include/sls_hip.h: sls_gp_set_laplace): the kernels that are not
// tile products.  The Hessian W of the Bradley-Terry-Luce terms is assembled without floating-point atomics: one lane owns one row of
// W and adds its tuples' contributions in increasing flat position, so every entry has one fixed accumulation order.
#include "kernels.hpp"

namespace slsk {

// One lane per tuple t with members flat[off[t] .. off[t+1]): p = softmax(y / s) with the maximum subtracted (no overflow at any y, s),
// P[e] = p of flat position e, logp0[t] = log p of the chosen (first) member.
__global__ __launch_bounds__(256) void laplace_probs_kernel(const int* __restrict__ off, const int* __restrict__ flat, int n_prefs,
                                                            const double* __restrict__ y, double inv_s, double* __restrict__ P,
                                                            double* __restrict__ logp0) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_prefs) return;
    const int e0 = off[t], e1 = off[t + 1];
    double mx = y[flat[e0]] * inv_s;
    for (int e = e0 + 1; e < e1; ++e) mx = fmax(mx, y[flat[e]] * inv_s);
    double sum = 0.0;
    for (int e = e0; e < e1; ++e) {
        const double v = exp(y[flat[e]] * inv_s - mx);
        P[e] = v;
        sum += v;
    }
    const double inv = 1.0 / sum;
    for (int e = e0; e < e1; ++e) P[e] *= inv;
    logp0[t] = (y[flat[e0]] * inv_s - mx) - log(sum);
}

// One lane per data point i (row i of W, zeroed by the caller).  csc_ent[csc_off[i] .. csc_off[i+1]) are the flat positions that name
// point i, increasing; tuple_of[e] the tuple of flat position e.  For the occurrence e of i in tuple t and every member f of t:
//   W[i, flat[f]] += ((f == e ? p_e : 0) - p_e p_f) / s^2
// A repeated index adds, as a scatter-add does.  Only this lane writes row i.
__global__ __launch_bounds__(256) void laplace_w_kernel(const int* __restrict__ csc_off, const int* __restrict__ csc_ent,
                                                        const int* __restrict__ tuple_of, const int* __restrict__ off,
                                                        const int* __restrict__ flat, const double* __restrict__ P, int N, int Np,
                                                        double inv_s2, double* __restrict__ W) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (int q = csc_off[i]; q < csc_off[i + 1]; ++q) {
        const int e = csc_ent[q];
        const int t = tuple_of[e];
        const double pe = P[e];
        for (int f = off[t]; f < off[t + 1]; ++f) {
            const double h = ((f == e ? pe : 0.0) - pe * P[f]) * inv_s2;
            double* w = W + (long)i + (long)flat[f] * Np;
            *w += h;
        }
    }
}

void launch_laplace_w(hipStream_t s, const int* off, const int* flat, const int* csc_off, const int* csc_ent, const int* tuple_of,
                      int n_prefs, const double* y, double btl_scale, int N, int Np, double* P, double* logp0, double* W) {
    (void)hipMemsetAsync(W, 0, (size_t)Np * Np * sizeof(double), s);
    hipLaunchKernelGGL(laplace_probs_kernel, dim3((n_prefs + 255) / 256), dim3(256), 0, s, off, flat, n_prefs, y, 1.0 / btl_scale, P,
                       logp0);
    hipLaunchKernelGGL(laplace_w_kernel, dim3((N + 255) / 256), dim3(256), 0, s, csc_off, csc_ent, tuple_of, off, flat, P, N, Np,
                       1.0 / (btl_scale * btl_scale), W);
}

// A[r, c] <- A[c, r] for r < c: the strictly upper triangle becomes the mirror of the lower one (exactly symmetric).  32 x 32 blocks
// through LDS; Np a multiple of 32.  Block (bi, bj) with bi >= bj reads lower block (rows 32 bi, columns 32 bj).
__global__ __launch_bounds__(256) void mirror_lower_kernel(double* __restrict__ A, int Np) {
    __shared__ double tile[32][33];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) tile[k][tx] = A[(long)(32 * bi + tx) + (long)(32 * bj + k) * Np];   // tile[col][row]
    __syncthreads();
    // upper block (rows 32 bj, columns 32 bi): element (32 bj + tx, 32 bi + k) = lower (32 bi + k, 32 bj + tx) = tile[tx][k]
    for (int k = ty; k < 32; k += 8) {
        if (bi == bj && tx >= k) continue;   // the diagonal block keeps its lower triangle and diagonal
        A[(long)(32 * bj + tx) + (long)(32 * bi + k) * Np] = tile[tx][k];
    }
}
void launch_mirror_lower(hipStream_t s, double* A, int Np) {
    hipLaunchKernelGGL(mirror_lower_kernel, dim3(Np / 32, Np / 32), dim3(256), 0, s, A, Np);
}

// out[0] = sum_t logp0[t], out[1] = 2 sum_{i<N} log LB[i, i], out[2] = sum_{i<N} y_i alpha_i: one workgroup, lane l adds its
// elements l, l + 256, .. in increasing order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void laplace_summary_kernel(const double* __restrict__ logp0, int n_prefs, const double* __restrict__ LB,
                                                              int Np, int N, const double* __restrict__ y,
                                                              const double* __restrict__ alpha, double* __restrict__ out) {
    __shared__ double red[3][256];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int t = threadIdx.x; t < n_prefs; t += 256) a += logp0[t];
    for (int i = threadIdx.x; i < N; i += 256) {
        b += log(LB[(long)i * (Np + 1)]);
        c += y[i] * alpha[i];
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0][0];
        out[1] = 2.0 * red[1][0];
        out[2] = red[2][0];
    }
}
void launch_laplace_summary(hipStream_t s, const double* logp0, int n_prefs, const double* LB, int Np, int N, const double* y,
                            const double* alpha, double* out) {
    hipLaunchKernelGGL(laplace_summary_kernel, dim3(1), dim3(256), 0, s, logp0, n_prefs, LB, Np, N, y, alpha, out);
}

}  // namespace slsk
