// Knowledge gradient on a discrete set (include/sls_hip.h "knowledge gradient"): the combiner that turns mu, sigma, the K posterior
// covariances c_k(x) and the K fixed means a_k into E_z max_j (a_j + b_j z) - a_max and its weights A_mu, A_sigma and H.  Everything
// around it (the covariances, U = -H W^T, the gradient contractions, the guard) is joint entropy search's (kernels_jes.hip).
//
// ONE workgroup per candidate; the candidate's n = K + include_self lines live in LDS by index k (slope bs, intercept as):
//   1. load: b_k = c_k / s, s = sqrt(sigma sigma + noise_var); line K is (mu, sigma sigma / s).  A NaN in any line makes the value NaN
//      (the finish turns it into the guard's 0) and H = 0.
//   2. bitonic sort of the 16-bit indices on the padded power of two P >= n (sentinels last) under the TOTAL order (b ascending, a
//      descending, index ascending): the sorted sequence is unique, so it depends on neither P nor the workgroup size.
//   3. one lane: the stack scan of Frazier's algorithm over the sorted lines, in place (the stack never passes the read position);
//      a line whose slope equals the previous sorted line's is skipped (the first of equal slopes stays); the breakpoints t_i are kept.
//   4. by k in parallel: a line on the envelope at position i forms beta = phi(t_i) - phi(t_i+1), pi as a difference of the smaller
//      tails, h_k = beta / s, the product beta c_k and the envelope term (b_e_i - b_e_i-1) f(-|t_i|); every other line gets 0.
//   5. two lanes: KG = the terms in envelope order; sum_k beta_k c_k in increasing k.  Both orders depend on the candidate's lines alone.
// LDS: four arrays of n doubles (rounded to 2), P + n 16-bit indices, 32 bytes: 39 024 bytes at n = 1025, P = 2048; 2 336 at n = 64.
#include "common.hpp"
#include "kernels.hpp"

namespace slsk {

namespace {
constexpr double KG_RSQRT2 = 0.70710678118654752440, KG_RSQRT_2PI = 0.39894228040143267794;
constexpr unsigned short KG_NONE = 0xFFFF;

struct KgArgs {
    int S, Sp, K, P, include_self, raw;
    long ld, ld_slope;
    const double *mu, *sigma, *cov, *a, *b_self;
    double noise_var, a_max;
    double *val, *a_mu, *a_sg, *H, *prob, *slope;
};

__device__ __forceinline__ double kg_phi(double t) {
#pragma clang fp contract(off)
    return exp(-0.5 * t * t) * KG_RSQRT_2PI;
}
// Phi(-t): the upper tail, no cancellation for t >= 0
__device__ __forceinline__ double kg_tail(double t) { return 0.5 * erfc(t * KG_RSQRT2); }
// f(-u) = phi(u) - u Phi(-u), u >= 0; 0 at u = +inf (inf 0 otherwise)
__device__ __forceinline__ double kg_f(double u) {
#pragma clang fp contract(off)
    if (isinf(u)) return 0.0;
    return kg_phi(u) - u * kg_tail(u);
}
// Phi(hi) - Phi(lo), lo < hi, as a difference of the smaller tails
__device__ __forceinline__ double kg_mass(double lo, double hi) {
#pragma clang fp contract(off)
    if (hi <= 0.0) return kg_tail(-hi) - kg_tail(-lo);
    if (lo >= 0.0) return kg_tail(lo) - kg_tail(hi);
    return (1.0 - kg_tail(-lo)) - kg_tail(hi);
}
// the total order of the sort on line indices (KG_NONE: the padding, after every line)
__device__ __forceinline__ bool kg_before(unsigned short p, unsigned short q, const double* bs, const double* as) {
    if (p == KG_NONE || q == KG_NONE) return p != KG_NONE && q == KG_NONE;
    const double bp = bs[p], bq = bs[q];
    if (bp < bq) return true;
    if (bp > bq) return false;
    const double ap = as[p], aq = as[q];
    if (ap > aq) return true;
    if (ap < aq) return false;
    return p < q;
}
}  // namespace

template <int NT>
__global__ __launch_bounds__(NT) void kg_combine_kernel(const KgArgs A) {
#pragma clang fp contract(off)   // every product is rounded on its own: the operation order of tests/kg_ref.py, whatever the compiler fuses elsewhere
    extern __shared__ __attribute__((aligned(16))) char kg_smem[];
    const int tid = threadIdx.x, m = blockIdx.x, K = A.K, P = A.P;
    const int n = K + (A.include_self ? 1 : 0), nn = (n + 1) & ~1;
    if (m >= A.S) {   // a padding row of the chunk: H = 0 (the U GEMM reads it)
        if (A.H && m < A.Sp)
            for (int k = tid; k < K; k += NT) A.H[(long)m + (long)k * A.ld] = 0.0;
        return;
    }
    double* bs = reinterpret_cast<double*>(kg_smem);
    double* as = bs + nn;
    double* wk = as + nn;
    double* tm = wk + nn;
    unsigned short* idx = reinterpret_cast<unsigned short*>(tm + nn);
    unsigned short* posk = idx + P;
    double* own = reinterpret_cast<double*>(kg_smem + (size_t)nn * 32 + (size_t)P * 2 + (size_t)((nn * 2 + 15) & ~15));   // beta_K, pi_K
    int* misc = reinterpret_cast<int*>(own + 2);

    // 1. the lines
    const double mu = A.mu ? A.mu[m] : 0.0;
    double sg = 0.0, s2 = 0.0, s = 1.0, b_own = 0.0;
    if (A.raw) {
        if (A.include_self) b_own = A.b_self[m];
    } else {
        sg = A.sigma[m];
        s2 = sg * sg;
        s = sqrt(s2 + A.noise_var);
        b_own = s2 / s;
    }
    int bad = 0;
    for (int k = tid; k < K; k += NT) {
        const double b = A.cov[(long)m + (long)k * A.ld] / s, a = A.a[k];
        bs[k] = b; as[k] = a;
        if (A.slope) A.slope[(long)m + (long)k * A.ld_slope] = b;
        bad |= (isnan(b) || isnan(a)) ? 1 : 0;
    }
    if (tid == 0 && A.include_self) {
        bs[K] = b_own; as[K] = mu;
        bad |= (isnan(b_own) || isnan(mu)) ? 1 : 0;
    }
    for (int p = tid; p < P; p += NT) idx[p] = p < n ? (unsigned short)p : KG_NONE;
    for (int k = tid; k < n; k += NT) posk[k] = KG_NONE;
    if (tid == 0) misc[1] = 0;
    __syncthreads();
    if (bad) misc[1] = 1;   // the same value from every writer
    __syncthreads();
    if (misc[1]) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int k = tid; k < K; k += NT) {
            if (A.H) A.H[(long)m + (long)k * A.ld] = 0.0;
            if (A.prob) A.prob[(long)m + (long)k * A.ld] = 0.0;
        }
        if (tid == 0) {
            A.val[m] = nan;
            if (A.a_mu) A.a_mu[m] = nan;
            if (A.a_sg) A.a_sg[m] = nan;
        }
        return;
    }

    // 2. the sort: P / 2 compare-exchanges per pass, one barrier per pass
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += NT) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
                const unsigned short p = idx[lo], q = idx[hi];
                const bool up = (lo & kk) == 0;
                if (kg_before(q, p, bs, as) == up) { idx[lo] = q; idx[hi] = p; }
            }
            __syncthreads();
        }

    // 3. the envelope: idx[0 .. E) the lines in slope order, tm[i] the breakpoint between lines i - 1 and i (tm[0] = -inf)
    if (tid == 0) {
        const double ninf = -__longlong_as_double(0x7ff0000000000000LL);
        int sz = 1;
        const int first = idx[0];
        double tb = bs[first], ta = as[first], tt = ninf, lastb = tb;
        tm[0] = ninf;
        for (int p = 1; p < n; ++p) {
            const int id = idx[p];
            const double bn = bs[id];
            if (bn == lastb) continue;
            lastb = bn;
            const double an = as[id];
            double t = ninf;
            while (sz > 0) {
                t = (ta - an) / (bn - tb);
                if (!(t <= tt)) break;
                --sz;
                if (sz > 0) {
                    const int top = idx[sz - 1];
                    tb = bs[top]; ta = as[top]; tt = tm[sz - 1];
                }
            }
            if (sz == 0) t = ninf;
            idx[sz] = (unsigned short)id;
            tm[sz] = t;
            tt = t; tb = bn; ta = an;
            ++sz;
        }
        misc[0] = sz;
    }
    __syncthreads();
    const int E = misc[0];
    for (int i = tid; i < E; i += NT) posk[idx[i]] = (unsigned short)i;
    __syncthreads();

    // 4. by line: weights of the lines on the envelope, zeros elsewhere.  Reads bs, tm, idx, posk; writes wk (by k) and as (by position).
    const bool want = A.H != nullptr;
    for (int k = tid; k < n; k += NT) {
        const int i = posk[k];
        double beta = 0.0, pi = 0.0;
        if (i != KG_NONE) {
            const double lo = tm[i], hi = i + 1 < E ? tm[i + 1] : __longlong_as_double(0x7ff0000000000000LL);
            beta = kg_phi(lo) - kg_phi(hi);
            pi = kg_mass(lo, hi);
            as[i] = i > 0 ? (bs[k] - bs[idx[i - 1]]) * kg_f(fabs(lo)) : 0.0;
        }
        if (k < K) {
            const long at = (long)m + (long)k * A.ld;
            if (want) {
                A.H[at] = beta / s;
                wk[k] = beta * A.cov[at];
            }
            if (A.prob) A.prob[at] = pi;
        } else {
            own[0] = beta;   // the candidate's own line
            own[1] = pi;
        }
    }
    __syncthreads();
    // 5. the two sums
    if (tid == 0) {
        double kg = 0.0;
        for (int i = 1; i < E; ++i) kg += as[i];
        if (A.include_self) kg += fmax(0.0, mu - A.a_max);
        A.val[m] = kg;
    }
    if (tid == NT - 1 && A.a_mu) {
        const double beta_own = A.include_self ? own[0] : 0.0, pi_own = A.include_self ? own[1] : 0.0;
        A.a_mu[m] = pi_own;
        if (A.raw) {
            A.a_sg[m] = beta_own;
        } else {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum += wk[k];
            A.a_sg[m] = (beta_own * (s2 + 2.0 * A.noise_var) - sum) * (sg / (s * s * s));
        }
    }
}

static void kg_launch(hipStream_t st, KgArgs A) {
    if (A.S <= 0) return;
    const int n = A.K + (A.include_self ? 1 : 0), nn = (n + 1) & ~1;
    int P = 64;
    while (P < n) P <<= 1;
    A.P = P;
    const size_t lds = (size_t)nn * 32 + (size_t)P * 2 + (size_t)((nn * 2 + 15) & ~15) + 32;
    if (P <= 128)
        hipLaunchKernelGGL(kg_combine_kernel<64>, dim3(A.Sp), dim3(64), lds, st, A);
    else
        hipLaunchKernelGGL(kg_combine_kernel<256>, dim3(A.Sp), dim3(256), lds, st, A);
}

void launch_kg_combine(hipStream_t st, int S, int Sp, long ld, const double* mu, const double* sigma, const double* cov, const double* a,
                       double a_max, int K, double noise_var, int include_self, double* val, double* a_mu, double* a_sg, double* H,
                       double* slope, long ld_slope) {
    KgArgs A{};
    A.S = S; A.Sp = Sp; A.K = K; A.include_self = include_self; A.raw = 0;
    A.ld = ld; A.ld_slope = ld_slope;
    A.mu = mu; A.sigma = sigma; A.cov = cov; A.a = a; A.b_self = nullptr;
    A.noise_var = noise_var; A.a_max = a_max;
    A.val = val; A.a_mu = a_mu; A.a_sg = a_sg; A.H = H; A.prob = nullptr; A.slope = slope;
    kg_launch(st, A);
}

void launch_kg_lines(hipStream_t st, int M, long ld, const double* a, double a_max, const double* B, int K, const double* a_self,
                     const double* b_self, double* val, double* beta, double* prob, double* self_pi, double* self_beta) {
    KgArgs A{};
    A.S = M; A.Sp = M; A.K = K; A.include_self = a_self != nullptr; A.raw = 1;
    A.ld = ld; A.ld_slope = 0;
    A.mu = a_self; A.sigma = nullptr; A.cov = B; A.a = a; A.b_self = b_self;
    A.noise_var = 0.0; A.a_max = a_max;
    A.val = val; A.a_mu = self_pi; A.a_sg = self_beta; A.H = beta; A.prob = prob; A.slope = nullptr;
    kg_launch(st, A);
}

}  // namespace slsk
