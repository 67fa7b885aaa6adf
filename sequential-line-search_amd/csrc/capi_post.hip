// C-ABI of the joint posterior at a set of query points (include/sls_hip.h: sls_gp_predict_cov, sls_gp_sample_posterior,
// sls_random_normal): host orchestration of kernels_post.hip and the tile products of kernels_tri.hip.  No CPU fallback.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <shared_mutex>

#include "common.hpp"
#include "kernels.hpp"

using namespace slsk;

namespace {

constexpr int POST_MAX_M = 8192;   // the largest factorisation this library has measured (README: potrf sizes)

// Device blocks of one call (pool-backed: a repeated call of the same shape costs no hipMalloc).
struct PostWs {
    int M = 0, Mp = 0;
    DBuf raw, XsT, ns, Ks, V, parts, mu, cov;
};

// mu (Mp) and Sigma (Mp x Mp, identity-padded) of the M query points Xs (host, D x M) on the context's stream.
//   prep (scaled coordinates, norms) -> cross_gram (K* and the mean's partial sums) -> finalize (mu) ->
//   V = K* L^-T (triangular: k < 128 (tn + 1)) -> post_cov (K(Xs, Xs) - V V^T, lower tiles + mirror)
void post_cov_device(const GpView& g, const double* Xs, int M, PostWs& w) {
    sls_ctx* c = g.ctx;
    const int Mp = round_up(M, 128), Np = g.Np, nbt = Np / 128;
    w.M = M;
    w.Mp = Mp;
    const size_t n = (size_t)g.D * M;
    w.raw.ensure(n);
    w.XsT.ensure((size_t)Mp * g.Dcols);
    w.ns.ensure(Mp);
    w.Ks.ensure((size_t)Mp * Np);
    w.V.ensure((size_t)Mp * Np);
    w.parts.ensure((size_t)6 * nbt * Mp);
    w.mu.ensure(Mp);
    w.cov.ensure((size_t)Mp * Mp);
    SLS_HIP(hipMemcpyAsync(w.raw.p, Xs, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    KernelSpec ks{g.kernel, g.a};
    double* mu_part = w.parts.p;
    double* ca_part = mu_part + (size_t)nbt * Mp;
    double* kw_part = ca_part + (size_t)nbt * Mp;   // finalize reads these sums; mu does not depend on them
    double* cw_part = kw_part + (size_t)2 * nbt * Mp;
    {
        ProfScope ps(c, "cross_gram");
        launch_prep_points(c->stream, w.raw.p, g.D, M, g.inv_ell, w.XsT.p, Mp, Mp, g.Dcols, w.ns.p);
        // Matern also writes the derivative weights C*: V's block is free until the triangular product overwrites it
        double* Cs = g.kernel == SLS_KERNEL_ARD_MATERN52 ? w.V.p : w.Ks.p;
        if (g.gram_direct)   // beyond the guard of the norm expansion (kernels.hpp): both Gram terms from the raw coordinate differences
            launch_cross_gram_direct(c->stream, w.raw.p, g.D, 1, M, Mp, g.X, g.D, g.inv_ell, Np, g.N, ks, g.alpha, w.Ks.p, Cs, Mp, mu_part,
                                     ca_part);
        else
            launch_cross_gram(c->stream, w.XsT.p, Mp, w.ns.p, Mp, g.XT, g.Np, g.nx, Np, g.N, g.Dp, ks, g.alpha, w.Ks.p, Cs, Mp, mu_part,
                              ca_part);
    }
    {
        ProfScope ps(c, "finalize");
        SLS_HIP(hipMemsetAsync(kw_part, 0, (size_t)4 * nbt * Mp * sizeof(double), c->stream));
        FinalizeArgs f;
        f.S = M; f.D = g.D; f.nbt = nbt; f.ldk = Mp; f.ntm = Mp / 128; f.split_first = 0x7fffffff;
        f.mu_part = mu_part; f.ca_part = ca_part; f.kw_part = kw_part; f.cw_part = cw_part;
        f.Gs = nullptr; f.Gm = nullptr; f.XsT = w.XsT.p; f.inv_ell = g.inv_ell;
        f.a = g.a; f.mu_best = 0.0; f.ucb_h = 0.0; f.acq = SLS_ACQ_EXPECTED_IMPROVEMENT;
        f.ldo = Mp;
        f.mu = w.mu.p; f.sigma = nullptr; f.dmu = nullptr; f.dsigma = nullptr; f.val = nullptr; f.grad = nullptr;
        launch_finalize(c->stream, f);
    }
    {
        ProfScope ps(c, "post_v");
        // V[m + j Mp] = sum_{i <= j} K*[m + i Mp] Linv[j + i Np]  (L^-1 is zero above its diagonal: tile column tn reads k < 128 (tn + 1))
        launch_gemm_rhs_lower(c->stream, w.Ks.p, Mp, g.Linv, Np, w.V.p, Mp, Mp / 128, nbt);
    }
    {
        ProfScope ps(c, "post_cov");
        // a Laplace handle: cov = K - V T V^T, the second factor Y = V T one plain product (K* is no longer needed: its block)
        const double* V2 = nullptr;
        if (g.laplace) {
            launch_gemm_plain(c->stream, w.V.p, Mp, false, g.lap_T, Np, false, w.Ks.p, Mp, Mp / 128, nbt, Np, 1.0, 0.0);
            V2 = w.Ks.p;
        }
        if (g.gram_direct) launch_post_cov_direct(c->stream, w.raw.p, g.D, g.inv_ell, w.V.p, Mp, Np, Mp, M, ks, w.cov.p, V2);
        else launch_post_cov(c->stream, w.XsT.p, Mp, g.Dp, w.ns.p, w.V.p, Mp, Np, Mp, M, ks, w.cov.p, V2);
    }
}

}  // namespace

extern "C" int sls_gp_predict_cov(sls_gp* gp, const double* Xs, int M, double* mu, double* cov) {
    SLS_TRY
    SLS_REQUIRE(gp != nullptr, "sls_gp_predict_cov: gp is NULL");
    SLS_REQUIRE(M >= 0, "sls_gp_predict_cov: M = %d", M);
    if (M > POST_MAX_M) {
        set_error("sls_gp_predict_cov: M = %d exceeds %d query points", M, POST_MAX_M);
        return SLS_ERR_UNSUPPORTED;
    }
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Xs && cov, "sls_gp_predict_cov: Xs / cov is NULL");
    GpReadCall call(gp);
    sls_ctx* c = call.g.ctx;
    PostWs w;
    post_cov_device(call.g, Xs, M, w);
    SLS_HIP(hipMemcpy2DAsync(cov, (size_t)M * 8, w.cov.p, (size_t)w.Mp * 8, (size_t)M * 8, M, hipMemcpyDeviceToHost, c->stream));
    if (mu) SLS_HIP(hipMemcpyAsync(mu, w.mu.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    SLS_CATCH
}

extern "C" int sls_gp_sample_posterior(sls_gp* gp, const double* Xs, int M, int n_samples, unsigned long long seed, double* samples,
                                       double* jitter_used) {
    SLS_TRY
    SLS_REQUIRE(gp != nullptr, "sls_gp_sample_posterior: gp is NULL");
    SLS_REQUIRE(M >= 0 && n_samples >= 1, "sls_gp_sample_posterior: M = %d, n_samples = %d", M, n_samples);
    if (M > POST_MAX_M) {
        set_error("sls_gp_sample_posterior: M = %d exceeds %d query points", M, POST_MAX_M);
        return SLS_ERR_UNSUPPORTED;
    }
    if (M == 0) {
        if (jitter_used) *jitter_used = 0.0;
        return SLS_OK;
    }
    SLS_REQUIRE(Xs && samples, "sls_gp_sample_posterior: Xs / samples is NULL");
    GpReadCall call(gp);
    sls_ctx* c = call.g.ctx;
    PostWs w;
    post_cov_device(call.g, Xs, M, w);
    const int Mp = w.Mp;
    // chol(Sigma + j I) on a copy: Sigma stays intact for the next jitter of the schedule
    DBuf Ls, Tinv, flag;
    Ls.ensure((size_t)Mp * Mp);
    Tinv.ensure((size_t)Mp * Mp);
    flag.ensure(1);
    // jitter schedule (relative to a): 0, then 1e-12 .. 1e-6 in factors of ten
    static const double sched[] = {0.0, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6};
    const int nsched = (int)(sizeof(sched) / sizeof(sched[0]));
    int step = 0, giveups = 0;
    double jit = 0.0;
    bool ok = false;
    while (step < nsched) {
        jit = sched[step] * call.g.a;
        SLS_HIP(hipMemcpyAsync(Ls.p, w.cov.p, (size_t)Mp * Mp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if (jit > 0.0) launch_add_diag(c->stream, Ls.p, Mp, M, jit);
        SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
        c->potrf_tick_rearm();
        int* df_sync = c->potrf_df_sync(Mp);
        {
            ProfScope ps(c, "post_potrf");
            launch_potrf(c->stream, Ls.p, Mp, Tinv.p, c->d_info, 0, df_sync);
        }
        // An exactly singular cov (duplicate query points) leaves a pivot of rounding size whose SIGN is an accident of the
        // summation order: a pivot L_ii^2 <= M eps a counts as non-positive too, so that such a cov always takes the jitter.
        launch_pivot_check(c->stream, Ls.p, Mp, M, (double)M * 0x1p-52 * call.g.a, reinterpret_cast<int*>(flag.p));
        int info[3] = {0, 0, 0};
        SLS_HIP(hipMemcpyAsync(info, c->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SLS_HIP(hipMemcpyAsync(info + 2, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SLS_HIP(hipStreamSynchronize(c->stream));
        if (potrf_gave_up(c, info[1], giveups)) {   // the single-launch form gave up: the same jitter once more, on the multi-launch schedule
            ++giveups;
            continue;
        }
        if (info[0] == 0 && info[2] == 0) {
            ok = true;
            break;
        }
        ++step;
    }
    if (!ok) {
        set_error("sls_gp_sample_posterior: cov + %g I is not positive definite (jitter schedule up to 1e-6 a exhausted)", jit);
        return SLS_ERR_NOT_SPD;
    }
    if (jitter_used) *jitter_used = jit;
    // potrf leaves the upper triangles of its diagonal blocks as they were; the sample product reads those blocks whole
    launch_zero_diag_upper(c->stream, Ls.p, Mp);
    // F = mu 1^T + L_S Z, chunked over samples: sample s at point j uses normal number s M + j whatever the chunk
    const int chunk = std::max(128, ((1 << 24) / Mp) / 128 * 128);
    const int cmax = std::min(round_up(n_samples, 128), chunk);
    DBuf Zt, F;
    Zt.ensure((size_t)cmax * Mp);
    F.ensure((size_t)cmax * Mp);
    for (int s0 = 0; s0 < n_samples; s0 += cmax) {
        const int sc = std::min(cmax, n_samples - s0), Scp = round_up(sc, 128);
        {
            ProfScope ps(c, "post_sample");
            launch_normal_fill(c->stream, seed, s0, sc, Scp, M, Mp, Zt.p, Scp);
            launch_bcast_cols(c->stream, w.mu.p, Mp, F.p, Mp, Scp);
            launch_gemm_lhs_lower(c->stream, Ls.p, Mp, Zt.p, Scp, F.p, Mp, Mp / 128, Scp / 128, 1.0, 1.0);
        }
        SLS_HIP(hipMemcpy2DAsync(samples + (size_t)s0 * M, (size_t)M * 8, F.p, (size_t)Mp * 8, (size_t)M * 8, sc, hipMemcpyDeviceToHost,
                                 c->stream));
    }
    SLS_HIP(hipStreamSynchronize(c->stream));
    SLS_CATCH
}

extern "C" int sls_random_normal(sls_ctx* ctx, unsigned long long seed, long offset, long n, double* out) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx != nullptr, "sls_random_normal: ctx is NULL");
    SLS_REQUIRE(offset >= 0 && n >= 0, "sls_random_normal: offset = %ld, n = %ld", offset, n);
    if (n == 0) return SLS_OK;
    SLS_REQUIRE(out != nullptr, "sls_random_normal: out is NULL");
    SLS_HIP(hipSetDevice(ctx->device));
    const long chunk = std::min(n, 1L << 24);
    DBuf buf;
    buf.ensure((size_t)chunk);
    for (long i0 = 0; i0 < n; i0 += chunk) {
        const long m = std::min(chunk, n - i0);
        launch_random_normal(ctx->stream, seed, offset + i0, m, buf.p);
        SLS_HIP(hipMemcpyAsync(out + i0, buf.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SLS_HIP(hipStreamSynchronize(ctx->stream));   // buf is refilled by the next chunk
    }
    SLS_CATCH
}
