// C-ABI of the pathwise posterior function draws (include/sls_hip.h: sls_path_*, and sls_qeubo_* / sls_qnei_* on them): host orchestration of
// kernels_path.hip and kernels_qeubo.hip, the cross Gram / gradient products of kernels_gram.hip / kernels_acq.hip, the tile GEMM
// and block solve of kernels_tri.hip and the lock-step L-BFGS rounds of lbfgs_driver.hpp.  No CPU fallback.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "lbfgs_driver.hpp"
#include "sub_maps.hpp"

using namespace slsk;

namespace {

constexpr int PATH_MAX_DRAWS = 4096;
constexpr int PATH_MAX_FREQ = 16384;

int* ints(DBuf& b, size_t n) {
    b.ensure((n + 1) / 2);
    return reinterpret_cast<int*>(b.p);
}

}  // namespace

struct sls_path {
    sls_gp* gp = nullptr;
    sls_ctx* ctx = nullptr;
    long generation = 0;
    int D = 0, N = 0, Np = 0, kernel = 0, n_draws = 0, F = 0, Fp = 0, Rp = 0;
    // the only state kept between calls (workspaces are per call and go back to the device pool at its end):
    // Om [l + d*Fp] (Fp x Dcols), W [r + s*2Fp] (cos rows, then sin rows; 2Fp x Rp), V [i + s*Np] (Np x Rp)
    DBuf Om, W, V;
};

namespace {

// candidates per device pass: the chunk x Np blocks (K*, C*, Pm) and the chunk x 2Fp block (G / Phi) stay below 2^26 doubles each
int chunk_of(int Np, int Fp) { return std::max(128, std::min(16384, ((1 << 26) / std::max(Np, 2 * Fp)) / 128 * 128)); }

// Device blocks of one evaluation pass (one call)
struct EvalWs {
    // Pm and G share one block: G = Pm + Cp Np (same leading dimension), so that [Pm | G] is ONE operand of the gradient contraction
    // against B2 = [X~ ; Om] (k-stacked, built once per call)
    // Gd: the data term's gradient contraction over raw coordinate differences, for handles beyond the guard of the norm expansion
    DBuf XsT, ns, Ks, Cs, PG, csum, vpart, Gt, B2, Gpart, Gd;
    bool b2_ready = false;
    void ensure(const sls_path* p, const GpView& g, int chunk) {
        const size_t C = chunk, Np = g.Np;
        if (g.gram_direct) Gd.ensure(C * g.Dcols);
        XsT.ensure(C * g.Dcols);
        ns.ensure(C);
        Ks.ensure(C * Np);
        if (g.kernel == SLS_KERNEL_ARD_MATERN52) Cs.ensure(C * Np);
        PG.ensure(C * (Np + 2 * (size_t)p->Fp));
        csum.ensure(C);
        vpart.ensure(C * (size_t)(p->Fp / 128));
        Gt.ensure(C * g.Dcols);
    }
};

// S candidates at raw coordinates xr: candidate-major xr[n + d*ldr], or point-major xr[d + n*D].
//   draw != nullptr (device, S ints): val[n] = f_{draw[n]}(x_n), grad[n + d*ldgrad] (may be nullptr);
//   draw == nullptr: val[n + s*ldall] = f_s(x_n) for every draw s (val has Rp columns), no gradient.
// Per chunk: cross_gram (K*, C*) -> the random-feature contraction on the matrix cores (path_feat) -> gathered form: chunk sums of the
// value, data term (path_data), gradient = G Om^T + Pm X~^T on the tile GEMM (path_grad); every-draw form: Phi^T W on the tile GEMM,
// then the data term.
void path_eval_device(sls_path* p, const GpView& g, EvalWs& w, const double* xr, long ldr, bool point_major, int S, const int* draw,
                      double* val, long ldall, double* grad, long ldgrad) {
    sls_ctx* c = g.ctx;
    const int D = g.D, Np = g.Np, Fp = p->Fp;
    const int chunk_max = std::min(round_up(S, 128), chunk_of(Np, Fp));
    w.ensure(p, g, chunk_max);
    KernelSpec ks{g.kernel, g.a};
    double* Cs = g.kernel == SLS_KERNEL_ARD_MATERN52 ? w.Cs.p : w.Ks.p;
    const long Kc = (long)Np + Fp;   // depth of the gradient contraction [Pm | G] [X~ ; Om]
    if (grad && !g.gram_direct && !w.b2_ready) {
        w.B2.ensure((size_t)Kc * g.Dcols);
        SLS_HIP(hipMemcpy2DAsync(w.B2.p, Kc * 8, g.XT, (size_t)Np * 8, (size_t)Np * 8, g.Dcols, hipMemcpyDeviceToDevice, c->stream));
        SLS_HIP(hipMemcpy2DAsync(w.B2.p + Np, Kc * 8, p->Om.p, (size_t)Fp * 8, (size_t)Fp * 8, g.Dcols, hipMemcpyDeviceToDevice, c->stream));
        w.b2_ready = true;
    }
    for (int s0 = 0; s0 < S; s0 += chunk_max) {
        const int sc = std::min(chunk_max, S - s0), Cp = round_up(sc, 128);
        double* Pm = w.PG.p;
        double* G = w.PG.p + (size_t)Cp * Np;
        {
            ProfScope ps(c, "cross_gram");
            if (point_major) launch_prep_points(c->stream, xr + (size_t)s0 * D, D, sc, g.inv_ell, w.XsT.p, Cp, Cp, g.Dcols, w.ns.p);
            else launch_prep_cands(c->stream, xr + s0, ldr, D, sc, g.inv_ell, w.XsT.p, Cp, Cp, g.Dcols, w.ns.p);
            if (g.gram_direct)   // beyond the guard of the norm expansion (kernels.hpp): the data term from the raw coordinate differences
                launch_cross_gram_direct(c->stream, point_major ? xr + (size_t)s0 * D : xr + s0, point_major ? D : 1, point_major ? 1 : ldr, sc,
                                         Cp, g.X, D, g.inv_ell, Np, g.N, ks, nullptr, w.Ks.p, Cs, Cp, nullptr, nullptr);
            else
                launch_cross_gram(c->stream, w.XsT.p, Cp, w.ns.p, Cp, g.XT, g.Np, g.nx, Np, g.N, g.Dp, ks, nullptr, w.Ks.p, Cs, Cp,
                                  nullptr, nullptr);
        }
        if (!draw) {
            {
                ProfScope ps(c, "path_prior");
                launch_path_feat(c->stream, w.XsT.p, Cp, g.Dp, Cp, p->Om.p, Fp, p->W.p, 2L * Fp, nullptr, sc, G, Cp, nullptr, 0);
                launch_gemm_plain(c->stream, G, Cp, false, p->W.p, 2L * Fp, true, val + s0, ldall, Cp / 128, p->Rp / 128, 2 * Fp, 1.0,
                                  0.0);
            }
            ProfScope ps(c, "path_data");
            launch_path_data(c->stream, w.Ks.p, Cs, Cp, g.N, Np, p->V.p, Np, nullptr, sc, ldall, sc * p->n_draws, val + s0, nullptr,
                             nullptr);
            continue;
        }
        {
            ProfScope ps(c, "path_prior");
            launch_path_feat(c->stream, w.XsT.p, Cp, g.Dp, Cp, p->Om.p, Fp, p->W.p, 2L * Fp, draw + s0, sc, G, Cp, w.vpart.p, Cp);
            launch_path_vsum(c->stream, w.vpart.p, Cp, Fp / 128, sc, val + s0);
        }
        {
            ProfScope ps(c, "path_data");
            launch_path_data(c->stream, w.Ks.p, Cs, Cp, g.N, Np, p->V.p, Np, draw + s0, 0, 0, sc, val + s0, grad ? Pm : nullptr,
                             w.csum.p);
        }
        if (grad && g.gram_direct) {
            // Beyond the guard: Gt = G Om alone (Fp deep) and the data term over raw coordinate differences (grad_direct).  In the one
            // contraction below the accumulator carries x~* sum_i c_i (|x~| ~ 1 / (2 l)) through the Fp additions of the prior and
            // loses it again only in path_grad: eps |x~| |csum| sqrt(Fp) / l, 20 times the rounding of the terms themselves at
            // F = 16384, l = 3e-3.
            {
                ProfScope ps(c, "path_grad_gemm");
                double* part = nullptr;
                if (D <= 64 && grad_gemm_wants_split(Cp)) {
                    w.Gpart.ensure((size_t)8 * Cp * 64);
                    part = w.Gpart.p;
                }
                launch_grad_gemm(c->stream, G, nullptr, Cp, Cp, p->Om.p, nullptr, Fp, Fp, D <= 64 ? -g.Dcols : g.Dcols, w.Gt.p, nullptr, part, 1);
                launch_grad_direct(c->stream, Pm, nullptr, Cp, Cp, point_major ? xr + (size_t)s0 * D : xr + s0, point_major ? D : 1,
                                   point_major ? 1 : ldr, sc, g.X, D, g.inv_ell, g.N, nullptr, w.Gd.p, nullptr);
            }
            ProfScope ps(c, "path_data");
            launch_path_grad_direct(c->stream, sc, D, Cp, w.Gt.p, w.Gd.p, g.inv_ell, grad + s0, ldgrad);
        } else if (grad) {
            {
                // Gt = [Pm | G] [X~ ; Om]: X~^T c of the data term plus the prior's gradient in scaled coordinates, ONE MFMA contraction
                // (Np + Fp deep) on grad_gemm's P-pass alone (fixed quarter order: a candidate's bits do not depend on the launch)
                ProfScope ps(c, "path_grad_gemm");
                double* part = nullptr;
                if (D <= 64 && grad_gemm_wants_split(Cp)) {
                    w.Gpart.ensure((size_t)8 * Cp * 64);
                    part = w.Gpart.p;
                }
                launch_grad_gemm(c->stream, Pm, nullptr, Cp, Cp, w.B2.p, nullptr, Kc, (int)Kc, D <= 64 ? -g.Dcols : g.Dcols, w.Gt.p, nullptr,
                                 part, 1);
            }
            ProfScope ps(c, "path_data");
            launch_path_grad(c->stream, sc, D, Cp, w.Gt.p, w.XsT.p, w.csum.p, g.inv_ell, grad + s0, ldgrad);
        }
    }
}

}  // namespace

extern "C" int sls_path_create(sls_gp* gp, int n_draws, int n_freq, unsigned long long seed, sls_path** out) {
    SLS_TRY
    SLS_REQUIRE(gp && out, "sls_path_create: NULL argument");
    *out = nullptr;
    SLS_REQUIRE(n_draws >= 1 && n_draws <= PATH_MAX_DRAWS, "sls_path_create: n_draws = %d (1 .. %d)", n_draws, PATH_MAX_DRAWS);
    SLS_REQUIRE(n_freq >= 1 && n_freq <= PATH_MAX_FREQ, "sls_path_create: n_freq = %d (1 .. %d)", n_freq, PATH_MAX_FREQ);
    GpReadCall call(gp);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    SLS_REQUIRE((long)g.N * n_draws < INT_MAX, "sls_path_create: N n_draws = %ld is too large", (long)g.N * n_draws);
    std::unique_ptr<sls_path> p(new sls_path);
    p->gp = gp; p->ctx = c; p->generation = g.generation;
    p->D = g.D; p->N = g.N; p->Np = g.Np; p->kernel = g.kernel; p->n_draws = n_draws; p->F = n_freq;
    p->Fp = round_up(n_freq, 128);
    p->Rp = round_up(n_draws, 128);
    const int F = n_freq, Fp = p->Fp, D = g.D, N = g.N, Np = g.Np, Rp = p->Rp;
    const bool matern = g.kernel == SLS_KERNEL_ARD_MATERN52;
    const long B0 = (long)F * D + (matern ? 5L * F : 0L);
    const long nE = (long)n_draws * (2L * F + N);
    DBuf Z, E, Phi;
    Z.ensure((size_t)B0);
    E.ensure((size_t)nE);
    p->Om.ensure((size_t)Fp * g.Dcols);
    p->W.ensure((size_t)2 * Fp * Rp);
    p->V.ensure((size_t)Np * Rp);
    {
        ProfScope ps(c, "path_setup");
        launch_random_normal(c->stream, seed, 0, B0, Z.p);
        launch_random_normal(c->stream, seed, B0, nE, E.p);
        launch_path_omega(c->stream, Z.p, F, Fp, D, g.Dcols, matern ? 1 : 0, p->Om.p);
        launch_path_weights(c->stream, E.p, F, Fp, N, n_draws, Rp, std::sqrt(g.a / F), p->W.p);
        // f_prior,s(x_i) for every draw into V's block (Phi_X^T W, row blocks of the training points), then r = y - sqrt(b) eps - f_prior
        const int rows = std::max(128, std::min(Np, ((1 << 26) / (2 * Fp)) / 128 * 128));
        Phi.ensure((size_t)rows * 2 * Fp);
        for (int i0 = 0; i0 < Np; i0 += rows) {
            const int rc = std::min(rows, Np - i0);
            launch_path_feat(c->stream, g.XT + i0, Np, g.Dp, rc, p->Om.p, Fp, p->W.p, 2L * Fp, nullptr, rc, Phi.p, rc, nullptr, 0);
            launch_gemm_plain(c->stream, Phi.p, rc, false, p->W.p, 2L * Fp, true, p->V.p + i0, Np, rc / 128, Rp / 128, 2 * Fp, 1.0, 0.0);
        }
        launch_path_rhs(c->stream, g.y, E.p, F, N, Np, n_draws, Rp, std::sqrt(g.b), p->V.p);
    }
    {
        ProfScope ps(c, "path_solve");
        launch_potrs(c->stream, g.L, g.Linv, Np, p->V.p, Rp);
    }
    SLS_HIP(hipStreamSynchronize(c->stream));
    ctx_retain(c);
    *out = p.release();
    SLS_CATCH
}

extern "C" int sls_path_destroy(sls_path* p) {
    if (!p) return SLS_OK;
    destroy_handle(p);
    return SLS_OK;
}

extern "C" int sls_path_eval(sls_path* p, const double* Xs, int M, const int* draw_of_point, double* val, double* grad) {
    SLS_TRY
    SLS_REQUIRE(p != nullptr, "sls_path_eval: p is NULL");
    SLS_REQUIRE(M >= 0, "sls_path_eval: M = %d", M);
    SLS_REQUIRE(draw_of_point || !grad, "sls_path_eval: grad must be NULL when draw_of_point is NULL (every-draw form)");
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Xs && val, "sls_path_eval: Xs / val is NULL");
    if (draw_of_point)
        for (int m = 0; m < M; ++m)
            SLS_REQUIRE(draw_of_point[m] >= 0 && draw_of_point[m] < p->n_draws, "sls_path_eval: draw_of_point[%d] = %d (n_draws = %d)", m,
                        draw_of_point[m], p->n_draws);
    GpReadCall call(p->gp, p->generation, "sls_path_eval");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, Mp = round_up(M, 128), nd = p->n_draws;
    DBuf raw, vout, gout, dbuf;
    raw.ensure((size_t)D * M);
    h2d(c, raw.p, Xs, (size_t)D * M);
    if (draw_of_point) {
        int* d_draw = ints(dbuf, (size_t)M);
        SLS_HIP(hipMemcpyAsync(d_draw, draw_of_point, (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
        vout.ensure(Mp);
        if (grad) gout.ensure((size_t)Mp * D);
        EvalWs ws;
        path_eval_device(p, g, ws, raw.p, 0, true, M, d_draw, vout.p, 0, grad ? gout.p : nullptr, Mp);
        d2h(c, val, vout.p, (size_t)M);
        std::vector<double> gh(grad ? (size_t)Mp * D : 0);
        if (grad) d2h(c, gh.data(), gout.p, gh.size());
        SLS_HIP(hipStreamSynchronize(c->stream));
        cm_to_host(gh.data(), Mp, D, M, grad);
    } else {
        vout.ensure((size_t)Mp * p->Rp);
        EvalWs ws;
        path_eval_device(p, g, ws, raw.p, 0, true, M, nullptr, vout.p, Mp, nullptr, 0);
        SLS_HIP(hipMemcpy2DAsync(val, (size_t)M * 8, vout.p, (size_t)Mp * 8, (size_t)M * 8, nd, hipMemcpyDeviceToHost, c->stream));
        SLS_HIP(hipStreamSynchronize(c->stream));
    }
    SLS_CATCH
}

extern "C" int sls_path_maximize(sls_path* p, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts, double* x_out,
                                 double* val_out, long* idx_out) {
    SLS_TRY
    SLS_REQUIRE(p && starts, "sls_path_maximize: NULL argument");
    SLS_REQUIRE(S >= 1 && (long)S * p->n_draws <= (1L << 26), "sls_path_maximize: S = %d starts per draw (1 .. 2^26 / n_draws)", S);
    GpReadCall call(p->gp, p->generation, "sls_path_maximize");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws, T = S * nd, Sp = round_up(T, 128);
    // the shared prologue and search over all T = n_draws S starts at once; the winner is per DRAW, so the epilogue below is this
    // entry point's own (and sls_acq_last_stats, which speaks of one winner's run, is left alone)
    LbfgsWs lb;
    EvalWs ws;
    MultistartRun r = maximize_begin("sls_path_maximize", nullptr, lb, opts, T, n_local, D, Sp);
    const LbfgsState& st = r.st;
    int* d_draw = lb.tail();   // the draw of every live column
    DBuf sd;
    sd.ensure((size_t)D * T);
    h2d(c, sd.p, starts, (size_t)D * T);
    // f_{live[j] / S} is the objective of compacted column j
    lockstep_rounds(c, r.st, lb, sd.p, T, n_local,
                    [&](const double* trial, long ld, int nlive, const int* live, double* val, double* grad) {
                        launch_path_draw_of_live(c->stream, live, nlive, S, d_draw);
                        path_eval_device(p, g, ws, trial, ld, false, nlive, d_draw, val, 0, grad, ld);
                    },
                    nullptr);
    DBuf best;
    best.ensure((size_t)nd * (D + 2));
    launch_path_argmax(c->stream, st.f, S, nd, st.x, Sp, D, best.p);
    std::vector<double> bh((size_t)nd * (D + 2));
    d2h(c, bh.data(), best.p, bh.size());
    SLS_HIP(hipStreamSynchronize(c->stream));
    for (int s = 0; s < nd; ++s) {
        const double* b = bh.data() + (size_t)s * (D + 2);
        if (val_out) val_out[s] = b[0];
        if (idx_out) idx_out[s] = (long)b[1];
        if (x_out) std::copy(b + 2, b + 2 + D, x_out + (size_t)s * D);
    }
    SLS_CATCH
}

// ---- the draws over affine subspaces (include/sls_hip.h "maximisation over affine subspaces") ------------------------------------
namespace {

// The two blocks of a call: the expanded points x = c + A z and their gradient, D x ld doubles each, from the device pool
struct SubWs {
    DBuf x, gx;
};

// path_eval_device (gathered form) at x = c + A z: z[n + j*ld] candidate-major, n < count, column n is start live[n] (nullptr:
// identity) under draw[n]; the fold of the gradient onto z goes to grad_z[n + j*ld] (may be nullptr).
void path_sub_eval_device(sls_path* p, const GpView& g, EvalWs& ws, SubWs& sw, const SubMaps& m, const double* z, long ld, int count,
                          const int* live, const int* draw, double* val, double* grad_z) {
    sls_ctx* c = g.ctx;
    sw.x.ensure((size_t)g.D * ld);
    if (grad_z) sw.gx.ensure((size_t)g.D * ld);
    sub_expand(c, m, count, live, z, ld, sw.x.p, ld);
    path_eval_device(p, g, ws, sw.x.p, ld, false, count, draw, val, 0, grad_z ? sw.gx.p : nullptr, ld);
    if (grad_z) sub_fold(c, m, count, live, sw.gx.p, ld, grad_z, ld);
}

}  // namespace

extern "C" int sls_path_eval_sub(sls_path* p, const sls_submaps* maps, const double* Z, int M, const int* draw_of_point, double* val,
                                 double* grad_z, double* X_out) {
    SLS_TRY
    SLS_REQUIRE(p != nullptr, "sls_path_eval_sub: p is NULL");
    SLS_REQUIRE(M >= 0, "sls_path_eval_sub: M = %d", M);
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(draw_of_point != nullptr, "sls_path_eval_sub: draw_of_point is NULL (the every-draw form has no _sub call)");
    SLS_REQUIRE(Z && val, "sls_path_eval_sub: Z / val is NULL");
    for (int m = 0; m < M; ++m)
        SLS_REQUIRE(draw_of_point[m] >= 0 && draw_of_point[m] < p->n_draws, "sls_path_eval_sub: draw_of_point[%d] = %d (n_draws = %d)", m,
                    draw_of_point[m], p->n_draws);
    GpReadCall call(p->gp, p->generation, "sls_path_eval_sub");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    SubMapsDev up;
    upload_sub_maps("sls_path_eval_sub", c, maps, g.D, M, up);
    const int D = g.D, d = up.m.d, Mp = round_up(M, 128);
    const std::vector<double> zh = host_to_cm(Z, d, M, Mp);
    DBuf zd, vout, gout, dbuf;
    zd.ensure(zh.size());
    h2d(c, zd.p, zh.data(), zh.size());
    int* d_draw = ints(dbuf, (size_t)M);
    SLS_HIP(hipMemcpyAsync(d_draw, draw_of_point, (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
    vout.ensure(Mp);
    if (grad_z) gout.ensure((size_t)Mp * d);
    EvalWs ws;
    SubWs sw;
    path_sub_eval_device(p, g, ws, sw, up.m, zd.p, Mp, M, nullptr, d_draw, vout.p, grad_z ? gout.p : nullptr);
    d2h(c, val, vout.p, (size_t)M);
    std::vector<double> gh(grad_z ? (size_t)Mp * d : 0), xh(X_out ? (size_t)Mp * D : 0);
    if (grad_z) d2h(c, gh.data(), gout.p, gh.size());
    if (X_out) d2h(c, xh.data(), sw.x.p, xh.size());
    SLS_HIP(hipStreamSynchronize(c->stream));
    cm_to_host(gh.data(), Mp, d, M, grad_z);
    cm_to_host(xh.data(), Mp, D, M, X_out);
    SLS_CATCH
}

extern "C" int sls_path_maximize_sub(sls_path* p, const sls_submaps* maps, const double* starts_z, int S, int n_local,
                                     const sls_lbfgs_opts* opts, double* z_out, double* x_out, double* val_out, long* idx_out) {
    SLS_TRY
    SLS_REQUIRE(p && starts_z, "sls_path_maximize_sub: NULL argument");
    SLS_REQUIRE(S >= 1 && (long)S * p->n_draws <= (1L << 26), "sls_path_maximize_sub: S = %d starts per draw (1 .. 2^26 / n_draws)", S);
    GpReadCall call(p->gp, p->generation, "sls_path_maximize_sub");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws, T = S * nd, Sp = round_up(T, 128);
    SubMapsDev up;
    upload_sub_maps("sls_path_maximize_sub", c, maps, D, T, up);
    const int d = up.m.d;
    // sls_path_maximize in the d variables: all T = n_draws S starts in one search, the winner per draw
    LbfgsWs lb;
    EvalWs ws;
    SubWs sw;
    MultistartRun r = maximize_begin("sls_path_maximize_sub", nullptr, lb, opts, T, n_local, d, Sp);
    const LbfgsState& st = r.st;
    int* d_draw = lb.tail();   // the draw of every live column
    DBuf sd;
    sd.ensure((size_t)d * T);
    h2d(c, sd.p, starts_z, (size_t)d * T);
    lockstep_rounds(c, r.st, lb, sd.p, T, n_local,
                    [&](const double* trial, long ld, int nlive, const int* live, double* val, double* grad) {
                        launch_path_draw_of_live(c->stream, live, nlive, S, d_draw);
                        path_sub_eval_device(p, g, ws, sw, up.m, trial, ld, nlive, live, d_draw, val, grad);
                    },
                    nullptr);
    // the points of the end variables (one more expand launch), then the per-draw first maximum once with z and once with x
    sw.x.ensure((size_t)D * Sp);
    sub_expand(c, up.m, T, nullptr, st.x, Sp, sw.x.p, Sp);
    DBuf best;
    const size_t nz = (size_t)nd * (d + 2), nx = (size_t)nd * (D + 2);
    best.ensure(nz + nx);
    launch_path_argmax(c->stream, st.f, S, nd, st.x, Sp, d, best.p);
    launch_path_argmax(c->stream, st.f, S, nd, sw.x.p, Sp, D, best.p + nz);
    std::vector<double> bh(nz + nx);
    d2h(c, bh.data(), best.p, bh.size());
    SLS_HIP(hipStreamSynchronize(c->stream));
    for (int s = 0; s < nd; ++s) {
        const double* bz = bh.data() + (size_t)s * (d + 2);
        const double* bx = bh.data() + nz + (size_t)s * (D + 2);
        if (val_out) val_out[s] = bz[0];
        if (idx_out) idx_out[s] = (long)bz[1];
        if (z_out) std::copy(bz + 2, bz + 2 + d, z_out + (size_t)s * d);
        if (x_out) std::copy(bx + 2, bx + 2 + D, x_out + (size_t)s * D);
    }
    SLS_CATCH
}

// ---- expected utility of the best of q options on the draws (include/sls_hip.h) ---------------------------------------------
namespace {

// Sets per pass.  points = q sets; every points-sized block -- values / mask (points x Rp), Wbar (2Fp x points), Vbar (Np x points),
// K*, C* (points x Np), [Pm | G] (points x (Np + 2Fp): the features of the every-draw form use G's 2Fp columns) -- stays below 2^26
// doubles, and points stay within the context's candidate chunk; whole 128-set tiles, never fewer than one.  That floor is the ONE
// exception to both bounds: a pass then holds 128 q points (at most 2048) whatever they say -- a candidate chunk below 128 q, or
// max(Rp, Np + 2 Fp) > 2^26 / (128 q) (e.g. q = 16 with Np + 2 Fp > 32768).  Blocks may then exceed 2^26 doubles; every index into
// them is a long, so the bound is one on memory, not on addressing (at most 2048 x (8192 + 2 x 16384) doubles = 640 MB for [Pm | G]
// at the largest N this library factorises).
int qeubo_sets_per_pass(const sls_ctx* c, int q, int Np, int Fp, int Rp) {
    const int points = std::min(c->cand_chunk, (1 << 26) / std::max(Rp, Np + 2 * Fp));
    return std::max(128, points / q / 128 * 128);
}

// What the selection of a pass computes: qEUBO (base == nullptr), qNEI (base: n_draws device doubles, the per-draw baseline) or
// qLogNEI (log_form, with base and the two temperatures).
struct SetMode {
    const double* base = nullptr;
    bool log_form = false;
    double tau_relu = 0.0, tau_max = 0.0;
};

struct QeuboWs {
    DBuf XsT, ns, Ks, Cs, PG, csum, vpart, Gt, B2, Gpart, Gd, VM, Wbar, Vbar, sum, fbar, gpt, badb, identb;
    DBuf lmq, lzq, lpmx, lpsm, lpbadb, lpwinb;   // the scratch of the log-form selection (launch_qlognei_select)
    int *lpbad = nullptr, *lpwin = nullptr;
    void ensure_log(const sls_path* p, int q, int Sp) {
        const size_t nsl = (size_t)qlognei_slices(p->n_draws);
        lmq.ensure((size_t)Sp * p->Rp);
        lzq.ensure((size_t)Sp * p->Rp);
        lpmx.ensure((size_t)Sp * nsl);
        lpsm.ensure((size_t)Sp * nsl);
        lpbad = ints(lpbadb, (size_t)Sp * nsl);
        lpwin = ints(lpwinb, (size_t)Sp * nsl * q);
    }
    bool b2_ready = false;
    int* bad = nullptr;     // one flag per set of the pass
    int* ident = nullptr;   // ident[j] = j: point j is evaluated under aggregated column j
    int ident_n = 0;
    // values_only: the blocks of the every-draw values alone (sls_path_max_over_points)
    void ensure(sls_ctx* c, const sls_path* p, const GpView& g, int Pp, int Sp, bool values_only = false) {
        const size_t P = Pp, Np = g.Np, Fp = p->Fp;
        XsT.ensure(P * g.Dcols);
        ns.ensure(P);
        Ks.ensure(P * Np);
        if (g.kernel == SLS_KERNEL_ARD_MATERN52) Cs.ensure(P * Np);
        PG.ensure(P * (Np + 2 * Fp));
        VM.ensure(P * p->Rp);
        if (values_only) return;
        csum.ensure(P);
        vpart.ensure(P * (Fp / 128));
        Gt.ensure(P * g.Dcols);
        if (g.gram_direct) Gd.ensure(P * g.Dcols);
        Wbar.ensure(2 * Fp * P);
        Vbar.ensure(Np * P);
        sum.ensure(Sp);
        fbar.ensure(P);
        gpt.ensure(P * g.D);
        bad = ints(badb, (size_t)Sp);
        if (Pp > ident_n) {
            ident = ints(identb, (size_t)Pp);
            launch_path_draw_of_live(c->stream, nullptr, Pp, 1, ident);
            ident_n = Pp;
        }
    }
};

// Every draw at the Pp points of a pass into w.VM (Pp x Rp): `prep` fills XsT / ns, then cross_gram, Phi^T W and K* V accumulated onto
// it, both on the tile GEMM.  `direct(ks, Cs)`: the cross Gram of the same points from their raw coordinates, for handles beyond the
// guard of the norm expansion (kernels.hpp).
template <class Prep, class Direct>
void draw_values_device(sls_path* p, const GpView& g, QeuboWs& w, int Pp, Prep&& prep, Direct&& direct) {
    sls_ctx* c = g.ctx;
    const int Np = g.Np, Fp = p->Fp, Rp = p->Rp;
    KernelSpec ks{g.kernel, g.a};
    double* Cs = g.kernel == SLS_KERNEL_ARD_MATERN52 ? w.Cs.p : w.Ks.p;
    double* G = w.PG.p + (size_t)Pp * Np;
    {
        ProfScope ps(c, "cross_gram");
        prep();
        if (g.gram_direct) direct(ks, Cs);
        else launch_cross_gram(c->stream, w.XsT.p, Pp, w.ns.p, Pp, g.XT, g.Np, g.nx, Np, g.N, g.Dp, ks, nullptr, w.Ks.p, Cs, Pp, nullptr, nullptr);
    }
    {
        ProfScope ps(c, "path_prior");
        launch_path_feat(c->stream, w.XsT.p, Pp, g.Dp, Pp, p->Om.p, Fp, p->W.p, 2L * Fp, nullptr, Pp, G, Pp, nullptr, 0);
        launch_gemm_plain(c->stream, G, Pp, false, p->W.p, 2L * Fp, true, w.VM.p, Pp, Pp / 128, Rp / 128, 2 * Fp, 1.0, 0.0);
    }
    {
        ProfScope ps(c, "qeubo_data_gemm");
        launch_gemm_plain(c->stream, w.Ks.p, Pp, false, p->V.p, Np, true, w.VM.p, Pp, Pp / 128, Rp / 128, Np, 1.0, 1.0);
    }
}

// qEUBO (+ its qD gradient and the win counts; val, grad, wins may each be nullptr) at M sets, candidate-major raw coordinates
// xr[n + r*ldr], rows iD..iD+D-1 the option i.  val[n], grad[n + r*ldo], wins[n + i*ldw].  The gradient is formed, and looked at by the
// guard, whether or not it is asked for: a set's value does not depend on that.
// base != nullptr (device, n_draws doubles): qNEI -- the selection competes against the per-draw baseline, the guard value is 0 and
// the two kernels count under "qnei".  mode.log_form: qLogNEI -- the selection is launch_qlognei_select (real weights in place of the
// mask), the finish divides nothing, the guard value is SLS_QEUBO_FLOOR and the launches count under "qlognei".
void qeubo_eval_device(sls_path* p, const GpView& g, QeuboWs& w, int q, const SetMode& mode, const double* xr, long ldr, int M,
                       double* val, double* grad, long ldo, int* wins, long ldw) {
    sls_ctx* c = g.ctx;
    const double* base = mode.base;
    const char* scope = mode.log_form ? "qlognei" : base ? "qnei" : "qeubo";
    const double floor = base && !mode.log_form ? 0.0 : SLS_QEUBO_FLOOR;
    const int D = g.D, Np = g.Np, Fp = p->Fp, Rp = p->Rp, S = p->n_draws;
    const int pass_max = std::min(round_up(M, 128), qeubo_sets_per_pass(c, q, Np, Fp, Rp));
    w.ensure(c, p, g, q * pass_max, pass_max);
    if (mode.log_form) w.ensure_log(p, q, pass_max);
    double* Cs = g.kernel == SLS_KERNEL_ARD_MATERN52 ? w.Cs.p : w.Ks.p;
    const long Kc = (long)Np + Fp;
    if (!g.gram_direct && !w.b2_ready) {
        w.B2.ensure((size_t)Kc * g.Dcols);
        SLS_HIP(hipMemcpy2DAsync(w.B2.p, Kc * 8, g.XT, (size_t)Np * 8, (size_t)Np * 8, g.Dcols, hipMemcpyDeviceToDevice, c->stream));
        SLS_HIP(hipMemcpy2DAsync(w.B2.p + Np, Kc * 8, p->Om.p, (size_t)Fp * 8, (size_t)Fp * 8, g.Dcols, hipMemcpyDeviceToDevice, c->stream));
        w.b2_ready = true;
    }
    for (int s0 = 0; s0 < M; s0 += pass_max) {
        const int sc = std::min(pass_max, M - s0), Sp = round_up(sc, 128), Pp = q * Sp;
        double* Pm = w.PG.p;
        double* G = w.PG.p + (size_t)Pp * Np;
        draw_values_device(p, g, w, Pp, [&] {
            for (int i = 0; i < q; ++i)
                launch_prep_cands(c->stream, xr + (size_t)i * D * ldr + s0, ldr, D, sc, g.inv_ell, w.XsT.p + (size_t)i * Sp, Pp, Sp, g.Dcols,
                                  w.ns.p + (size_t)i * Sp);
        }, [&](KernelSpec ks, double* Cs) {
            for (int i = 0; i < q; ++i)
                launch_cross_gram_direct(c->stream, xr + (size_t)i * D * ldr + s0, 1, ldr, sc, Sp, g.X, D, g.inv_ell, g.Np, g.N, ks, nullptr,
                                         w.Ks.p + (size_t)i * Sp, Cs + (size_t)i * Sp, Pp, nullptr, nullptr);
        });
        {
            ProfScope ps(c, scope);
            if (mode.log_form)
                launch_qlognei_select(c->stream, sc, Sp, q, S, Rp, w.VM.p, Pp, base, mode.tau_relu, mode.tau_max, w.lmq.p, w.lzq.p, w.lpmx.p,
                                      w.lpsm.p, w.lpbad, w.lpwin, w.sum.p, wins ? wins + s0 : nullptr, ldw, w.bad);
            else
                launch_qeubo_select(c->stream, sc, Sp, q, S, Rp, w.VM.p, Pp, base, w.sum.p, wins ? wins + s0 : nullptr, ldw, w.bad);
        }
        {
            // aggregated weights of every point: the sums of the columns of W / V over the draws its option wins
            ProfScope ps(c, "qeubo_agg");
            launch_gemm_plain(c->stream, p->W.p, 2L * Fp, false, w.VM.p, Pp, false, w.Wbar.p, 2L * Fp, 2 * Fp / 128, Pp / 128, Rp, 1.0, 0.0);
            launch_gemm_plain(c->stream, p->V.p, Np, false, w.VM.p, Pp, false, w.Vbar.p, Np, Np / 128, Pp / 128, Rp, 1.0, 0.0);
        }
        {
            // the gathered route of a path evaluation with point j under "draw" j of (Wbar, Vbar)
            ProfScope ps(c, "path_prior");
            launch_path_feat(c->stream, w.XsT.p, Pp, g.Dp, Pp, p->Om.p, Fp, w.Wbar.p, 2L * Fp, w.ident, Pp, G, Pp, w.vpart.p, Pp);
            // fbar = fbar_i(x_i) is scratch with no consumer: the reused kernels accumulate a value beside the gradient weights, and
            // path_data adds onto it, so it starts from path_feat's chunk sums rather than from whatever the block held
            launch_path_vsum(c->stream, w.vpart.p, Pp, Fp / 128, Pp, w.fbar.p);
        }
        {
            ProfScope ps(c, "path_data");
            launch_path_data(c->stream, w.Ks.p, Cs, Pp, g.N, Np, w.Vbar.p, Np, w.ident, 0, 0, Pp, w.fbar.p, Pm, w.csum.p);
        }
        {
            ProfScope ps(c, "path_grad_gemm");
            double* part = nullptr;
            if (D <= 64 && grad_gemm_wants_split(Pp)) {
                w.Gpart.ensure((size_t)8 * Pp * 64);
                part = w.Gpart.p;
            }
            if (g.gram_direct) {   // as in path_eval_device: G Om alone, the data term over raw coordinate differences per option
                launch_grad_gemm(c->stream, G, nullptr, Pp, Pp, p->Om.p, nullptr, Fp, Fp, D <= 64 ? -g.Dcols : g.Dcols, w.Gt.p, nullptr, part, 1);
                for (int i = 0; i < q; ++i)
                    launch_grad_direct(c->stream, Pm + (size_t)i * Sp, nullptr, Pp, Sp, xr + (size_t)i * D * ldr + s0, 1, ldr, sc, g.X, D,
                                       g.inv_ell, g.N, nullptr, w.Gd.p + (size_t)i * Sp, nullptr);
            } else {
                launch_grad_gemm(c->stream, Pm, nullptr, Pp, Pp, w.B2.p, nullptr, Kc, (int)Kc, D <= 64 ? -g.Dcols : g.Dcols, w.Gt.p, nullptr,
                                 part, 1);
            }
        }
        {
            ProfScope ps(c, "path_data");
            if (g.gram_direct) launch_path_grad_direct(c->stream, Pp, D, Pp, w.Gt.p, w.Gd.p, g.inv_ell, w.gpt.p, Pp);
            else launch_path_grad(c->stream, Pp, D, Pp, w.Gt.p, w.XsT.p, w.csum.p, g.inv_ell, w.gpt.p, Pp);
        }
        {
            ProfScope ps(c, scope);
            launch_qeubo_finish(c->stream, sc, Sp, q, D, S, w.sum.p, w.bad, w.gpt.p, Pp, floor, val ? val + s0 : nullptr,
                                grad ? grad + s0 : nullptr, ldo, mode.log_form);
        }
    }
}

}  // namespace

// taus = (tau_relu, tau_max) of the log form, checked once per call before anything is uploaded
static void require_temperatures(const char* who, const double* taus) {
    SLS_REQUIRE(std::isfinite(taus[0]) && taus[0] > 0.0, "%s: tau_relu = %g (finite, > 0)", who, taus[0]);
    SLS_REQUIRE(std::isfinite(taus[1]) && taus[1] > 0.0, "%s: tau_max = %g (finite, > 0)", who, taus[1]);
}
static SetMode set_mode(const double* device_base, const double* taus) {
    SetMode m;
    m.base = device_base;
    if (taus) {
        m.log_form = true;
        m.tau_relu = taus[0];
        m.tau_max = taus[1];
    }
    return m;
}

static void require_finite_baseline(const char* who, const sls_path* p, const double* baseline) {
    SLS_REQUIRE(baseline != nullptr, "%s: baseline is NULL", who);
    for (int s = 0; s < p->n_draws; ++s) SLS_REQUIRE(std::isfinite(baseline[s]), "%s: baseline[%d] is not finite", who, s);
}

// sls_qeubo_eval / sls_qnei_eval (want_base: competes against the per-draw baseline)
static int set_eval(const char* who, sls_path* p, int q, const double* baseline, bool want_base, const double* sets, int M, double* val,
                    double* grad, int* wins, const double* taus = nullptr) {
    SLS_TRY
    SLS_REQUIRE(p != nullptr, "%s: p is NULL", who);
    SLS_REQUIRE(q >= 1 && q <= SLS_QEUBO_MAX_OPTIONS, "%s: q = %d (1 .. %d)", who, q, SLS_QEUBO_MAX_OPTIONS);
    SLS_REQUIRE(M >= 0, "%s: M = %d", who, M);
    SLS_REQUIRE(sets != nullptr, "%s: sets is NULL", who);
    if (taus) require_temperatures(who, taus);
    if (want_base) require_finite_baseline(who, p, baseline);
    GpReadCall call(p->gp, p->generation, who);
    if (M == 0) return SLS_OK;
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int qD = q * g.D, Mp = round_up(M, 128);
    const std::vector<double> t = host_to_cm(sets, qD, M, Mp);   // alive until the synchronisation below
    DBuf raw, out, wb, tb;
    raw.ensure(t.size());
    h2d(c, raw.p, t.data(), t.size());
    if (want_base) {
        tb.ensure((size_t)p->n_draws);
        h2d(c, tb.p, baseline, (size_t)p->n_draws);
    }
    out.ensure((size_t)Mp * (1 + qD));
    int* d_wins = wins ? ints(wb, (size_t)Mp * q) : nullptr;
    QeuboWs ws;
    qeubo_eval_device(p, g, ws, q, set_mode(tb.p, taus), raw.p, Mp, M, out.p, grad ? out.p + Mp : nullptr, Mp, d_wins, Mp);
    std::vector<double> oh((size_t)Mp * (grad ? 1 + qD : 1));
    std::vector<int> wh(wins ? (size_t)Mp * q : 0);
    d2h(c, oh.data(), out.p, oh.size());
    if (wins) SLS_HIP(hipMemcpyAsync(wh.data(), d_wins, wh.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    cm_to_host(oh.data(), Mp, 1, M, val);
    cm_to_host(oh.data() + Mp, Mp, qD, M, grad);
    cm_to_host(wh.data(), Mp, q, M, wins);
    SLS_CATCH
}

extern "C" int sls_qeubo_eval(sls_path* p, int q, const double* sets, int M, double* val, double* grad, int* wins) {
    return set_eval("sls_qeubo_eval", p, q, nullptr, false, sets, M, val, grad, wins);
}

// sls_qeubo_maximize / sls_qnei_maximize
static int set_maximize(const char* who, sls_path* p, int q, const double* baseline, bool want_base, const double* starts, int S_starts,
                        int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                        double* x_stars, double* y_stars, const double* taus = nullptr) {
    SLS_TRY
    SLS_REQUIRE(p && starts, "%s: NULL argument", who);
    SLS_REQUIRE(q >= 1 && q <= SLS_QEUBO_MAX_OPTIONS, "%s: q = %d (1 .. %d)", who, q, SLS_QEUBO_MAX_OPTIONS);
    if (taus) require_temperatures(who, taus);
    if (want_base) require_finite_baseline(who, p, baseline);
    GpReadCall call(p->gp, p->generation, who);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    // the maximiser of sls_acq_maximize over [0,1]^(qD): one start = one set of q options.  Workspaces are per call; the best start
    // and every fetch come back through pageable memory.
    const int S = S_starts, qD = q * g.D;
    LbfgsWs lb;
    QeuboWs ws;
    MultistartRun r = maximize_begin(who, p->gp, lb, opts, S, n_local, qD);
    DBuf sd, best, tb;
    sd.ensure((size_t)qD * S);
    best.ensure((size_t)8 + qD);
    h2d(c, sd.p, starts, (size_t)qD * S);
    if (want_base) {   // once, before the first round
        tb.ensure((size_t)p->n_draws);
        h2d(c, tb.p, baseline, (size_t)p->n_draws);
    }
    const SetMode mode = set_mode(tb.p, taus);
    LockstepStats ls;
    lockstep_rounds(c, r.st, lb, sd.p, S, n_local,
                    [&](const double* trial, long ld, int nlive, const int*, double* val, double* grad) {
                        qeubo_eval_device(p, g, ws, q, mode, trial, ld, nlive, val, grad, ld, nullptr, 0);
                    },
                    &ls);
    std::vector<double> bh((size_t)8 + qD), pageable;
    auto fetch = [&](const double* dev, size_t n) {
        pageable.resize(n);
        d2h(c, pageable.data(), dev, n);
        SLS_HIP(hipStreamSynchronize(c->stream));
        return pageable.data();
    };
    maximize_finish(c, r, ls, BestBlock{best.p, bh.data(), true}, fetch, start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}

extern "C" int sls_qeubo_maximize(sls_path* p, int q, const double* starts, int S_starts, int n_local, const sls_lbfgs_opts* opts,
                                  long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars,
                                  double* y_stars) {
    return set_maximize("sls_qeubo_maximize", p, q, nullptr, false, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out,
                        idx_out, x_stars, y_stars);
}

// ---- noisy expected improvement on the draws (include/sls_hip.h) ---------------------------------------------------------------
extern "C" int sls_path_max_over_points(sls_path* p, const double* Xb, int Mb, double* t_out, int* arg_out) {
    SLS_TRY
    SLS_REQUIRE(p && Xb, "sls_path_max_over_points: NULL argument");
    SLS_REQUIRE(Mb >= 1, "sls_path_max_over_points: Mb = %d", Mb);
    GpReadCall call(p->gp, p->generation, "sls_path_max_over_points");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws;
    // passes of points bounded as a qEUBO pass of one-option sets bounds them; the running (max, argmax) per draw merges across passes
    const int pass_max = std::min(round_up(Mb, 128), qeubo_sets_per_pass(c, 1, g.Np, p->Fp, p->Rp));
    QeuboWs ws;
    ws.ensure(c, p, g, pass_max, pass_max, true);
    DBuf raw, tb, ab;
    raw.ensure((size_t)D * Mb);
    h2d(c, raw.p, Xb, (size_t)D * Mb);
    tb.ensure((size_t)nd);
    int* d_arg = ints(ab, (size_t)nd);
    for (int p0 = 0; p0 < Mb; p0 += pass_max) {
        const int pc = std::min(pass_max, Mb - p0), Pp = round_up(pc, 128);
        draw_values_device(p, g, ws, Pp, [&] {
            launch_prep_points(c->stream, raw.p + (size_t)p0 * D, D, pc, g.inv_ell, ws.XsT.p, Pp, Pp, g.Dcols, ws.ns.p);
        }, [&](KernelSpec ks, double* Cs) {
            launch_cross_gram_direct(c->stream, raw.p + (size_t)p0 * D, D, 1, pc, Pp, g.X, D, g.inv_ell, g.Np, g.N, ks, nullptr, ws.Ks.p, Cs,
                                     Pp, nullptr, nullptr);
        });
        ProfScope ps(c, "path_max");
        launch_path_colmax(c->stream, ws.VM.p, Pp, pc, nd, p0, tb.p, d_arg);   // the pc live rows only
    }
    if (t_out) d2h(c, t_out, tb.p, (size_t)nd);
    if (arg_out) SLS_HIP(hipMemcpyAsync(arg_out, d_arg, (size_t)nd * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    SLS_CATCH
}

extern "C" int sls_qnei_eval(sls_path* p, int q, const double* baseline, const double* sets, int M, double* val, double* grad, int* wins) {
    return set_eval("sls_qnei_eval", p, q, baseline, true, sets, M, val, grad, wins);
}

extern "C" int sls_qnei_maximize(sls_path* p, int q, const double* baseline, const double* starts, int S_starts, int n_local,
                                 const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                                 double* x_stars, double* y_stars) {
    return set_maximize("sls_qnei_maximize", p, q, baseline, true, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out,
                        idx_out, x_stars, y_stars);
}

// ---- log-space noisy expected improvement on the draws (include/sls_hip.h) --------------------------------------------------
extern "C" int sls_qlognei_eval(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* sets, int M,
                                double* val, double* grad, int* wins) {
    const double taus[2] = {tau_relu, tau_max};
    return set_eval("sls_qlognei_eval", p, q, baseline, true, sets, M, val, grad, wins, taus);
}

extern "C" int sls_qlognei_maximize(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* starts,
                                    int S_starts, int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out,
                                    double* val_out, long* idx_out, double* x_stars, double* y_stars) {
    const double taus[2] = {tau_relu, tau_max};
    return set_maximize("sls_qlognei_maximize", p, q, baseline, true, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out,
                        idx_out, x_stars, y_stars, taus);
}

// ---- expected utility of the best slider position on the draws (include/sls_hip.h) ------------------------------------------
namespace {

struct LineWs {
    QeuboWs q;
    DBuf sets, sgrad;   // the expanded sets and their gradient of ONE pass (qD x pass), never of the whole call
};

// Line EUBO (qNEI form with base) at M lines, candidate-major lines[n + r*ld] (2D rows, or D rows with the device D-vector anchor).
// val[n], grad[n + r*ldo] (2D / D rows), wins[n + i*ldw]; each may be nullptr.  Per pass of the qEUBO sizing: expand, ONE pass of
// qeubo_eval_device, fold.  A pass's bits do not depend on the split, so driving the chunks here only bounds the two workspaces.
void line_eval_device(sls_path* p, const GpView& g, LineWs& w, int q, const double* base, const double* anchor, const double* lines,
                      long ld, int M, double* val, double* grad, long ldo, int* wins, long ldw) {
    sls_ctx* c = g.ctx;
    const int D = g.D;
    const int pass_max = std::min(round_up(M, 128), qeubo_sets_per_pass(c, q, g.Np, p->Fp, p->Rp));
    w.sets.ensure((size_t)q * D * pass_max);
    if (grad) w.sgrad.ensure((size_t)q * D * pass_max);
    for (int s0 = 0; s0 < M; s0 += pass_max) {
        const int sc = std::min(pass_max, M - s0);
        {
            ProfScope ps(c, "line");
            launch_line_expand(c->stream, sc, D, q, lines + s0, ld, anchor, w.sets.p, pass_max);
        }
        qeubo_eval_device(p, g, w.q, q, set_mode(base, nullptr), w.sets.p, pass_max, sc, val ? val + s0 : nullptr,
                          grad ? w.sgrad.p : nullptr, pass_max, wins ? wins + s0 : nullptr, ldw);
        if (grad) {
            ProfScope ps(c, "line");
            launch_line_fold(c->stream, sc, D, q, anchor != nullptr, w.sgrad.p, pass_max, grad + s0, ldo);
        }
    }
}

void require_line_args(const char* who, const sls_path* p, int q, const double* baseline, const double* anchor) {
    SLS_REQUIRE(p != nullptr, "%s: p is NULL", who);
    SLS_REQUIRE(q >= SLS_LINE_MIN_POSITIONS && q <= SLS_QEUBO_MAX_OPTIONS, "%s: q = %d (%d .. %d)", who, q, SLS_LINE_MIN_POSITIONS,
                SLS_QEUBO_MAX_OPTIONS);
    if (baseline) require_finite_baseline(who, p, baseline);
    if (anchor)
        for (int d = 0; d < p->D; ++d) SLS_REQUIRE(std::isfinite(anchor[d]), "%s: anchor[%d] is not finite", who, d);
}

}  // namespace

extern "C" int sls_line_eval(sls_path* p, int q, const double* baseline, const double* anchor, const double* lines, int M, double* val,
                             double* grad, int* wins) {
    SLS_TRY
    const char* who = "sls_line_eval";
    require_line_args(who, p, q, baseline, anchor);
    SLS_REQUIRE(M >= 0, "%s: M = %d", who, M);
    SLS_REQUIRE(lines != nullptr, "%s: lines is NULL", who);
    GpReadCall call(p->gp, p->generation, who);
    if (M == 0) return SLS_OK;
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nvar = anchor ? D : 2 * D, Mp = round_up(M, 128);
    const std::vector<double> t = host_to_cm(lines, nvar, M, Mp);   // alive until the synchronisation below
    DBuf raw, out, wb, tb, ab;
    raw.ensure(t.size());
    h2d(c, raw.p, t.data(), t.size());
    if (baseline) {
        tb.ensure((size_t)p->n_draws);
        h2d(c, tb.p, baseline, (size_t)p->n_draws);
    }
    if (anchor) {
        ab.ensure((size_t)D);
        h2d(c, ab.p, anchor, (size_t)D);
    }
    out.ensure((size_t)Mp * (1 + nvar));
    int* d_wins = wins ? ints(wb, (size_t)Mp * q) : nullptr;
    LineWs ws;
    line_eval_device(p, g, ws, q, tb.p, ab.p, raw.p, Mp, M, out.p, grad ? out.p + Mp : nullptr, Mp, d_wins, Mp);
    std::vector<double> oh((size_t)Mp * (grad ? 1 + nvar : 1));
    std::vector<int> wh(wins ? (size_t)Mp * q : 0);
    d2h(c, oh.data(), out.p, oh.size());
    if (wins) SLS_HIP(hipMemcpyAsync(wh.data(), d_wins, wh.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    cm_to_host(oh.data(), Mp, 1, M, val);
    cm_to_host(oh.data() + Mp, Mp, nvar, M, grad);
    cm_to_host(wh.data(), Mp, q, M, wins);
    SLS_CATCH
}

extern "C" int sls_line_maximize(sls_path* p, int q, const double* baseline, const double* anchor, const double* starts, int S_starts,
                                 int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                                 long* idx_out, double* x_stars, double* y_stars) {
    SLS_TRY
    const char* who = "sls_line_maximize";
    SLS_REQUIRE(p && starts, "%s: NULL argument", who);
    require_line_args(who, p, q, baseline, anchor);
    GpReadCall call(p->gp, p->generation, who);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    // the maximiser of sls_qeubo_maximize over the ENDS: one start = one line, 2D variables (D with the anchor) whatever q is
    const int S = S_starts, D = g.D, nvar = anchor ? D : 2 * D;
    LbfgsWs lb;
    LineWs ws;
    MultistartRun r = maximize_begin(who, p->gp, lb, opts, S, n_local, nvar);
    DBuf sd, best, tb, ab;
    sd.ensure((size_t)nvar * S);
    best.ensure((size_t)8 + nvar);
    h2d(c, sd.p, starts, (size_t)nvar * S);
    if (baseline) {   // both once, before the first round
        tb.ensure((size_t)p->n_draws);
        h2d(c, tb.p, baseline, (size_t)p->n_draws);
    }
    if (anchor) {
        ab.ensure((size_t)D);
        h2d(c, ab.p, anchor, (size_t)D);
    }
    LockstepStats ls;
    lockstep_rounds(c, r.st, lb, sd.p, S, n_local,
                    [&](const double* trial, long ld, int nlive, const int*, double* val, double* grad) {
                        line_eval_device(p, g, ws, q, tb.p, ab.p, trial, ld, nlive, val, grad, ld, nullptr, 0);
                    },
                    &ls);
    std::vector<double> bh((size_t)8 + nvar), pageable;
    auto fetch = [&](const double* dev, size_t n) {
        pageable.resize(n);
        d2h(c, pageable.data(), dev, n);
        SLS_HIP(hipStreamSynchronize(c->stream));
        return pageable.data();
    };
    maximize_finish(c, r, ls, BestBlock{best.p, bh.data(), true}, fetch, start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}
