// C-ABI of the pathwise posterior function draws (include/sls_hip.h: sls_path_*, and sls_qeubo_* / sls_qnei_* / sls_qlognei_* / sls_qbald_* /
// sls_line_* / sls_patch_* on them): host orchestration of kernels_path.hip and kernels_qeubo.hip, the cross Gram / gradient products of
// kernels_gram.hip / kernels_acq.hip, the tile GEMM and block solve of kernels_tri.hip and the lock-step L-BFGS rounds of
// lbfgs_driver.hpp.  No CPU fallback.
// Every route is put together from the same pieces:
//   PassWs / SetWs          the device blocks of a pass of points, and what a pass of sets adds to them
//   PassPoints              where the raw coordinates of a pass live (point-major, candidate-major, q option segments)
//   pass_cross_gram         scaled coordinates and K*, C* of a pass, tiled or from the raw differences (gram_direct)
//   every_draw_prefix       pass_cross_gram, the features and Phi^T W: every draw at every point, before the caller's data term
//   gathered_route          one weight column per point: value, data term and gradient (tiled, or direct beyond the guard)
//   path_eval_gathered      host body of sls_path_eval (gathered form) and sls_path_eval_sub
//   path_maximize           host body of sls_path_maximize and sls_path_maximize_sub
//   set_eval / set_maximize host bodies of sls_qeubo_*, sls_qnei_*, sls_qlognei_*, sls_qbald_*, sls_line_* and sls_patch_* (SetCall tells them apart)
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

// Device blocks of a pass of points (one call).  Pm and G share one block: G = Pm + Pp Np (same leading dimension), so that [Pm | G]
// is ONE operand of the gradient contraction against B2 = [X~ ; Om] (k-stacked, built once per call).  Gd: the data term's gradient
// contraction over raw coordinate differences, for handles beyond the guard of the norm expansion.
struct PassWs {
    DBuf XsT, ns, Ks, Cs, PG, csum, vpart, Gt, B2, Gpart, Gd;
    bool b2_ready = false;
    // Pp points; values_only: the blocks of the every-draw values alone (sls_path_max_over_points)
    void ensure(const sls_path* p, const GpView& g, int Pp, bool values_only = false) {
        const size_t P = Pp, Np = g.Np, Fp = p->Fp;
        XsT.ensure(P * g.Dcols);
        ns.ensure(P);
        Ks.ensure(P * Np);
        if (g.kernel == SLS_KERNEL_ARD_MATERN52) Cs.ensure(P * Np);
        PG.ensure(P * (Np + 2 * Fp));
        if (values_only) return;
        csum.ensure(P);
        vpart.ensure(P * (Fp / 128));
        Gt.ensure(P * g.Dcols);
        if (g.gram_direct) Gd.ensure(P * g.Dcols);
    }
    // B2 = [X~ ; Om], Np + Fp deep: for the gradient of a handle inside the guard
    void ensure_b2(const sls_path* p, const GpView& g) {
        if (b2_ready) return;
        const long Np = g.Np, Fp = p->Fp, Kc = Np + Fp;
        hipStream_t s = g.ctx->stream;
        B2.ensure((size_t)Kc * g.Dcols);
        SLS_HIP(hipMemcpy2DAsync(B2.p, Kc * 8, g.XT, (size_t)Np * 8, (size_t)Np * 8, g.Dcols, hipMemcpyDeviceToDevice, s));
        SLS_HIP(hipMemcpy2DAsync(B2.p + Np, Kc * 8, p->Om.p, (size_t)Fp * 8, (size_t)Fp * 8, g.Dcols, hipMemcpyDeviceToDevice, s));
        b2_ready = true;
    }
    double* cstar(const GpView& g) { return g.kernel == SLS_KERNEL_ARD_MATERN52 ? Cs.p : Ks.p; }   // C* (the SE kernel's is K*)
};

// Where the raw coordinates of a pass's points live: nseg segments of `rows` padded rows each (the pass's points are segment-major,
// nseg * rows in all), the first `live` of every segment real, coordinate d of point n of segment i at x[(i D + d) sd + n sn].  This is
// the point-major block (sn = D, sd = 1, one segment), the candidate-major block (sn = 1, sd = its leading dimension, one segment)
// and the candidate-major set block (segment i = option i of every set).  Candidate-major blocks are padded to 128 columns, so
// sd == 1 says point-major.
struct PassPoints {
    const double* x;
    long sn, sd;
    int nseg, rows, live;
    int padded() const { return nseg * rows; }
    const double* seg(int i, int D) const { return x + (size_t)i * D * sd; }
};

// Scaled coordinates, norms and K* / C* of a pass: cross_gram on the tiles, or, for handles beyond the guard of the norm expansion
// (kernels.hpp), the data term from the raw coordinate differences.
void pass_cross_gram(const GpView& g, PassWs& w, const PassPoints& pt) {
    sls_ctx* c = g.ctx;
    const int D = g.D, Pp = pt.padded();
    KernelSpec ks{g.kernel, g.a};
    ProfScope ps(c, "cross_gram");
    for (int i = 0; i < pt.nseg; ++i) {
        const size_t o = (size_t)i * pt.rows;
        if (pt.sd == 1) launch_prep_points(c->stream, pt.seg(i, D), D, pt.live, g.inv_ell, w.XsT.p + o, Pp, pt.rows, g.Dcols, w.ns.p + o);
        else launch_prep_cands(c->stream, pt.seg(i, D), pt.sd, D, pt.live, g.inv_ell, w.XsT.p + o, Pp, pt.rows, g.Dcols, w.ns.p + o);
    }
    if (!g.gram_direct)
        launch_cross_gram(c->stream, w.XsT.p, Pp, w.ns.p, Pp, g.XT, g.Np, g.nx, g.Np, g.N, g.Dp, ks, nullptr, w.Ks.p, w.cstar(g), Pp, nullptr,
                          nullptr);
    else
        for (int i = 0; i < pt.nseg; ++i)
            launch_cross_gram_direct(c->stream, pt.seg(i, D), pt.sn, pt.sd, pt.live, pt.rows, g.X, D, g.inv_ell, g.Np, g.N, ks, nullptr,
                                     w.Ks.p + (size_t)i * pt.rows, w.cstar(g) + (size_t)i * pt.rows, Pp, nullptr, nullptr);
}

// The prior part of every draw at every point of a pass: pass_cross_gram, the features Phi (nfeat rows of them) into G's 2Fp
// columns, dst[n + s*ldd] = (Phi^T W)[n, s] on the tile GEMM.  The data term is the caller's: the two every-draw routes add it in
// different ways (path_data / an accumulating tile GEMM) and so differ in their bits.
void every_draw_prefix(sls_path* p, const GpView& g, PassWs& w, const PassPoints& pt, int nfeat, double* dst, long ldd) {
    sls_ctx* c = g.ctx;
    const int Fp = p->Fp, Pp = pt.padded();
    double* G = w.PG.p + (size_t)Pp * g.Np;
    pass_cross_gram(g, w, pt);
    ProfScope ps(c, "path_prior");
    launch_path_feat(c->stream, w.XsT.p, Pp, g.Dp, Pp, p->Om.p, Fp, p->W.p, 2L * Fp, nullptr, nfeat, G, Pp, nullptr, 0);
    launch_gemm_plain(c->stream, G, Pp, false, p->W.p, 2L * Fp, true, dst, ldd, Pp / 128, p->Rp / 128, 2 * Fp, 1.0, 0.0);
}

// The gathered route on a pass whose K* / C* stand (pass_cross_gram): point n < count under column draw[n] of the weight blocks W
// (2Fp rows) and V (Np rows).  val[n] = the chunk sums of the random-feature contraction on the matrix cores (path_feat) plus the data
// term (path_data); with want_grad, grad[n + d*ldgrad] = G Om^T + Pm X~^T on the tile GEMM (path_grad), or beyond the guard G Om^T
// and the data term over the raw coordinate differences of pt (path_grad_direct).
void gathered_route(sls_path* p, const GpView& g, PassWs& w, const PassPoints& pt, const double* W, long ldw, const double* V, long ldv,
                    const int* draw, int count, bool want_grad, double* val, double* grad, long ldgrad) {
    sls_ctx* c = g.ctx;
    const int D = g.D, Np = g.Np, Fp = p->Fp, Pp = pt.padded();
    double* Pm = w.PG.p;
    double* G = w.PG.p + (size_t)Pp * Np;
    {
        ProfScope ps(c, "path_prior");
        launch_path_feat(c->stream, w.XsT.p, Pp, g.Dp, Pp, p->Om.p, Fp, W, ldw, draw, count, G, Pp, w.vpart.p, Pp);
        launch_path_vsum(c->stream, w.vpart.p, Pp, Fp / 128, count, val);
    }
    {
        ProfScope ps(c, "path_data");
        launch_path_data(c->stream, w.Ks.p, w.cstar(g), Pp, g.N, Np, V, ldv, draw, 0, 0, count, val, want_grad ? Pm : nullptr, w.csum.p);
    }
    if (!want_grad) return;
    {
        ProfScope ps(c, "path_grad_gemm");
        double* part = grad_split_scratch(w.Gpart, D, Pp);
        const int dcols = D <= 64 ? -g.Dcols : g.Dcols;
        if (g.gram_direct) {
            // Beyond the guard: Gt = G Om alone (Fp deep) and the data term over raw coordinate differences (grad_direct).  In the one
            // contraction below the accumulator carries x~* sum_i c_i (|x~| ~ 1 / (2 l)) through the Fp additions of the prior and
            // loses it again only in path_grad: eps |x~| |csum| sqrt(Fp) / l, 20 times the rounding of the terms themselves at
            // F = 16384, l = 3e-3.
            launch_grad_gemm(c->stream, G, nullptr, Pp, Pp, p->Om.p, nullptr, Fp, Fp, dcols, w.Gt.p, nullptr, part, 1);
            for (int i = 0; i < pt.nseg; ++i)
                launch_grad_direct(c->stream, Pm + (size_t)i * pt.rows, nullptr, Pp, pt.rows, pt.seg(i, D), pt.sn, pt.sd, pt.live, g.X, D,
                                   g.inv_ell, g.N, nullptr, w.Gd.p + (size_t)i * pt.rows, nullptr);
        } else {
            // Gt = [Pm | G] [X~ ; Om]: X~^T c of the data term plus the prior's gradient in scaled coordinates, ONE MFMA contraction
            // (Np + Fp deep) on grad_gemm's P-pass alone (fixed quarter order: a candidate's bits do not depend on the launch)
            const long Kc = (long)Np + Fp;
            launch_grad_gemm(c->stream, Pm, nullptr, Pp, Pp, w.B2.p, nullptr, Kc, (int)Kc, dcols, w.Gt.p, nullptr, part, 1);
        }
    }
    ProfScope ps(c, "path_data");
    if (g.gram_direct) launch_path_grad_direct(c->stream, count, D, Pp, w.Gt.p, w.Gd.p, g.inv_ell, grad, ldgrad);
    else launch_path_grad(c->stream, count, D, Pp, w.Gt.p, w.XsT.p, w.csum.p, g.inv_ell, grad, ldgrad);
}

// S candidates at raw coordinates xr: candidate-major xr[n + d*ldr], or point-major xr[d + n*D], in chunks of chunk_of.
//   draw != nullptr (device, S ints): val[n] = f_{draw[n]}(x_n), grad[n + d*ldgrad] (may be nullptr): the gathered route;
//   draw == nullptr: val[n + s*ldall] = f_s(x_n) for every draw s (val has Rp columns), no gradient: the every-draw prefix, then the
//   data term (path_data).
void path_eval_device(sls_path* p, const GpView& g, PassWs& w, const double* xr, long ldr, bool point_major, int S, const int* draw,
                      double* val, long ldall, double* grad, long ldgrad) {
    sls_ctx* c = g.ctx;
    const int D = g.D, Np = g.Np, Fp = p->Fp;
    const int chunk_max = std::min(round_up(S, 128), chunk_of(Np, Fp));
    w.ensure(p, g, chunk_max);
    if (grad && !g.gram_direct) w.ensure_b2(p, g);
    for (int s0 = 0; s0 < S; s0 += chunk_max) {
        const int sc = std::min(chunk_max, S - s0), Cp = round_up(sc, 128);
        const PassPoints pt = point_major ? PassPoints{xr + (size_t)s0 * D, D, 1, 1, Cp, sc} : PassPoints{xr + s0, 1, ldr, 1, Cp, sc};
        if (!draw) {
            every_draw_prefix(p, g, w, pt, sc, val + s0, ldall);
            ProfScope ps(c, "path_data");
            launch_path_data(c->stream, w.Ks.p, w.cstar(g), Cp, g.N, Np, p->V.p, Np, nullptr, sc, ldall, sc * p->n_draws, val + s0, nullptr,
                             nullptr);
            continue;
        }
        pass_cross_gram(g, w, pt);
        gathered_route(p, g, w, pt, p->W.p, 2L * Fp, p->V.p, Np, draw + s0, sc, grad != nullptr, val + s0, grad ? grad + s0 : nullptr, ldgrad);
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
    // a Laplace handle (sls_gp_set_laplace): every draw takes N more numbers, z, after eps -- the sampled goodness vector
    const int Ndraw = g.laplace ? 2 * N : N;
    const long nE = (long)n_draws * (2L * F + Ndraw);
    DBuf Z, E, Phi, Lc, Zm, Xm, Q;   // alive until the synchronisation at the end
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
        launch_path_weights(c->stream, E.p, F, Fp, Ndraw, n_draws, Rp, std::sqrt(g.a / F), p->W.p);
        // f_prior,s(x_i) for every draw into V's block (Phi_X^T W, row blocks of the training points), then r = y - sqrt(b) eps - f_prior
        const int rows = std::max(128, std::min(Np, ((1 << 26) / (2 * Fp)) / 128 * 128));
        Phi.ensure((size_t)rows * 2 * Fp);
        for (int i0 = 0; i0 < Np; i0 += rows) {
            const int rc = std::min(rows, Np - i0);
            launch_path_feat(c->stream, g.XT + i0, Np, g.Dp, rc, p->Om.p, Fp, p->W.p, 2L * Fp, nullptr, rc, Phi.p, rc, nullptr, 0);
            launch_gemm_plain(c->stream, Phi.p, rc, false, p->W.p, 2L * Fp, true, p->V.p + i0, Np, rc / 128, Rp / 128, 2 * Fp, 1.0, 0.0);
        }
        if (g.laplace) {
            // Q = L (L_B^-T Z): one product with the explicit L_B^-1 for all draws at once, then one with a copy of L whose upper
            // triangle is cleared (the factor's own buffer keeps K_y's entries there)
            const size_t n2 = (size_t)Np * Np, nr = (size_t)Np * Rp;
            Lc.ensure(n2); Zm.ensure(nr); Xm.ensure(nr); Q.ensure(nr);
            SLS_HIP(hipMemcpyAsync(Lc.p, g.L, n2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            launch_zero_upper(c->stream, Lc.p, Np);
            launch_path_laplace_z(c->stream, E.p, F, N, Np, n_draws, Rp, Zm.p);
            launch_gemm_plain(c->stream, g.lap_LBinv, Np, true, Zm.p, Np, true, Xm.p, Np, Np / 128, Rp / 128, Np, 1.0, 0.0);
            launch_gemm_plain(c->stream, Lc.p, Np, false, Xm.p, Np, true, Q.p, Np, Np / 128, Rp / 128, Np, 1.0, 0.0);
        }
        launch_path_rhs(c->stream, g.y, E.p, F, N, Np, n_draws, Rp, std::sqrt(g.b), p->V.p, g.laplace ? Q.p : nullptr);
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

// ---- the draws over affine subspaces (include/sls_hip.h "maximisation over affine subspaces") ------------------------------------
namespace {

// The two blocks of a call: the expanded points x = c + A z and their gradient, D x ld doubles each, from the device pool
struct SubWs {
    DBuf x, gx;
};

}  // namespace

// The gathered evaluation behind sls_path_eval (pts = Xs, point-major as the caller holds them) and, with sub, sls_path_eval_sub (pts =
// Z, evaluated at x = c + A z): the draw indices checked and uploaded, one device call, values / gradient (in the variables: D rows, or
// d with sub) / expanded points (sub only) back through pageable memory.
static void path_eval_gathered(const char* who, sls_path* p, bool sub, const sls_submaps* maps, const double* pts, int M,
                               const int* draw_of_point, double* val, double* grad, double* X_out) {
    for (int m = 0; m < M; ++m)
        SLS_REQUIRE(draw_of_point[m] >= 0 && draw_of_point[m] < p->n_draws, "%s: draw_of_point[%d] = %d (n_draws = %d)", who, m,
                    draw_of_point[m], p->n_draws);
    GpReadCall call(p->gp, p->generation, who);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    SubMapsDev up;
    if (sub) upload_sub_maps(who, c, maps, g.D, M, up);
    const int D = g.D, rows = sub ? up.m.d : D, Mp = round_up(M, 128);
    const std::vector<double> zh = sub ? host_to_cm(pts, rows, M, Mp) : std::vector<double>();   // alive until the synchronisation
    const size_t n_in = sub ? zh.size() : (size_t)D * M;
    DBuf in, vout, gout, dbuf;
    in.ensure(n_in);
    h2d(c, in.p, sub ? zh.data() : pts, n_in);
    int* d_draw = ints(dbuf, (size_t)M);
    SLS_HIP(hipMemcpyAsync(d_draw, draw_of_point, (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
    vout.ensure(Mp);
    if (grad) gout.ensure((size_t)Mp * rows);
    PassWs ws;
    SubWs sw;
    if (sub)   // path_eval_device (gathered form) at x = c + A z, point m under d_draw[m]
        sub_eval(c, up.m, sw.x, sw.gx, in.p, Mp, M, nullptr, grad ? gout.p : nullptr,
                 [&](const double* x, double* gx) { path_eval_device(p, g, ws, x, Mp, false, M, d_draw, vout.p, 0, gx, Mp); });
    else path_eval_device(p, g, ws, in.p, 0, true, M, d_draw, vout.p, 0, grad ? gout.p : nullptr, Mp);
    d2h(c, val, vout.p, (size_t)M);
    std::vector<double> gh(grad ? (size_t)Mp * rows : 0), xh(X_out ? (size_t)Mp * D : 0);
    if (grad) d2h(c, gh.data(), gout.p, gh.size());
    if (X_out) d2h(c, xh.data(), sw.x.p, xh.size());
    SLS_HIP(hipStreamSynchronize(c->stream));
    cm_to_host(gh.data(), Mp, rows, M, grad);
    cm_to_host(xh.data(), Mp, D, M, X_out);
}

extern "C" int sls_path_eval(sls_path* p, const double* Xs, int M, const int* draw_of_point, double* val, double* grad) {
    SLS_TRY
    SLS_REQUIRE(p != nullptr, "sls_path_eval: p is NULL");
    SLS_REQUIRE(M >= 0, "sls_path_eval: M = %d", M);
    SLS_REQUIRE(draw_of_point || !grad, "sls_path_eval: grad must be NULL when draw_of_point is NULL (every-draw form)");
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Xs && val, "sls_path_eval: Xs / val is NULL");
    if (draw_of_point) {
        path_eval_gathered("sls_path_eval", p, false, nullptr, Xs, M, draw_of_point, val, grad, nullptr);
        return SLS_OK;
    }
    GpReadCall call(p->gp, p->generation, "sls_path_eval");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, Mp = round_up(M, 128);
    DBuf raw, vout;
    raw.ensure((size_t)D * M);
    h2d(c, raw.p, Xs, (size_t)D * M);
    vout.ensure((size_t)Mp * p->Rp);
    PassWs ws;
    path_eval_device(p, g, ws, raw.p, 0, true, M, nullptr, vout.p, Mp, nullptr, 0);
    SLS_HIP(hipMemcpy2DAsync(val, (size_t)M * 8, vout.p, (size_t)Mp * 8, (size_t)M * 8, p->n_draws, hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    SLS_CATCH
}

extern "C" int sls_path_eval_sub(sls_path* p, const sls_submaps* maps, const double* Z, int M, const int* draw_of_point, double* val,
                                 double* grad_z, double* X_out) {
    SLS_TRY
    SLS_REQUIRE(p != nullptr, "sls_path_eval_sub: p is NULL");
    SLS_REQUIRE(M >= 0, "sls_path_eval_sub: M = %d", M);
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(draw_of_point != nullptr, "sls_path_eval_sub: draw_of_point is NULL (the every-draw form has no _sub call)");
    SLS_REQUIRE(Z && val, "sls_path_eval_sub: Z / val is NULL");
    path_eval_gathered("sls_path_eval_sub", p, true, maps, Z, M, draw_of_point, val, grad_z, X_out);
    SLS_CATCH
}

// sls_path_maximize and, with sub, sls_path_maximize_sub (the same search in the d variables z, x = c + A z: expand and fold around
// the objective).  All T = n_draws S starts in one search through the shared prologue; the winner is per DRAW, so the epilogue is this
// body's own (and sls_acq_last_stats, which speaks of one winner's run, is left alone): the per-draw first maximum with the end
// variables, and with sub once more with their points (one more expand launch).  z_out: sub only.
static void path_maximize(const char* who, sls_path* p, bool sub, const sls_submaps* maps, const double* starts, int S, int n_local,
                          const sls_lbfgs_opts* opts, double* z_out, double* x_out, double* val_out, long* idx_out) {
    SLS_REQUIRE(p && starts, "%s: NULL argument", who);
    SLS_REQUIRE(S >= 1 && (long)S * p->n_draws <= (1L << 26), "%s: S = %d starts per draw (1 .. 2^26 / n_draws)", who, S);
    GpReadCall call(p->gp, p->generation, who);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws, T = S * nd, Sp = round_up(T, 128);
    SubMapsDev up;
    if (sub) upload_sub_maps(who, c, maps, D, T, up);
    const int d = sub ? up.m.d : D;
    LbfgsWs lb;
    PassWs ws;
    SubWs sw;
    MultistartRun r = maximize_begin(who, nullptr, lb, opts, T, n_local, d, Sp);
    const LbfgsState& st = r.st;
    int* d_draw = lb.tail();   // the draw of every live column
    DBuf sd;
    sd.ensure((size_t)d * T);
    h2d(c, sd.p, starts, (size_t)d * T);
    // f_{live[j] / S} is the objective of compacted column j
    lockstep_rounds(c, r.st, lb, sd.p, T, n_local,
                    [&](const double* trial, long ld, int nlive, const int* live, double* val, double* grad) {
                        launch_path_draw_of_live(c->stream, live, nlive, S, d_draw);
                        if (sub)
                            sub_eval(c, up.m, sw.x, sw.gx, trial, ld, nlive, live, grad, [&](const double* x, double* gx) {
                                path_eval_device(p, g, ws, x, ld, false, nlive, d_draw, val, 0, gx, ld);
                            });
                        else path_eval_device(p, g, ws, trial, ld, false, nlive, d_draw, val, 0, grad, ld);
                    },
                    nullptr);
    if (sub) {
        sw.x.ensure((size_t)D * Sp);
        sub_expand(c, up.m, T, nullptr, st.x, Sp, sw.x.p, Sp);
    }
    DBuf best;
    const size_t nz = (size_t)nd * (d + 2), nx = sub ? (size_t)nd * (D + 2) : 0;
    best.ensure(nz + nx);
    launch_path_argmax(c->stream, st.f, S, nd, st.x, Sp, d, best.p);
    if (sub) launch_path_argmax(c->stream, st.f, S, nd, sw.x.p, Sp, D, best.p + nz);
    std::vector<double> bh(nz + nx);
    d2h(c, bh.data(), best.p, bh.size());
    SLS_HIP(hipStreamSynchronize(c->stream));
    double* var_out = sub ? z_out : x_out;   // without maps the variables are the points
    for (int s = 0; s < nd; ++s) {
        const double* bz = bh.data() + (size_t)s * (d + 2);
        if (val_out) val_out[s] = bz[0];
        if (idx_out) idx_out[s] = (long)bz[1];
        if (var_out) std::copy(bz + 2, bz + 2 + d, var_out + (size_t)s * d);
        if (sub && x_out) {
            const double* bx = bh.data() + nz + (size_t)s * (D + 2);
            std::copy(bx + 2, bx + 2 + D, x_out + (size_t)s * D);
        }
    }
}

extern "C" int sls_path_maximize(sls_path* p, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts, double* x_out,
                                 double* val_out, long* idx_out) {
    SLS_TRY
    path_maximize("sls_path_maximize", p, false, nullptr, starts, S, n_local, opts, nullptr, x_out, val_out, idx_out);
    SLS_CATCH
}

extern "C" int sls_path_maximize_sub(sls_path* p, const sls_submaps* maps, const double* starts_z, int S, int n_local,
                                     const sls_lbfgs_opts* opts, double* z_out, double* x_out, double* val_out, long* idx_out) {
    SLS_TRY
    path_maximize("sls_path_maximize_sub", p, true, maps, starts_z, S, n_local, opts, z_out, x_out, val_out, idx_out);
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
// qLogNEI (log_form, with base and the two temperatures), or qBALD (bald: the BTL scale, no base; prob[n + i*ldp], device, receives
// the predicted choice probabilities of the call's columns, nullptr: not asked for).
struct SetMode {
    const double* base = nullptr;
    bool log_form = false;
    double tau_relu = 0.0, tau_max = 0.0;
    bool bald = false;
    double scale = 0.0;
    double* prob = nullptr;
    long ldp = 0;
};

// What a pass of sets adds to the blocks of its q Sp points
struct SetWs : PassWs {
    DBuf VM, Wbar, Vbar, sum, fbar, gpt, badb, identb;
    DBuf lmq, lzq, lpmx, lpsm, lpbadb, lpwinb;   // the scratch of the log-form selection (launch_qlognei_select)
    DBuf bpp, bkl, bpbar;                        // the scratch of the BTL selection (launch_qbald_select), with lpbadb and lpwinb
    int *lpbad = nullptr, *lpwin = nullptr;
    void ensure_bald(const sls_path* p, int q, int Sp) {
        const size_t nsl = (size_t)qbald_slices(p->n_draws);
        bpp.ensure((size_t)Sp * nsl * q);
        bkl.ensure((size_t)Sp * nsl);
        bpbar.ensure((size_t)Sp * q);
        lpbad = ints(lpbadb, (size_t)Sp * nsl);
        lpwin = ints(lpwinb, (size_t)Sp * nsl * q);
    }
    void ensure_log(const sls_path* p, int q, int Sp) {
        const size_t nsl = (size_t)qlognei_slices(p->n_draws);
        lmq.ensure((size_t)Sp * p->Rp);
        lzq.ensure((size_t)Sp * p->Rp);
        lpmx.ensure((size_t)Sp * nsl);
        lpsm.ensure((size_t)Sp * nsl);
        lpbad = ints(lpbadb, (size_t)Sp * nsl);
        lpwin = ints(lpwinb, (size_t)Sp * nsl * q);
    }
    int* bad = nullptr;     // one flag per set of the pass
    int* ident = nullptr;   // ident[j] = j: point j is evaluated under aggregated column j
    int ident_n = 0;
    // Pp points in Sp sets; values_only: the blocks of the every-draw values alone (sls_path_max_over_points)
    void ensure_sets(sls_ctx* c, const sls_path* p, const GpView& g, int Pp, int Sp, bool values_only = false) {
        const size_t P = Pp, Np = g.Np, Fp = p->Fp;
        ensure(p, g, Pp, values_only);
        VM.ensure(P * p->Rp);
        if (values_only) return;
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

// Every draw at the points of a pass into w.VM (Pp x Rp): the every-draw prefix, then K* V accumulated onto it on the tile GEMM
void draw_values_device(sls_path* p, const GpView& g, SetWs& w, const PassPoints& pt) {
    sls_ctx* c = g.ctx;
    const int Pp = pt.padded();
    every_draw_prefix(p, g, w, pt, Pp, w.VM.p, Pp);
    ProfScope ps(c, "qeubo_data_gemm");
    launch_gemm_plain(c->stream, w.Ks.p, Pp, false, p->V.p, g.Np, true, w.VM.p, Pp, Pp / 128, p->Rp / 128, g.Np, 1.0, 1.0);
}

// qEUBO (+ its qD gradient and the win counts; val, grad, wins may each be nullptr) at M sets, candidate-major raw coordinates
// xr[n + r*ldr], rows iD..iD+D-1 the option i.  val[n], grad[n + r*ldo], wins[n + i*ldw].  The gradient is formed, and looked at by the
// guard, whether or not it is asked for: a set's value does not depend on that.
// base != nullptr (device, n_draws doubles): qNEI -- the selection competes against the per-draw baseline, the guard value is 0 and
// the two kernels count under "qnei".  mode.log_form: qLogNEI -- the selection is launch_qlognei_select (real weights in place of the
// mask), the finish divides nothing, the guard value is SLS_QEUBO_FLOOR and the launches count under "qlognei".
// mode.bald: qBALD -- the selection is launch_qbald_select (real weights again), the finish is launch_qbald_finish (it adds the
// slices' sums of KL_s, divides once and writes mode.prob), the guard value is SLS_QEUBO_FLOOR and the launches count under "qbald".
void qeubo_eval_device(sls_path* p, const GpView& g, SetWs& w, int q, const SetMode& mode, const double* xr, long ldr, int M,
                       double* val, double* grad, long ldo, int* wins, long ldw) {
    sls_ctx* c = g.ctx;
    const double* base = mode.base;
    const char* scope = mode.bald ? "qbald" : mode.log_form ? "qlognei" : base ? "qnei" : "qeubo";
    const double floor = base && !mode.log_form ? 0.0 : SLS_QEUBO_FLOOR;
    const int D = g.D, Np = g.Np, Fp = p->Fp, Rp = p->Rp, S = p->n_draws;
    const int pass_max = std::min(round_up(M, 128), qeubo_sets_per_pass(c, q, Np, Fp, Rp));
    w.ensure_sets(c, p, g, q * pass_max, pass_max);
    if (mode.log_form) w.ensure_log(p, q, pass_max);
    if (mode.bald) w.ensure_bald(p, q, pass_max);
    if (!g.gram_direct) w.ensure_b2(p, g);
    for (int s0 = 0; s0 < M; s0 += pass_max) {
        const int sc = std::min(pass_max, M - s0), Sp = round_up(sc, 128), Pp = q * Sp;
        const PassPoints pt{xr + s0, 1, ldr, q, Sp, sc};   // segment i: option i of the pass's sets
        draw_values_device(p, g, w, pt);
        {
            ProfScope ps(c, scope);
            if (mode.bald)
                launch_qbald_select(c->stream, sc, Sp, q, S, Rp, w.VM.p, Pp, mode.scale, w.bpp.p, w.bkl.p, w.lpbad, w.lpwin, w.bpbar.p,
                                    wins ? wins + s0 : nullptr, ldw, w.bad);
            else if (mode.log_form)
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
        // The gathered route with point j under "draw" j of (Wbar, Vbar).  fbar = fbar_i(x_i) is scratch with no consumer: the route
        // accumulates a value beside the gradient weights, path_data adding onto path_feat's chunk sums.
        gathered_route(p, g, w, pt, w.Wbar.p, 2L * Fp, w.Vbar.p, Np, w.ident, Pp, true, w.fbar.p, w.gpt.p, Pp);
        {
            ProfScope ps(c, scope);
            if (mode.bald)
                launch_qbald_finish(c->stream, sc, Sp, q, D, S, w.bkl.p, w.bad, w.gpt.p, Pp, w.bpbar.p, floor, val ? val + s0 : nullptr,
                                    grad ? grad + s0 : nullptr, ldo, mode.prob ? mode.prob + s0 : nullptr, mode.ldp);
            else
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

// The BTL scale of the choice likelihood, checked once per call before anything is uploaded
static void require_scale(const char* who, double scale) {
    SLS_REQUIRE(std::isnormal(scale) && scale > 0.0, "%s: scale = %g (finite, > 0, not subnormal)", who, scale);
}

static void require_finite_baseline(const char* who, const sls_path* p, const double* baseline) {
    SLS_REQUIRE(baseline != nullptr, "%s: baseline is NULL", who);
    for (int s = 0; s < p->n_draws; ++s) SLS_REQUIRE(std::isfinite(baseline[s]), "%s: baseline[%d] is not finite", who, s);
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
    SetWs ws;
    ws.ensure_sets(c, p, g, pass_max, pass_max, true);
    DBuf raw, tb, ab;
    raw.ensure((size_t)D * Mb);
    h2d(c, raw.p, Xb, (size_t)D * Mb);
    tb.ensure((size_t)nd);
    int* d_arg = ints(ab, (size_t)nd);
    for (int p0 = 0; p0 < Mb; p0 += pass_max) {
        const int pc = std::min(pass_max, Mb - p0), Pp = round_up(pc, 128);
        draw_values_device(p, g, ws, PassPoints{raw.p + (size_t)p0 * D, D, 1, 1, Pp, pc});
        ProfScope ps(c, "path_max");
        launch_path_colmax(c->stream, ws.VM.p, Pp, pc, nd, p0, tb.p, d_arg);   // the pc live rows only
    }
    if (t_out) d2h(c, t_out, tb.p, (size_t)nd);
    if (arg_out) SLS_HIP(hipMemcpyAsync(arg_out, d_arg, (size_t)nd * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    SLS_CATCH
}

// ---- expected utility of the best slider position on the draws (include/sls_hip.h) ------------------------------------------
namespace {

struct LineWs {
    SetWs q;
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
        qeubo_eval_device(p, g, w.q, q, SetMode{base}, w.sets.p, pass_max, sc, val ? val + s0 : nullptr, grad ? w.sgrad.p : nullptr,
                          pass_max, wins ? wins + s0 : nullptr, ldw);
        if (grad) {
            ProfScope ps(c, "line");
            launch_line_fold(c->stream, sc, D, q, anchor != nullptr, w.sgrad.p, pass_max, grad + s0, ldo);
        }
    }
}

// The optional baseline and the optional anchor of the slider and gallery forms
void require_baseline_and_anchor(const char* who, const sls_path* p, const double* baseline, const double* anchor) {
    if (baseline) require_finite_baseline(who, p, baseline);
    if (anchor)
        for (int d = 0; d < p->D; ++d) SLS_REQUIRE(std::isfinite(anchor[d]), "%s: anchor[%d] is not finite", who, d);
}

void require_line_args(const char* who, const sls_path* p, int q, const double* baseline, const double* anchor) {
    SLS_REQUIRE(p != nullptr, "%s: p is NULL", who);
    SLS_REQUIRE(q >= SLS_LINE_MIN_POSITIONS && q <= SLS_QEUBO_MAX_OPTIONS, "%s: q = %d (%d .. %d)", who, q, SLS_LINE_MIN_POSITIONS,
                SLS_QEUBO_MAX_OPTIONS);
    require_baseline_and_anchor(who, p, baseline, anchor);
}

// ---- expected utility of the best gallery cell on the draws (include/sls_hip.h) ----------------------------------------------
// Gallery EUBO (qNEI form with base) at M patches, candidate-major patches[n + r*ld] (4D rows, or 3D rows with the device D-vector
// anchor as c00).  val[n], grad[n + r*ldo] (4D / 3D rows), wins[n + k*ldw] for cell k = i + qs j; each may be nullptr.  Per pass of the
// qEUBO sizing for q = qs qt: expand, ONE pass of qeubo_eval_device, fold -- line_eval_device with the patch's two kernels.
void patch_eval_device(sls_path* p, const GpView& g, LineWs& w, int qs, int qt, const double* base, const double* anchor,
                       const double* patches, long ld, int M, double* val, double* grad, long ldo, int* wins, long ldw) {
    sls_ctx* c = g.ctx;
    const int D = g.D, q = qs * qt;
    const int pass_max = std::min(round_up(M, 128), qeubo_sets_per_pass(c, q, g.Np, p->Fp, p->Rp));
    w.sets.ensure((size_t)q * D * pass_max);
    if (grad) w.sgrad.ensure((size_t)q * D * pass_max);
    for (int s0 = 0; s0 < M; s0 += pass_max) {
        const int sc = std::min(pass_max, M - s0);
        {
            ProfScope ps(c, "patch");
            launch_patch_expand(c->stream, sc, D, qs, qt, patches + s0, ld, anchor, w.sets.p, pass_max);
        }
        qeubo_eval_device(p, g, w.q, q, SetMode{base}, w.sets.p, pass_max, sc, val ? val + s0 : nullptr, grad ? w.sgrad.p : nullptr,
                          pass_max, wins ? wins + s0 : nullptr, ldw);
        if (grad) {
            ProfScope ps(c, "patch");
            launch_patch_fold(c->stream, sc, D, qs, qt, anchor != nullptr, w.sgrad.p, pass_max, grad + s0, ldo);
        }
    }
}

// The cells of a qs x qt grid, or 0 where the grid is outside the contract (either axis below SLS_PATCH_MIN_POSITIONS, or more than
// SLS_QEUBO_MAX_OPTIONS cells); no product is formed of numbers that could overflow it
int patch_cells(int qs, int qt) {
    const bool ok = qs >= SLS_PATCH_MIN_POSITIONS && qt >= SLS_PATCH_MIN_POSITIONS && qs <= SLS_QEUBO_MAX_OPTIONS &&
                    qt <= SLS_QEUBO_MAX_OPTIONS && qs * qt <= SLS_QEUBO_MAX_OPTIONS;
    return ok ? qs * qt : 0;
}

void require_patch_args(const char* who, const sls_path* p, int qs, int qt, const double* baseline, const double* anchor) {
    SLS_REQUIRE(p != nullptr, "%s: p is NULL", who);
    SLS_REQUIRE(patch_cells(qs, qt) > 0, "%s: grid %d x %d (at least %d per axis, at most %d cells)", who, qs, qt,
                SLS_PATCH_MIN_POSITIONS, SLS_QEUBO_MAX_OPTIONS);
    require_baseline_and_anchor(who, p, baseline, anchor);
}

// ---- the host front end of the set-shaped objectives --------------------------------------------------------------------------
// What tells their entry points apart.  sls_qeubo_*: q alone; sls_qnei_*: need_base, the per-draw baseline the options compete
// against; sls_qlognei_*: need_base and taus = (tau_relu, tau_max); sls_line_*: line, with the optional baseline and the optional
// anchor -- one start is then one line, 2D variables (D with the anchor) whatever q is; sls_patch_*: the grid (qs, qt) with q = its
// cells (patch_cells: 0 for a grid outside the contract), the optional baseline and anchor -- one start is one patch, 4D variables
// (3D with the anchor) whatever the grid; sls_qbald_*: scale, the BTL scale of the choice likelihood, and prob, the optional q x M
// output of the predicted choice probabilities (an evaluation's; a maximisation has none).
struct SetCall {
    const char* who;
    int q;
    const double* baseline = nullptr;
    bool need_base = false;
    const double* taus = nullptr;
    bool line = false;
    const double* anchor = nullptr;
    bool patch = false;
    int qs = 0, qt = 0;
    const double* scale = nullptr;
    double* prob = nullptr;
    int nvar(int D) const { return patch ? (anchor ? 3 : 4) * D : !line ? q * D : anchor ? D : 2 * D; }
    const char* block_name() const { return patch ? "patches" : line ? "lines" : "sets"; }
};

// Every refusal ahead of the generation check, in each entry point's order.  M: of an evaluation (nullptr: a maximisation); block:
// the sets / lines / patches / starts.
void require_set_args(const SetCall& s, const sls_path* p, const int* M, const double* block) {
    const char* who = s.who;
    if (!M) SLS_REQUIRE(p && block, "%s: NULL argument", who);
    if (s.patch) {
        require_patch_args(who, p, s.qs, s.qt, s.baseline, s.anchor);
    } else if (s.line) {
        require_line_args(who, p, s.q, s.baseline, s.anchor);
    } else {
        SLS_REQUIRE(p != nullptr, "%s: p is NULL", who);
        SLS_REQUIRE(s.q >= 1 && s.q <= SLS_QEUBO_MAX_OPTIONS, "%s: q = %d (1 .. %d)", who, s.q, SLS_QEUBO_MAX_OPTIONS);
    }
    if (M) {
        SLS_REQUIRE(*M >= 0, "%s: M = %d", who, *M);
        SLS_REQUIRE(block != nullptr, "%s: %s is NULL", who, s.block_name());
    }
    if (s.taus) require_temperatures(who, s.taus);
    if (s.scale) require_scale(who, *s.scale);
    if (s.need_base) require_finite_baseline(who, p, s.baseline);
}

// The optional per-draw baseline and the optional anchor of a call, once to the device (nullptr where absent)
struct SetInputs {
    DBuf base, anchor;
    void upload(sls_ctx* c, const sls_path* p, const SetCall& s) {
        if (s.baseline) {
            base.ensure((size_t)p->n_draws);
            h2d(c, base.p, s.baseline, (size_t)p->n_draws);
        }
        if (s.anchor) {
            anchor.ensure((size_t)p->D);
            h2d(c, anchor.p, s.anchor, (size_t)p->D);
        }
    }
};

// The objective of a call at n columns of candidate-major variables trial[j + r*ld]: val[j], grad[j + r*ldo], wins[j + i*ldw] and,
// of sls_qbald_eval alone, prob[j + i*ldp]
void set_objective(sls_path* p, const GpView& g, LineWs& w, const SetCall& s, const SetInputs& in, const double* trial, long ld, int n,
                   double* val, double* grad, long ldo, int* wins, long ldw, double* prob = nullptr, long ldp = 0) {
    if (s.patch) {
        patch_eval_device(p, g, w, s.qs, s.qt, in.base.p, in.anchor.p, trial, ld, n, val, grad, ldo, wins, ldw);
        return;
    }
    if (s.line) {
        line_eval_device(p, g, w, s.q, in.base.p, in.anchor.p, trial, ld, n, val, grad, ldo, wins, ldw);
        return;
    }
    const SetMode mode{in.base.p,          s.taus != nullptr,        s.taus ? s.taus[0] : 0.0, s.taus ? s.taus[1] : 0.0,
                       s.scale != nullptr, s.scale ? *s.scale : 0.0, prob,                     ldp};
    qeubo_eval_device(p, g, w.q, s.q, mode, trial, ld, n, val, grad, ldo, wins, ldw);
}

// sls_qeubo_eval / sls_qnei_eval / sls_qlognei_eval / sls_qbald_eval / sls_line_eval / sls_patch_eval
int set_eval(const SetCall& s, sls_path* p, const double* block, int M, double* val, double* grad, int* wins) {
    SLS_TRY
    require_set_args(s, p, &M, block);
    GpReadCall call(p->gp, p->generation, s.who);
    if (M == 0) return SLS_OK;
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int q = s.q, nvar = s.nvar(g.D), Mp = round_up(M, 128);
    const std::vector<double> t = host_to_cm(block, nvar, M, Mp);   // alive until the synchronisation below
    DBuf raw, out, wb, pb;
    SetInputs in;
    raw.ensure(t.size());
    h2d(c, raw.p, t.data(), t.size());
    in.upload(c, p, s);
    out.ensure((size_t)Mp * (1 + nvar));
    int* d_wins = wins ? ints(wb, (size_t)Mp * q) : nullptr;
    if (s.prob) pb.ensure((size_t)Mp * q);
    LineWs ws;
    set_objective(p, g, ws, s, in, raw.p, Mp, M, out.p, grad ? out.p + Mp : nullptr, Mp, d_wins, Mp, s.prob ? pb.p : nullptr, Mp);
    std::vector<double> oh((size_t)Mp * (grad ? 1 + nvar : 1));
    std::vector<int> wh(wins ? (size_t)Mp * q : 0);
    std::vector<double> ph(s.prob ? (size_t)Mp * q : 0);
    d2h(c, oh.data(), out.p, oh.size());
    if (s.prob) d2h(c, ph.data(), pb.p, ph.size());
    if (wins) SLS_HIP(hipMemcpyAsync(wh.data(), d_wins, wh.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    cm_to_host(oh.data(), Mp, 1, M, val);
    cm_to_host(oh.data() + Mp, Mp, nvar, M, grad);
    cm_to_host(wh.data(), Mp, q, M, wins);
    cm_to_host(ph.data(), Mp, q, M, s.prob);
    SLS_CATCH
}

// sls_qeubo_maximize / sls_qnei_maximize / sls_qlognei_maximize / sls_qbald_maximize / sls_line_maximize / sls_patch_maximize: the maximiser of
// sls_acq_maximize over the box of the call's variables, one start = one set of q options (one line, one patch).  Workspaces are per
// call; the best start and every fetch come back through pageable memory.
int set_maximize(const SetCall& s, sls_path* p, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                 long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars) {
    SLS_TRY
    require_set_args(s, p, nullptr, starts);
    GpReadCall call(p->gp, p->generation, s.who);
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int nvar = s.nvar(g.D);
    LbfgsWs lb;
    LineWs ws;
    MultistartRun r = maximize_begin(s.who, p->gp, lb, opts, S, n_local, nvar);
    DBuf sd, best;
    SetInputs in;
    sd.ensure((size_t)nvar * S);
    best.ensure((size_t)8 + nvar);
    h2d(c, sd.p, starts, (size_t)nvar * S);
    in.upload(c, p, s);   // once, before the first round
    LockstepStats ls;
    lockstep_rounds(c, r.st, lb, sd.p, S, n_local,
                    [&](const double* trial, long ld, int nlive, const int*, double* val, double* grad) {
                        set_objective(p, g, ws, s, in, trial, ld, nlive, val, grad, ld, nullptr, 0);
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

}  // namespace

// ---- the entry points of the set-shaped objectives: what each asks of set_eval / set_maximize ---------------------------------
extern "C" int sls_qeubo_eval(sls_path* p, int q, const double* sets, int M, double* val, double* grad, int* wins) {
    return set_eval({"sls_qeubo_eval", q}, p, sets, M, val, grad, wins);
}

extern "C" int sls_qeubo_maximize(sls_path* p, int q, const double* starts, int S_starts, int n_local, const sls_lbfgs_opts* opts,
                                  long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars,
                                  double* y_stars) {
    return set_maximize({"sls_qeubo_maximize", q}, p, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out, idx_out,
                        x_stars, y_stars);
}

extern "C" int sls_qnei_eval(sls_path* p, int q, const double* baseline, const double* sets, int M, double* val, double* grad, int* wins) {
    return set_eval({"sls_qnei_eval", q, baseline, true}, p, sets, M, val, grad, wins);
}

extern "C" int sls_qnei_maximize(sls_path* p, int q, const double* baseline, const double* starts, int S_starts, int n_local,
                                 const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                                 double* x_stars, double* y_stars) {
    return set_maximize({"sls_qnei_maximize", q, baseline, true}, p, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out,
                        idx_out, x_stars, y_stars);
}

extern "C" int sls_qlognei_eval(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* sets, int M,
                                double* val, double* grad, int* wins) {
    const double taus[2] = {tau_relu, tau_max};
    return set_eval({"sls_qlognei_eval", q, baseline, true, taus}, p, sets, M, val, grad, wins);
}

extern "C" int sls_qlognei_maximize(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* starts,
                                    int S_starts, int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out,
                                    double* val_out, long* idx_out, double* x_stars, double* y_stars) {
    const double taus[2] = {tau_relu, tau_max};
    return set_maximize({"sls_qlognei_maximize", q, baseline, true, taus}, p, starts, S_starts, n_local, opts, start_index_offset, x_out,
                        val_out, idx_out, x_stars, y_stars);
}

extern "C" int sls_qbald_eval(sls_path* p, int q, double scale, const double* sets, int M, double* val, double* grad, double* prob,
                              int* wins) {
    SetCall s{"sls_qbald_eval", q};
    s.scale = &scale;
    s.prob = prob;
    return set_eval(s, p, sets, M, val, grad, wins);
}

extern "C" int sls_qbald_maximize(sls_path* p, int q, double scale, const double* starts, int S_starts, int n_local,
                                  const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                                  double* x_stars, double* y_stars) {
    SetCall s{"sls_qbald_maximize", q};
    s.scale = &scale;
    return set_maximize(s, p, starts, S_starts, n_local, opts, start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
}

extern "C" int sls_line_eval(sls_path* p, int q, const double* baseline, const double* anchor, const double* lines, int M, double* val,
                             double* grad, int* wins) {
    return set_eval({"sls_line_eval", q, baseline, false, nullptr, true, anchor}, p, lines, M, val, grad, wins);
}

extern "C" int sls_line_maximize(sls_path* p, int q, const double* baseline, const double* anchor, const double* starts, int S_starts,
                                 int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                                 long* idx_out, double* x_stars, double* y_stars) {
    return set_maximize({"sls_line_maximize", q, baseline, false, nullptr, true, anchor}, p, starts, S_starts, n_local, opts,
                        start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
}

extern "C" int sls_patch_eval(sls_path* p, int qs, int qt, const double* baseline, const double* anchor, const double* patches, int M,
                              double* val, double* grad, int* wins) {
    return set_eval({"sls_patch_eval", patch_cells(qs, qt), baseline, false, nullptr, false, anchor, true, qs, qt}, p, patches, M, val,
                    grad, wins);
}

extern "C" int sls_patch_maximize(sls_path* p, int qs, int qt, const double* baseline, const double* anchor, const double* starts,
                                  int S_starts, int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out,
                                  double* val_out, long* idx_out, double* x_stars, double* y_stars) {
    return set_maximize({"sls_patch_maximize", patch_cells(qs, qt), baseline, false, nullptr, false, anchor, true, qs, qt}, p, starts,
                        S_starts, n_local, opts, start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
}
