// C-ABI of the pathwise posterior function draws (include/sls_hip.h: sls_path_*): host orchestration of kernels_path.hip, the
// cross Gram / gradient products of kernels_gram.hip / kernels_acq.hip, the block solve of kernels_tri.hip and the lock-step
// L-BFGS rounds of lbfgs_driver.hpp.  No CPU fallback.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "lbfgs_driver.hpp"

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
    DBuf XsT, ns, Ks, Cs, PG, csum, vpart, Gt, B2, Gpart;
    bool b2_ready = false;
    void ensure(const sls_path* p, const GpView& g, int chunk) {
        const size_t C = chunk, Np = g.Np;
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
    if (grad && !w.b2_ready) {
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
        if (grad) {
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
    SLS_HIP(hipMemcpyAsync(raw.p, Xs, (size_t)D * M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (draw_of_point) {
        int* d_draw = ints(dbuf, (size_t)M);
        SLS_HIP(hipMemcpyAsync(d_draw, draw_of_point, (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
        vout.ensure(Mp);
        if (grad) gout.ensure((size_t)Mp * D);
        EvalWs ws;
        path_eval_device(p, g, ws, raw.p, 0, true, M, d_draw, vout.p, 0, grad ? gout.p : nullptr, Mp);
        SLS_HIP(hipMemcpyAsync(val, vout.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        std::vector<double> gh;
        if (grad) {
            gh.resize((size_t)Mp * D);
            SLS_HIP(hipMemcpyAsync(gh.data(), gout.p, gh.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        SLS_HIP(hipStreamSynchronize(c->stream));
        if (grad)
            for (int m = 0; m < M; ++m)
                for (int d = 0; d < D; ++d) grad[d + (size_t)m * D] = gh[m + (size_t)d * Mp];
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
    SLS_REQUIRE(S >= 1 && n_local >= 1, "sls_path_maximize: need S >= 1 and n_local >= 1 (S = %d, n_local = %d)", S, n_local);
    SLS_REQUIRE((long)S * p->n_draws <= (1L << 26), "sls_path_maximize: n_draws S = %ld starts exceed 2^26", (long)S * p->n_draws);
    const sls_lbfgs_opts o = read_lbfgs_opts(opts);
    SLS_REQUIRE(o.history >= 1 && o.history <= 8, "L-BFGS history must be in 1..8");
    GpReadCall call(p->gp, p->generation, "sls_path_maximize");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws, T = S * nd, Sp = round_up(T, 128);
    LbfgsWs lb;
    EvalWs ws;
    lb.ensure(Sp, o.history, D, Sp);
    LbfgsState st = lb.state(T, D, o);
    int* d_draw = lb.tail();   // the draw of every live column
    DBuf sd;
    sd.ensure((size_t)D * T);
    SLS_HIP(hipMemcpyAsync(sd.p, starts, (size_t)D * T * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the shared lock-step rounds over the active set, with f_{live[j] / S} as the objective of compacted column j
    lockstep_rounds(c, st, lb, sd.p, T, n_local,
                    [&](const double* trial, long ld, int nlive, const int* live, double* val, double* grad) {
                        launch_path_draw_of_live(c->stream, live, nlive, S, d_draw);
                        path_eval_device(p, g, ws, trial, ld, false, nlive, d_draw, val, 0, grad, ld);
                    },
                    nullptr);
    DBuf best;
    best.ensure((size_t)nd * (D + 2));
    launch_path_argmax(c->stream, st.f, S, nd, st.x, Sp, D, best.p);
    std::vector<double> bh((size_t)nd * (D + 2));
    SLS_HIP(hipMemcpyAsync(bh.data(), best.p, bh.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SLS_HIP(hipStreamSynchronize(c->stream));
    for (int s = 0; s < nd; ++s) {
        const double* b = bh.data() + (size_t)s * (D + 2);
        if (val_out) val_out[s] = b[0];
        if (idx_out) idx_out[s] = (long)b[1];
        if (x_out) std::copy(b + 2, b + 2 + D, x_out + (size_t)s * D);
    }
    SLS_CATCH
}
