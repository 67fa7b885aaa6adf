// C-ABI of the pathwise posterior function draws (include/sls_hip.h: sls_path_*): host orchestration of kernels_path.hip, the
// cross Gram / gradient products of kernels_gram.hip / kernels_acq.hip, the block solve of kernels_tri.hip and the lock-step
// L-BFGS of kernels_vec.hip.  No CPU fallback.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

using namespace slsk;

namespace {

constexpr int PATH_MAX_DRAWS = 4096;
constexpr int PATH_MAX_FREQ = 16384;

#define SLS_TRY slsk::note_entry(); try {
#define SLS_CATCH                                   \
    }                                               \
    catch (const slsk::HipFail& f) { return f.code; } \
    catch (const std::exception& e) {               \
        slsk::set_error("exception: %s", e.what()); \
        return SLS_ERR_INVALID;                     \
    }                                               \
    return SLS_OK;

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

// the context's lock, the handle's state lock (shared), and a handle that still is what the object was made from
struct PathCall {
    std::unique_lock<std::recursive_mutex> ctx_lock;
    std::shared_lock<std::shared_mutex> state_lock;
    GpView g;
    PathCall(sls_gp* gp, const sls_path* p, const char* who) : g(gp_view(gp)) {
        ctx_lock = std::unique_lock<std::recursive_mutex>(g.ctx->mtx);
        (void)hipSetDevice(g.ctx->device);
        state_lock = std::shared_lock<std::shared_mutex>(*g.state);
        g = gp_view(gp);
        if (p)
            SLS_REQUIRE(g.generation == p->generation,
                        "%s: the GP handle was refitted or grown since sls_path_create (generation %ld, now %ld): create a new object",
                        who, p->generation, g.generation);
    }
};

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

// L-BFGS state of one sls_path_maximize call
struct LbfgsWs {
    DBuf x, g, dir, xt, scr, Sh, Yh, rho, f, t, val, grad, xc, ib;
    int* ints = nullptr;
    void ensure(int Sp, int m, int D) {
        const size_t S = Sp;
        x.ensure(S * D); g.ensure(S * D); dir.ensure(S * D); xt.ensure(S * D); scr.ensure(S * D);
        const size_t Dh = D <= 16 ? 16 : (D <= 64 ? 64 : D);   // as capi.hip: lbfgs_step_reg_kernel's rows of 4 DPL doubles
        Sh.ensure(S * Dh * m); Yh.ensure(S * Dh * m); rho.ensure(S * m);
        f.ensure(S); t.ensure(S); val.ensure(S); grad.ensure(S * D); xc.ensure(S * D);
        ints = ::ints(ib, S * 7 + 128 + S / 1024 + 8);   // hlen | hpos | nbt | done | live A | live B | count (64) | blocks | draws
    }
};

}  // namespace

extern "C" int sls_path_create(sls_gp* gp, int n_draws, int n_freq, unsigned long long seed, sls_path** out) {
    SLS_TRY
    SLS_REQUIRE(gp && out, "sls_path_create: NULL argument");
    *out = nullptr;
    SLS_REQUIRE(n_draws >= 1 && n_draws <= PATH_MAX_DRAWS, "sls_path_create: n_draws = %d (1 .. %d)", n_draws, PATH_MAX_DRAWS);
    SLS_REQUIRE(n_freq >= 1 && n_freq <= PATH_MAX_FREQ, "sls_path_create: n_freq = %d (1 .. %d)", n_freq, PATH_MAX_FREQ);
    PathCall call(gp, nullptr, "sls_path_create");
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
    sls_ctx* c = p->ctx;
    {
        std::unique_lock<std::recursive_mutex> lock_(c->mtx);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        delete p;
    }
    ctx_release(c);
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
    PathCall call(p->gp, p, "sls_path_eval");
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
    PathCall call(p->gp, p, "sls_path_maximize");
    const GpView& g = call.g;
    sls_ctx* c = g.ctx;
    const int D = g.D, nd = p->n_draws, T = S * nd, Sp = round_up(T, 128);
    LbfgsWs lb;
    EvalWs ws;
    lb.ensure(Sp, o.history, D);
    int* lb_int = lb.ints;
    LbfgsState st;
    st.live = nullptr; st.nlive = T; st.ldv = Sp;
    st.S = T; st.D = D; st.m = o.history; st.ld = Sp;
    st.x = lb.x.p; st.g = lb.g.p; st.dir = lb.dir.p; st.xt = lb.xt.p; st.scr = lb.scr.p;
    st.Sh = lb.Sh.p; st.Yh = lb.Yh.p; st.rho = lb.rho.p; st.f = lb.f.p; st.t = lb.t.p;
    st.hlen = lb_int; st.hpos = lb_int + Sp; st.nbt = lb_int + 2 * (size_t)Sp; st.done = lb_int + 3 * (size_t)Sp;
    st.c1 = o.c1; st.shrink = o.shrink; st.gtol = o.gtol; st.max_backtracks = o.max_backtracks;
    st.ftol_rel = o.ftol_rel; st.xtol_rel = o.xtol_rel;
    int* live_a = lb_int + 4 * (size_t)Sp;
    int* live_b = live_a + Sp;
    int* d_count = live_b + Sp;
    int* d_blocks = d_count + 64;
    int* d_draw = d_blocks + Sp / 1024 + 8;
    DBuf sd;
    sd.ensure((size_t)D * T);
    SLS_HIP(hipMemcpyAsync(sd.p, starts, (size_t)D * T * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // The lock-step rounds of capi.hip's maximize_impl over the active set, with f_{live[j] / S} as the objective of compacted column
    // j.  A candidate's arithmetic does not depend on its column, so SLS_COMPACT=0 (every start re-evaluated every round) ends with
    // the same bits.
    const bool compact = tune_on(TUNE_COMPACT);
    launch_clamp_starts(c->stream, sd.p, D, T, st.xt, Sp, Sp);
    const double* trial = st.xt;
    const int* live = nullptr;
    int nlive = T;
    for (int ev = 0; ev < n_local && nlive > 0; ++ev) {
        launch_path_draw_of_live(c->stream, live, nlive, S, d_draw);
        path_eval_device(p, g, ws, trial, Sp, false, nlive, d_draw, lb.val.p, 0, lb.grad.p, Sp);
        {
            ProfScope ps(c, "lbfgs");
            st.live = live; st.nlive = nlive;
            launch_lbfgs_step(c->stream, st, lb.val.p, lb.grad.p, ev == 0);
            if (ev + 1 < n_local) {
                int* live_next = (live == live_a) ? live_b : live_a;
                launch_compact_live(c->stream, live, nlive, st.done, live_next, d_count, d_blocks);
                if (compact) {
                    launch_gather_trials(c->stream, st.xt, Sp, D, live_next, d_count, nlive, lb.xc.p, Sp);
                    live = live_next;
                    trial = lb.xc.p;
                }
            }
        }
        if (ev + 1 < n_local && compact) {
            int cnt = 0;
            SLS_HIP(hipMemcpyAsync(&cnt, d_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            SLS_HIP(hipStreamSynchronize(c->stream));
            nlive = cnt;
        }
    }
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
