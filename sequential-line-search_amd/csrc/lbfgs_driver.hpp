// Host side of the multistart L-BFGS maximisers (kernels_acq.hip: lbfgs_step, compact_live, gather_trials): the device blocks of
// one run, the lock-step round loop over the active set, and the maximiser around it that every *_maximize entry point shares --
// maximize_begin (options, workspace, statistics), a search the caller supplies, maximize_finish (winner and per-start results).
#pragma once
#include "common.hpp"

namespace slsk {

// Device blocks of one multistart run; grow-only, so a workspace kept with a handle costs a repeated call no allocation.
struct LbfgsWs {
    DBuf x, g, dir, xt, scr, Sh, Yh, rho, f, t, val, grad, xc, ib;
    size_t Sp = 0;   // of the last ensure(): the integer regions below are carved for it
    // tail: ints behind the named regions, for the caller (sls_path_maximize keeps the draw of every live column there)
    void ensure(int Sp_, int m, int D, size_t tail_ints = 0) {
        const size_t S = Sp = Sp_;
        x.ensure(S * D); g.ensure(S * D); dir.ensure(S * D); xt.ensure(S * D); scr.ensure(S * D);
        const size_t Dh = D <= 16 ? 16 : (D <= 64 ? 64 : D);   // lbfgs_step_reg_kernel keeps rows of 4 DPL doubles per (start, pair)
        Sh.ensure(S * Dh * m); Yh.ensure(S * Dh * m); rho.ensure(S * m);
        f.ensure(S); t.ensure(S); val.ensure(S); grad.ensure(S * D); xc.ensure(S * D);
        // hlen | hpos | nbt | done | live A | live B (Sp each) | count (64) | blocks (Sp / 1024 + 8) | tail | 64 spare
        ib.ensure((6 * S + 64 + (S / 1024 + 8) + tail_ints + 64 + 1) / 2);
    }
    int* ints() const { return reinterpret_cast<int*>(ib.p); }
    int* hlen() const { return ints(); }
    int* hpos() const { return ints() + Sp; }
    int* nbt() const { return ints() + 2 * Sp; }
    int* done() const { return ints() + 3 * Sp; }
    int* live_a() const { return ints() + 4 * Sp; }
    int* live_b() const { return ints() + 5 * Sp; }
    int* count() const { return ints() + 6 * Sp; }     // live count of the compaction
    int* blocks() const { return count() + 64; }       // its per-block counts
    int* tail() const { return blocks() + Sp / 1024 + 8; }
    // the one-wavefront-per-start run (kernels_wave.hip) never compacts: its counters alias the compaction words
    unsigned long long* wave_useful() const { return reinterpret_cast<unsigned long long*>(count() + 32); }
    long long* wave_trace() const { return reinterpret_cast<long long*>(blocks()); }   // 9 words, into the spare ints

    // the kernels' view of a run of S starts (S <= Sp of the last ensure())
    LbfgsState state(int S, int D, const sls_lbfgs_opts& o) const {
        LbfgsState st;
        st.live = nullptr; st.nlive = S; st.ldv = (long)Sp;
        st.S = S; st.D = D; st.m = o.history; st.ld = (long)Sp;
        st.x = x.p; st.g = g.p; st.dir = dir.p; st.xt = xt.p; st.scr = scr.p;
        st.Sh = Sh.p; st.Yh = Yh.p; st.rho = rho.p; st.f = f.p; st.t = t.p;
        st.hlen = hlen(); st.hpos = hpos(); st.nbt = nbt(); st.done = done();
        st.c1 = o.c1; st.shrink = o.shrink; st.gtol = o.gtol; st.max_backtracks = o.max_backtracks;
        st.ftol_rel = o.ftol_rel; st.xtol_rel = o.xtol_rel;
        return st;
    }
};

struct LockstepStats {
    long issued = 0;             // evaluations of starts that were still moving
    int rounds = 0, live_end = 0;
    // a search that counts `issued` on the device instead: maximize_finish reads the counter back with the best start
    const unsigned long long* issued_dev = nullptr;
};

// Lock-step rounds over the ACTIVE SET.  NLopt's max_evals is a cap per start, not a quota (src/acquisition-function.cpp:128-129): a
// start that can no longer move (stationary projected gradient, null step, exhausted backtracking) is finished.  After every round
// the starts still moving are compacted, in increasing order, into dense 128-wide tiles, so the evaluation only sees live columns.
// A candidate's arithmetic does not depend on the column it occupies, so every start ends with the same bits as in the uncompacted
// schedule (SLS_COMPACT=0: every start is re-evaluated every round; tests compare the two).
//   eval(trial, ld, nlive, live, val, grad): objective and gradient at the candidate-major trial points trial[j + d*ld], j < nlive;
//   column j belongs to start live[j] (device; nullptr: identity).  Ends with the starts' points in st.x and values in st.f.
template <class Eval>
void lockstep_rounds(sls_ctx* c, LbfgsState& st, LbfgsWs& ws, const double* starts_dev, int S, int n_local, Eval&& eval,
                     LockstepStats* stats) {
    const bool compact = tune_on(TUNE_COMPACT);
    const int D = st.D;
    const long Sp = st.ld;
    launch_clamp_starts(c->stream, starts_dev, D, S, st.xt, Sp, (int)Sp);
    const double* trial = st.xt;      // candidate-major trial points of this round, leading dimension Sp
    const int* live = nullptr;        // identity
    int nlive = S, moving = S;
    LockstepStats s;
    for (int ev = 0; ev < n_local && nlive > 0; ++ev) {
        eval(trial, Sp, nlive, live, ws.val.p, ws.grad.p);
        s.issued += compact ? nlive : moving;             // SLS_COMPACT=0 evaluates finished starts too: they do not count
        s.rounds += 1;
        {
            ProfScope ps(c, "lbfgs");
            st.live = live; st.nlive = nlive;
            launch_lbfgs_step(c->stream, st, ws.val.p, ws.grad.p, ev == 0);
            if (ev + 1 < n_local) {
                int* live_next = (live == ws.live_a()) ? ws.live_b() : ws.live_a();
                launch_compact_live(c->stream, live, nlive, st.done, live_next, ws.count(), ws.blocks());
                if (compact) {
                    launch_gather_trials(c->stream, st.xt, Sp, D, live_next, ws.count(), nlive, ws.xc.p, Sp);
                    live = live_next;
                    trial = ws.xc.p;
                }
            }
        }
        if (ev + 1 < n_local) {
            int cnt = 0;
            SLS_HIP(hipMemcpyAsync(&cnt, ws.count(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
            SLS_HIP(hipStreamSynchronize(c->stream));
            if (compact) nlive = cnt;
            else moving = cnt;                            // statistics only: the launch shapes stay at S
        }
    }
    s.live_end = compact ? nlive : moving;
    if (stats) *stats = s;
}

// ---- the maximiser around a search ------------------------------------------------------------------------------------------------
// One run over S starts in nvar variables (D; 2D for query pairs; qD for sets of q options).
struct MultistartRun {
    sls_lbfgs_opts o;
    LbfgsState st;       // st.S starts, st.D variables, leading dimension st.ld = round_up(S, 128)
    int n_local;
    sls_gp* stats_of;    // the handle whose sls_acq_last_stats this run is (nullptr: none)
};

// Prologue: the caller's options over the defaults, the workspace (the handle's on the sls_gp routes, so that a repeated call costs no
// allocation; tail_ints as in LbfgsWs::ensure) and the statistics of a run that has not evaluated anything yet.
inline MultistartRun maximize_begin(const char* who, sls_gp* stats_of, LbfgsWs& ws, const sls_lbfgs_opts* opts, int S, int n_local,
                                    int nvar, size_t tail_ints = 0) {
    SLS_REQUIRE(S >= 1 && n_local >= 1, "%s: need S >= 1 and n_local >= 1 (S = %d, n_local = %d)", who, S, n_local);
    const sls_lbfgs_opts o = read_lbfgs_opts(opts);
    SLS_REQUIRE(o.history >= 1 && o.history <= 8, "%s: L-BFGS history must be in 1..8 (got %d)", who, o.history);
    ws.ensure(round_up(S, 128), o.history, nvar, tail_ints);
    MultistartRun r;
    r.o = o;
    r.st = ws.state(S, nvar, o);
    r.n_local = n_local;
    r.stats_of = stats_of;
    if (stats_of) gp_set_acq_stats(stats_of, 0, (long)S * n_local, 0, 0);
    return r;
}

// Between the two, the search: lockstep_rounds with the caller's objective, or anything else that leaves the starts' end points in
// st.x and their negated values in st.f on the context's stream and says what it did in a LockstepStats.

// The best start's block, 8 + nvar doubles (launch_argmax_neg_gather): a mapped block as the device and the host see it, or
// (copy) a device block and pageable memory it is copied to ahead of the synchronisation.
struct BestBlock {
    double* dev;
    double* host;
    bool copy;
};

// Epilogue of a maximiser with ONE winner: first maximum of -f and its point in one launch, ONE synchronisation, the statistics, then
// what the caller asked for -- value, index (+ off) and point of the winner; every start's end point (x_stars, nvar x S column-major)
// and value (y_stars).  fetch(dev, n): n doubles of device memory where the host can read them on return (one synchronisation each).
// Returns the winner's index among the S starts (without `off`).
template <class Fetch>
long maximize_finish(sls_ctx* c, const MultistartRun& r, const LockstepStats& ls, BestBlock best, Fetch&& fetch, long off,
                     double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars) {
    const LbfgsState& st = r.st;
    const int S = st.S, nvar = st.D;
    launch_argmax_neg_gather(c->stream, st.f, S, st.x, st.ld, nvar, best.dev, ls.issued_dev);
    if (best.copy) d2h(c, best.host, best.dev, (size_t)8 + nvar);
    SLS_HIP(hipStreamSynchronize(c->stream));
    const double* b = best.host;
    const long winner = (long)b[1];   // taken here, once: callers need not read the best block again behind the fetches below
    if (r.stats_of) gp_set_acq_stats(r.stats_of, ls.issued_dev ? (long)b[2] : ls.issued, (long)S * r.n_local, ls.rounds, ls.live_end);
    if (val_out) *val_out = b[0];
    if (idx_out) *idx_out = winner + off;
    if (x_out) std::copy(b + 8, b + 8 + nvar, x_out);
    if (x_stars) cm_to_host(fetch(st.x, (size_t)st.ld * nvar), st.ld, nvar, S, x_stars);
    if (y_stars) {
        const double* f = fetch(st.f, (size_t)st.ld);
        for (int i = 0; i < S; ++i) y_stars[i] = -f[i];
    }
    return winner;
}

}  // namespace slsk
