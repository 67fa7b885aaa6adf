"""Restatement of the multi-start bounded L-BFGS step (csrc/kernels_acq.hip: lbfgs_step_kernel, driven as lockstep_rounds in
csrc/lbfgs_driver.hpp drives it with SLS_COMPACT=1) with the objective as a callable.  No GPU, no oracle: numpy only.

Only the optimiser arithmetic lives here.  Every statement of the kernel has its line below, in the kernel's order; products are
rounded before they are added (no fused multiply-add), and every sum over the coordinates goes through coord_sum(), which knows
two orders:
  "sequential"  d = 0, 1, 2, ... into one accumulator          (oracle/sls_oracle.c)
  "lanes"       four accumulators over d mod 4, each in increasing d, combined (q0 + q1) + (q2 + q3)   (the device)
The starts are vectorised (arrays are nvar x S); nothing couples two starts."""
import numpy as np


def coord_sum(a, order):
    """Sum of a (nvar x k) over the coordinates, per column, in the named order."""
    a = np.asarray(a, dtype=np.float64)
    k = a.shape[1]
    if order == "sequential":
        acc = np.zeros(k)
        for d in range(a.shape[0]):
            acc = acc + a[d]
        return acc
    if order == "lanes":
        part = [np.zeros(k) for _ in range(4)]
        for d in range(a.shape[0]):
            part[d % 4] = part[d % 4] + a[d]
        return (part[0] + part[1]) + (part[2] + part[3])
    raise ValueError(f"order must be 'lanes' or 'sequential', got {order!r}")


def f_stalled(f_old, f_new, tol):
    """lbfgs_f_stalled (csrc/kernels.hpp)."""
    if not tol > 0.0:
        return np.zeros(np.shape(f_old), dtype=bool)
    return (np.abs(f_new - f_old) < tol * 0.5 * (np.abs(f_new) + np.abs(f_old))) | (f_new == f_old)


def x_moved(x_old, x_new, tol):
    """lbfgs_x_moved (csrc/kernels.hpp): True where the coordinate still moved by more than its tolerance."""
    return ~((np.abs(x_new - x_old) < tol * 0.5 * (np.abs(x_new) + np.abs(x_old))) | (x_new == x_old))


def run(evaluate, starts, n_local, history=6, c1=1e-4, shrink=0.5, gtol=0.0, max_backtracks=20, ftol_rel=0.0, xtol_rel=0.0,
        order="lanes", with_live=False):
    """Maximise over [0,1]^nvar from every column of starts (nvar x S).  evaluate(T) gets the nvar x k trial points of the live
    starts, in increasing start order, and returns (val[k], grad[nvar x k]) of the function to be MAXIMISED; with_live=True it is
    called as evaluate(T, live), live[j] = the start of column j (an objective that differs from start to start).  Returns a dict:
    x_stars (nvar x S), y_stars, index / value / x of the first maximum, armijo_margin (oracle/sls_oracle.c: the smallest
    |ft - (f + c1 g.s)| / max(|f|, |ft|) over the start's Armijo tests, inf when it had none), evals_issued (sum of the live counts per
    round), rounds, live_at_end, evals (per start), accepted (per start: accepted steps), ring_max (per start: largest ring length)."""
    starts = np.asarray(starts, dtype=np.float64)
    nvar, S = starts.shape
    m = int(history)
    assert S >= 1 and n_local >= 1 and 1 <= m
    csum = lambda a: coord_sum(a, order)

    x = np.zeros((nvar, S)); g = np.zeros((nvar, S)); dirn = np.zeros((nvar, S))
    Sh = np.zeros((m, nvar, S)); Yh = np.zeros((m, nvar, S)); rho = np.zeros((m, S))
    f = np.zeros(S); t = np.ones(S)
    hlen = np.zeros(S, dtype=np.int64); hpos = np.zeros(S, dtype=np.int64); nbt = np.zeros(S, dtype=np.int64)
    done = np.zeros(S, dtype=bool)
    margin = np.full(S, np.inf)
    evals = np.zeros(S, dtype=np.int64); accepted = np.zeros(S, dtype=np.int64); ring_max = np.zeros(S, dtype=np.int64)

    xt = np.minimum(np.maximum(starts, 0.0), 1.0)          # clamp_starts_kernel
    live = np.arange(S)
    issued = rounds = 0
    for ev in range(n_local):
        if live.size == 0:
            break
        T = np.asfortranarray(xt[:, live])
        val, grad = evaluate(T, live.copy()) if with_live else evaluate(T)
        val = np.asarray(val, dtype=np.float64).reshape(live.size)
        grad = np.asarray(grad, dtype=np.float64).reshape(nvar, live.size)
        issued += live.size
        rounds += 1
        evals[live] += 1

        # ---- one lbfgs_step over the live columns; n = the starts this block of statements still applies to
        if ev == 0:
            n = live
            f[n] = -val
            x[:, n] = xt[:, n]
            g[:, n] = -grad
            need_dir = np.ones(n.size, dtype=bool)
        else:
            ft = -val
            sd = xt[:, live] - x[:, live]
            gs = csum(g[:, live] * sd)
            ss = csum(sd * sd)
            null = ss == 0.0
            done[live[null]] = True                          # ss == 0: stop, state untouched
            keep = ~null
            n, ft, gs, sd = live[keep], ft[keep], gs[keep], sd[:, keep]
            gt = -grad[:, keep]
            sc = np.maximum(np.abs(f[n]), np.abs(ft))
            mg = np.abs(ft - (f[n] + c1 * gs)) / np.where(sc > 0.0, sc, 1.0)
            margin[n] = np.minimum(margin[n], mg)
            acc = ft <= f[n] + c1 * gs                       # Armijo
            need_dir = acc.copy()
            # accepted step
            a = n[acc]
            if a.size:
                idx = hpos[a]
                sa = sd[:, acc]
                ya = gt[:, acc] - g[:, a]
                still = x_moved(x[:, a], xt[:, a], xtol_rel).any(axis=0)
                Sh[idx, :, a] = sa.T
                Yh[idx, :, a] = ya.T
                sy = csum(sa * ya)
                yy = csum(ya * ya)
                x[:, a] = xt[:, a]
                g[:, a] = gt[:, acc]
                ok = (sy > 1e-10 * yy) & (sy > 0.0)
                ao, io = a[ok], idx[ok]
                rho[io, ao] = 1.0 / sy[ok]
                hpos[ao] = (io + 1) % m
                hlen[ao] = np.minimum(hlen[ao] + 1, m)
                stop = f_stalled(f[a], ft[acc], ftol_rel)
                if xtol_rel > 0.0:
                    stop = stop | ~still
                done[a[stop]] = True
                f[a] = ft[acc]
                accepted[a] += 1
                ring_max[a] = np.maximum(ring_max[a], hlen[a])
            # rejected step
            r = n[~acc]
            t[r] *= shrink
            nbt[r] += 1
            done[r[nbt[r] > max_backtracks]] = True

        # ---- direction: projected gradient, two-loop recursion
        p = n[need_dir & ~done[n]]
        if p.size:
            pg = g[:, p].copy()
            xv = x[:, p]
            pg[((xv <= 0.0) & (pg > 0.0)) | ((xv >= 1.0) & (pg < 0.0))] = 0.0
            pgmax = np.fmax.reduce(np.abs(pg), axis=0, initial=0.0)
            pgn2 = csum(pg * pg)
            stat = ~(pgmax > gtol)
            done[p[stat]] = True
            go = ~stat
            p, pg, pgn2 = p[go], pg[:, go], pgn2[go]
        if p.size:
            dv = pg.copy()
            hl, hp = hlen[p].copy(), hpos[p]
            al = np.zeros((m, p.size))
            for h in range(m):
                w = np.nonzero(h < hl)[0]
                if not w.size:
                    continue
                idx = (hp[w] - 1 - h + 2 * m) % m
                s_, y_ = Sh[idx, :, p[w]].T, Yh[idx, :, p[w]].T
                al[h, w] = rho[idx, p[w]] * csum(s_ * dv[:, w])
                dv[:, w] = dv[:, w] - al[h, w] * y_
            nn = np.sqrt(pgn2)
            gamma = 1.0 / np.where(nn > 1.0, nn, 1.0)
            w = np.nonzero(hl > 0)[0]
            if w.size:
                idx = (hp[w] - 1 + m) % m
                s_, y_ = Sh[idx, :, p[w]].T, Yh[idx, :, p[w]].T
                gamma[w] = csum(s_ * y_) / csum(y_ * y_)
            dv = dv * gamma
            for h in range(m - 1, -1, -1):
                w = np.nonzero(h < hl)[0]
                if not w.size:
                    continue
                idx = (hp[w] - 1 - h + 2 * m) % m
                s_, y_ = Sh[idx, :, p[w]].T, Yh[idx, :, p[w]].T
                beta = rho[idx, p[w]] * csum(y_ * dv[:, w])
                dv[:, w] = dv[:, w] + s_ * (al[h, w] - beta)
            dv = np.where(pg == 0.0, 0.0, -dv)
            gd = csum(pg * dv)
            fb = np.nonzero(~(gd < 0.0))[0]                  # not a descent direction: steepest descent, empty ring
            if fb.size:
                hlen[p[fb]] = 0
                nf = np.sqrt(pgn2[fb])
                gf = 1.0 / np.where(nf > 1.0, nf, 1.0)
                dv[:, fb] = -gf * pg[:, fb]
                gd[fb] = csum(pg[:, fb] * dv[:, fb])
                done[p[fb[~(gd[fb] < 0.0)]]] = True
            dirn[:, p] = dv
            ok = ~done[p]
            t[p[ok]] = 1.0
            nbt[p[ok]] = 0

        # ---- next trial; one that does not move retires the start here, one evaluation early
        v = x[:, n].copy()
        mv = np.nonzero(~done[n])[0]
        if mv.size:
            nm = n[mv]
            tv = x[:, nm] + t[nm] * dirn[:, nm]
            tv = np.where(tv < 0.0, 0.0, np.where(tv > 1.0, 1.0, tv))
            v[:, mv] = tv
            done[nm[~(tv != x[:, nm]).any(axis=0)]] = True
        xt[:, n] = v

        if ev + 1 < n_local:                                 # compact_live (not after the last round)
            live = live[~done[live]]

    y_stars = -f
    best = int(np.argmax(y_stars))                           # first maximum
    return dict(x_stars=np.asfortranarray(x), y_stars=y_stars, index=best, value=float(y_stars[best]), x=x[:, best].copy(),
                armijo_margin=margin, evals_issued=int(issued), rounds=int(rounds), live_at_end=int(live.size), evals=evals,
                accepted=accepted, ring_max=ring_max)
