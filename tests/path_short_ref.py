"""Direct-difference restatement of the pathwise posterior draws and of what is built on them, for handles whose fit lies beyond the
guard of the norm expansion (tests/test_path_short_ref_cpu.py, tests/test_gpu_short_length_scales_paths.py).

path_ref.kernel_c takes q from |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j, which is wrong by eps D / (2 l^2) absolute: the restatement the
path tests use cannot judge the regime the direct form exists for.  Here the data term k(x, X) v, its gradient and K_y itself come
from gram_ref (raw coordinates differenced first, divided by l afterwards), the generator layout from path_ref (frequencies,
draw_normals: their fp64 outputs are the inputs on both sides), and everything is evaluated in numpy.float64 or numpy.longdouble:

  f_s(x) = sqrt(a/F) sum_l [ w_{s,l} cos(om_l . x~) + w'_{s,l} sin(om_l . x~) ]  +  sum_i v_{s,i} k(x, x_i)
  v_s    = K_y^-1 ( y - f_prior,s(X) - sqrt(b) eps_s ),   x~ = (x - 0.5) / l

A ShortPathRef has the attributes qeubo_ref / qnei_ref / line_ref read from a path_ref.PathRef (D, N, F, n_draws, a, ell, theta,
kernel, X, om, W, v, eval_all) and its own grad_with_weights, so their selection logic runs on it unchanged.  EUBO pairs go through
eubo_ref.closed_form on gram_ref.predict's mean and covariance.

band(): per quantity max |float64 - longdouble| of this restatement, the reference's own rounding at that case; the GPU tests add 16
bands to the tolerance the entry point's ordinary restatement test uses (tolerances())."""
import numpy as np

import eubo_ref
import gram_ref as gr
import path_ref as ph
import qeubo_ref as qr
import qnei_ref as nr

EPS = gr.EPS
F, SEED = 200, 4321                                    # Fp = 256
SIZES = ((129, 6), (300, 33), (200, 65))               # both sides of one 128-row tile, of D = 32 / 64; a second dimension chunk
ELL_CASES = (0.3, 3e-3, 1e-5, 1e-8, "ard")
CASES = [(N, D, case, 5) for (N, D) in SIZES for case in ELL_CASES] + [(200, 65, 0.02, 5), (129, 6, 1e-5, 130)]
# D > 128 (gram_ref.WIDE_CASES): Dcols = 256 / 384 and Dp = 144 / 208 / 272 in the feature and gradient kernels, tiled routes only
WIDE_CASES = [(N, D, case, 5) for (N, D, case) in gr.WIDE_CASES]
CASES += WIDE_CASES
INSIDE = [(N, D, 0.3) for (N, D) in SIZES] + list(gr.WIDE_DENSE)            # the cases inside the guard of the norm expansion
QS = (2, 5, 16)
LINE_Q = 4
BAND_FACTOR = 16.0                                     # device and restatement: two fp64 evaluations in different summation orders
MARGIN_FACTOR = 100.0                                  # a winner counts where it leads by this many value tolerances
MAX_DROPPED = 0.10
# EUBO pairs among gram_ref's candidates: two ordinary, near a training point / ordinary, outside the box / ordinary, the near-duplicates
PAIRS = ((0, 1), (28, 2), (16, 3), gr.CAND_PAIR)
PAIR_NAMES = ("ordinary", "near_training", "outside_box", "near_duplicate")


def beyond_guard(ell, D):
    """gram_expansion_ok of csrc/kernels.hpp, negated: ilm^2 (D/2) 2.3e-16 > 1e-11."""
    ilm = 1.0 / float(np.min(ell))
    return ilm * ilm * (D / 2.0) * 2.3e-16 > 1e-11


class ShortPathRef:
    """The n_draws draws of an object made from (X, y, theta, b, kernel) with F frequencies and stream `seed`, in `dtype`."""

    def __init__(self, X, y, theta, b, kernel, n_draws, F, seed, dtype=np.float64, fit=None):
        dt = self.dt = dtype
        self.X, self.y = np.asarray(X, dtype=dt), np.asarray(y, dtype=dt)
        self.theta = np.asarray(theta, dtype=dt)
        self.D, self.N = self.X.shape
        self.a, self.ell, self.b, self.kernel = self.theta[0], self.theta[1:], dt(b), kernel
        self.F, self.n_draws = F, n_draws
        self.om = ph.frequencies(seed, self.D, F, kernel).astype(dt)
        w, wp, eps = (z.astype(dt) for z in ph.draw_normals(seed, self.D, self.N, F, kernel, n_draws))
        self.eps = eps
        self.W = np.sqrt(self.a / dt(F)) * np.vstack([w, wp])                                   # 2F x n_draws
        self.fit = gr.fit(X, y, np.asarray(theta[1:], dtype=np.float64), float(theta[0]), float(b), kernel, dt) if fit is None else fit
        assert self.fit["dtype"] is dt
        self.Ky = self.fit["K"]
        r = self.y[:, None] - self.prior_all(self.X) - np.sqrt(self.b) * eps
        self.v = self.fit["Li"].T @ (self.fit["Li"] @ r)                                        # N x n_draws

    # ---- the two terms ----------------------------------------------------------------------------------------------------------
    def phase(self, Xs):
        return self.om @ ((np.asarray(Xs, dtype=self.dt) - self.dt(0.5)) / self.ell[:, None])   # F x M

    def prior_all(self, Xs):
        T = self.phase(Xs)
        return np.cos(T).T @ self.W[:self.F] + np.sin(T).T @ self.W[self.F:]

    def kc(self, Xs):
        """(k, c) between the columns of Xs and the training points, M x N each, from raw coordinate differences."""
        return gr.kern(gr.sqdist(Xs, self.X, self.ell, self.dt), self.a, self.kernel, self.dt)

    def data_all(self, Xs):
        return self.kc(Xs)[0] @ self.v

    def eval_all(self, Xs):
        """M x n_draws."""
        return self.prior_all(Xs) + self.data_all(Xs)

    def grad_parts(self, Xs, Wb, Vb):
        """(prior term, data term) of the gradient (D x M each) at Xs[:, m] of the path function with weights (Wb[:, m] (2F),
        Vb[:, m] (N)).  Data term: -sum_i c_i v_i (x_d - x_id) / l_d^2, the difference taken first."""
        dt = self.dt
        Xs, Wb, Vb = np.asarray(Xs, dtype=dt), np.asarray(Wb, dtype=dt), np.asarray(Vb, dtype=dt)
        T = self.phase(Xs)
        g = Wb[self.F:] * np.cos(T) - Wb[:self.F] * np.sin(T)
        gp = (self.om.T @ g) / self.ell[:, None]
        cv = self.kc(Xs)[1] * Vb.T                                                              # M x N
        gd = np.empty(Xs.shape, dtype=dt)
        for d in range(self.D):
            gd[d] = -((Xs[d][:, None] - self.X[d][None, :]) * cv).sum(axis=1) / (self.ell[d] * self.ell[d])
        return gp, gd

    def grad_with_weights(self, Xs, Wb, Vb):
        gp, gd = self.grad_parts(Xs, Wb, Vb)
        return gp + gd

    def eval(self, Xs, draws, parts=False):
        """(val (M,), grad (D x M)) of f_{draws[m]} at Xs[:, m]; with parts, a dict of the prior and the data term of each as well."""
        draws = np.asarray(draws)
        T = self.phase(Xs)
        wc, ws = self.W[:self.F, draws], self.W[self.F:, draws]
        vp = np.sum(wc * np.cos(T) + ws * np.sin(T), axis=0)
        vd = np.sum(self.kc(Xs)[0] * self.v[:, draws].T, axis=1)
        gp, gd = self.grad_parts(Xs, self.W[:, draws], self.v[:, draws])
        if parts:
            return vp + vd, gp + gd, dict(val_prior=vp, val_data=vd, grad_prior=gp, grad_data=gd)
        return vp + vd, gp + gd

    def data_identity(self):
        """y_i - sqrt(b) eps_{s,i} - b v_{s,i}: what f_s(x_i) equals (path_ref.PathRef.data_identity)."""
        return self.y[:, None] - np.sqrt(self.b) * self.eps - self.b * self.v


def eubo(fit, pairs):
    """eubo_ref.closed_form on the posterior of gram_ref: fit a gram_ref.fit(), pairs (2D, M).  Returns (val, grad, info) with
    info's keys as eubo_ref.eubo's (what tests/test_gpu_eubo.py's tolerances read); the posterior is formed in the fit's number type,
    the closed form (erfc) in float64."""
    dt = fit["dtype"]
    pairs = np.asarray(pairs, dtype=np.float64)
    D, M = pairs.shape[0] // 2, pairs.shape[1]
    P = np.concatenate([pairs[:D], pairs[D:]], axis=1)
    p = gr.predict(fit, P, want_grad=True)
    i, j = np.arange(M), M + np.arange(M)
    mu = np.stack([p["mean"][i], p["mean"][j]])
    s2 = p["cov"][i, i] + p["cov"][j, j] - dt(2) * p["cov"][i, j]
    X, ell, a = np.asarray(fit["X"], dtype=dt), np.asarray(fit["ell"], dtype=dt), fit["a"]
    x = [np.asarray(pairs[:D], dtype=dt), np.asarray(pairs[D:], dtype=dt)]
    kc = [gr.kern(gr.sqdist(X, x[o], ell, dt), a, fit["kernel"], dt) for o in range(2)]         # N x M
    w = fit["Kinv"] @ (kc[0][0] - kc[1][0])
    q12 = np.zeros(M, dtype=dt)
    for d in range(D):
        t = (x[0][d] - x[1][d]) / ell[d]
        q12 += t * t
    c12 = gr.kern(q12, a, fit["kernel"], dt)[1]
    dmu = np.stack([p["dmean"][:, i], p["dmean"][:, j]])
    ds2 = np.empty((2, D, M), dtype=dt)
    for o in range(2):
        cw = kc[o][1] * w
        for d in range(D):
            e = c12 * (x[0][d] - x[1][d]) / (ell[d] * ell[d])
            T = ((x[o][d][None, :] - X[d][:, None]) * cw).sum(axis=0) / (ell[d] * ell[d])
            ds2[o, d] = (dt(2) if o == 0 else dt(-2)) * (e + T)
    f64 = [np.asarray(z, dtype=np.float64) for z in (mu, s2, dmu, ds2)]
    val, grad, s, u, Phi, phi, bad = eubo_ref.closed_form(*f64)
    ev = np.linalg.eigvalsh(np.asarray(fit["K"], dtype=np.float64))
    return val, grad, dict(mu=f64[0], s2=f64[1], s=s, u=u, Phi=Phi, phi=phi, dmu=f64[2], ds2=f64[3], cond=ev[-1] / ev[0],
                           alpha=np.asarray(fit["alpha"], dtype=np.float64), bad=bad)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def draws_of_points(M, nd):
    return np.arange(M) % nd


def sets_of(Xs, q):
    """N_CAND sets of q of the candidates: option i of set m is candidate (m + 7 i) mod 40 (distinct within a set, and the
    near-duplicate pair never in one set: its two values differ by less than any margin)."""
    M = Xs.shape[1]
    return np.concatenate([Xs[:, (np.arange(M) + 7 * i) % M] for i in range(q)], axis=0)


def lines_of(Xs, anchored):
    """(lines, anchor): sliders from candidate m to candidate (m + 11) mod 40, or from the midpoint of candidates 5 and 6 (no
    candidate itself: that line would be one point q times over) to every candidate."""
    M = Xs.shape[1]
    if anchored:
        return np.asfortranarray(Xs), 0.5 * (Xs[:, 5] + Xs[:, 6])
    return np.concatenate([Xs, Xs[:, (np.arange(M) + 11) % M]], axis=0), None


def pairs_of(Xs):
    return np.concatenate([Xs[:, [p[0] for p in PAIRS]], Xs[:, [p[1] for p in PAIRS]]], axis=0)


def tolerances(ref):
    """tol_v / tol_g of test_eval_agrees_with_the_restatement (tests/test_gpu_path_sample.py; the tolerances() of test_gpu_qeubo.py
    and test_gpu_qnei.py are the same expressions) with this case's cond(K_y), |v| and shortest length scale.  ref: the float64
    reference."""
    ev = np.linalg.eigvalsh(np.asarray(ref.Ky, dtype=np.float64))
    cond = ev[-1] / ev[0]
    vs, a = float(np.abs(ref.v).max()), float(ref.a)
    tol_v = 1e-10 * a + 4 * cond * EPS * vs * a * np.sqrt(ref.N)
    tol_g = 1e-9 * a + 4 * cond * EPS * vs * a * np.sqrt(ref.N) / float(ref.ell.min())
    return float(tol_v), float(tol_g), float(cond)


def quantities(ref, Xs):
    """Everything a case compares, in ref's number type: gathered value and gradient with their two terms, every-draw values, v,
    the per-draw maximum over the training points, and per q the qEUBO and qNEI values, gradients, wins and gaps."""
    nd = ref.n_draws
    val, grad, parts = ref.eval(Xs, draws_of_points(Xs.shape[1], nd), parts=True)
    out = dict(parts, val=val, grad=grad, all=ref.eval_all(Xs), v=ref.v)
    t, arg, gap = nr.max_over_points(ref, ref.X)
    out.update(t=t, t_arg=arg, t_gap=gap)
    for q in QS:
        sets = sets_of(Xs, q)
        for name, res in (("qeubo", qr.qeubo(ref, sets, q)), ("qnei", nr.qnei(ref, sets, q, np.asarray(t, dtype=np.float64)))):
            out.update({f"{name}{q}_val": res[0], f"{name}{q}_grad": res[1], f"{name}{q}_wins": res[2], f"{name}{q}_gap": res[3]})
    return out


_CACHE = {}
# the normal stream of a case: SEED, except where that stream puts one candidate's value within the winner margin of a draw's
# baseline (a candidate sits in q of the 40 sets, so one such entry drops 40 % of the q = 16 sets: test_path_short_ref_cpu.py)
SEEDS = {(300, 33, 1e-8, 0, 5): SEED + 1}


def path_seed(N, D, case, kernel, nd=5):
    return SEEDS.get((N, D, case, kernel, nd), SEED)


def reference(N, D, case, kernel, nd=5):
    """One case, computed once per session and shared (callers must not modify it): gram_ref.problem, the float64 and the longdouble
    ShortPathRef (ref64, ref80), their quantities() at the 40 candidates (q64, q80), band (per quantity max |q64 - q80|), tol_v /
    tol_g / cond of tolerances(), tol (per quantity: the tolerance plus BAND_FACTOR bands) and kept (per selection: the boolean mask
    of the sets, or draws, whose winner leads by MARGIN_FACTOR every-draw value tolerances in the longdouble reference)."""
    key = (N, D, case, kernel, nd)
    if key in _CACHE:
        return _CACHE[key]
    p = gr.problem(N, D, case)
    r = dict(p, N=N, D=D, case=case, kernel=kernel, nd=nd, seed=path_seed(N, D, case, kernel, nd))
    for name, dt in (("64", np.float64), ("80", np.longdouble)):
        ref = ShortPathRef(p["X"], p["y"], p["theta"], p["b"], kernel, nd, F, r["seed"], dt)
        r["ref" + name], r["q" + name] = ref, quantities(ref, p["Xs"])
    r["tol_v"], r["tol_g"], r["cond"] = tolerances(r["ref64"])
    skip = ("wins", "gap", "arg")
    r["band"] = {k: float(np.abs(np.asarray(r["q64"][k], dtype=np.longdouble) - r["q80"][k]).max())
                 for k in r["q80"] if not k.endswith(skip)}
    r["tol"] = {k: (r["tol_g"] if "grad" in k else r["tol_v"]) + BAND_FACTOR * bk for k, bk in r["band"].items()}
    margin = MARGIN_FACTOR * r["tol"]["all"]
    r["margin"] = margin
    r["kept"] = {k[:-4]: np.asarray(r["q80"][k] >= margin) for k in r["q80"] if k.endswith("_gap")}
    _CACHE[key] = r
    return r


def eubo_reference(N, D, case, kernel):
    """The EUBO pairs of the case (PAIRS), cached like reference(): pairs, (val, grad, info) of eubo() on the float64 and on the
    longdouble fit (e64, e80), and band (val (M,), grad (2, M): per pair, and per option for the gradient)."""
    key = ("eubo", N, D, case, kernel)
    if key not in _CACHE:
        r = reference(N, D, case, kernel)
        pairs = pairs_of(r["Xs"])
        e64, e80 = eubo(r["ref64"].fit, pairs), eubo(r["ref80"].fit, pairs)
        dg = np.abs(e64[1] - e80[1])
        _CACHE[key] = dict(pairs=pairs, e64=e64, e80=e80,
                           band=dict(val=np.abs(e64[0] - e80[0]), grad=np.stack([dg[:D].max(axis=0), dg[D:].max(axis=0)])))
    return _CACHE[key]


def band(N, D, case, kernel, nd=5):
    """band[q] = max |ref64 - ref80| per quantity of the case."""
    return reference(N, D, case, kernel, nd)["band"]
