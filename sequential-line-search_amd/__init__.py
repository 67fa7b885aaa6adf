"""sequential-line-search_amd -- MI355X-native GP regression + acquisition maximisation.

This module is a thin ctypes binding of the C ABI in include/sls_hip.h (libsls_hip.so, hand-written
gfx950 HIP kernels).  It exists for the tests and bench.py; the product host layer is the C++ classes
under include/sequential-line-search/ + host/.  There is NO CPU fallback here: if the shared library is
missing or no GPU is present every call raises.

Array convention = the reference's Eigen layout: X has shape (D, N), one data point per column.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLS_HIP_LIB") or os.path.join(_HERE, "libsls_hip.so")   # SLS_HIP_LIB: A/B runs of another build

KERNEL_SE, KERNEL_MATERN52 = 0, 1
ACQ_EI, ACQ_UCB = 0, 1
ACQ_LOG_EI = 2   # log-space expected improvement (SLS_ACQ_LOG_EXPECTED_IMPROVEMENT); ucb_h is ignored
GP_K_Y, GP_K_Y_INV, GP_CHOL_L, GP_ALPHA, GP_MU_DATA = 0, 1, 2, 3, 4

_dp = C.POINTER(C.c_double)
_lib = None


class SlsError(RuntimeError):
    pass


class LbfgsOpts(C.Structure):
    """sls_lbfgs_opts (include/sls_hip.h).  struct_size is filled in here; the positional arguments are the option members."""
    _fields_ = [("struct_size", C.c_int), ("history", C.c_int), ("c1", C.c_double), ("shrink", C.c_double), ("gtol", C.c_double),
                ("max_backtracks", C.c_int), ("ftol_rel", C.c_double), ("xtol_rel", C.c_double)]

    def __init__(self, history=6, c1=1e-4, shrink=0.5, gtol=0.0, max_backtracks=20, ftol_rel=0.0, xtol_rel=0.0):
        super().__init__(C.sizeof(LbfgsOpts), history, c1, shrink, gtol, max_backtracks, ftol_rel, xtol_rel)


class _SubMapsStruct(C.Structure):
    """sls_submaps (include/sls_hip.h)."""
    _fields_ = [("struct_size", C.c_int), ("d", C.c_int), ("n_maps", C.c_int), ("A", _dp), ("c", _dp), ("map_of_column", C.POINTER(C.c_int))]


class SubMaps:
    """The maps of a *_sub call (sls_submaps): a column with map k stands for the point x = c[k] + A[k] @ z.  A is (n_maps, D, d) or
    (D, d), c is (n_maps, D) or (D,); map_of_column (one entry per point / start, None: every column uses map 0).  Nothing is
    checked here: the library refuses what the contract refuses."""

    def __init__(self, A, c, map_of_column=None):
        A, c = np.asarray(A, dtype=np.float64), np.asarray(c, dtype=np.float64)
        if A.ndim == 2:
            A, c = A[None], c.reshape(1, -1)
        assert A.ndim == 3 and c.shape == A.shape[:2], (A.shape, c.shape)
        self.n_maps, self.D, self.d = A.shape
        self.A, self.c = A, c
        # n_maps blocks of D x d, column-major: A_k[r + j*D]
        self._A = np.ascontiguousarray(A.transpose(0, 2, 1)).ravel()
        self._c = np.ascontiguousarray(c).ravel()
        self.map_of_column = None if map_of_column is None else np.ascontiguousarray(np.asarray(map_of_column, dtype=np.int32).ravel())

    def struct(self, **override):
        """The C struct (keeps this object's arrays alive only as long as this object lives); override: members for refusal tests."""
        moc = self.map_of_column
        s = _SubMapsStruct(C.sizeof(_SubMapsStruct), self.d, self.n_maps, _p(self._A), _p(self._c),
                           moc.ctypes.data_as(C.POINTER(C.c_int)) if moc is not None else None)
        for k, v in override.items():
            setattr(s, k, v)
        return s

    def subset(self, columns):
        """The same maps for a subset (or reordering) of the columns."""
        return SubMaps(self.A, self.c, None if self.map_of_column is None else self.map_of_column[np.asarray(columns)])


def _sub_struct(maps):
    return maps if isinstance(maps, _SubMapsStruct) else maps.struct()


def lib():
    """Load libsls_hip.so (raises if it has not been built -- see __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SlsError(f"{LIB_PATH} is missing: build it with `make -C sequential-line-search_amd/csrc` "
                           "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.sls_last_error.restype = C.c_char_p
    return _lib


EXPORTS = [
    "sls_last_error", "sls_version", "sls_ctx_create", "sls_ctx_destroy", "sls_ctx_set_stream", "sls_ctx_synchronize",
    "sls_ctx_set_candidate_chunk", "sls_gram", "sls_gram_cross", "sls_potrf", "sls_potrs", "sls_potri", "sls_gp_create",
    "sls_gp_destroy", "sls_gp_get_matrix", "sls_gp_get_summary", "sls_gp_predict", "sls_gp_predict_grad", "sls_acq_eval",
    "sls_lbfgs_default_opts", "sls_acq_maximize", "sls_acq_maximize_dev", "sls_gp_refit_dev", "sls_prof_enable",
    "sls_prof_reset", "sls_prof_get", "sls_nll_create", "sls_nll_destroy", "sls_nll_set_tolerances", "sls_nll_eval", "sls_gp_nll_grad", "sls_gp_nll_batch", "sls_multi_nll_create", "sls_multi_nll_destroy",
    "sls_multi_gp_nll_batch",
    "sls_pref_objective", "sls_pref_map_fit", "sls_gp_map_fit", "sls_gp_set_sigma_mode", "sls_acq_eval_pair", "sls_acq_maximize_pair", "sls_gp_append_point", "sls_acq_last_stats",
    "sls_multi_create", "sls_multi_destroy", "sls_multi_size", "sls_multi_exchange", "sls_multi_ctx", "sls_multi_gp_create", "sls_multi_gp_create_from",
    "sls_multi_gp_destroy", "sls_multi_gp_shard", "sls_multi_acq_maximize", "sls_multi_gp_predict", "sls_comm_unique_id", "sls_comm_create",
    "sls_comm_destroy", "sls_comm_allgather_best", "sls_device_trim_cache", "sls_tuning_reload", "sls_gp_generation",
    "sls_gp_predict_cov", "sls_gp_sample_posterior", "sls_random_normal",
    "sls_path_create", "sls_path_destroy", "sls_path_eval", "sls_path_maximize",
    "sls_mes_terms", "sls_mes_eval", "sls_mes_maximize", "sls_logei_terms",
    "sls_eubo_eval", "sls_eubo_maximize", "sls_qeubo_eval", "sls_qeubo_maximize",
    "sls_path_max_over_points", "sls_qnei_eval", "sls_qnei_maximize",
    "sls_line_eval", "sls_line_maximize", "sls_patch_eval", "sls_patch_maximize",
    "sls_qlognei_terms", "sls_qlognei_eval", "sls_qlognei_maximize", "sls_qbald_eval", "sls_qbald_maximize",
    "sls_acq_eval_sub", "sls_acq_maximize_sub", "sls_mes_eval_sub", "sls_mes_maximize_sub", "sls_path_eval_sub", "sls_path_maximize_sub",
    "sls_nll_loo", "sls_gp_loo_grad", "sls_gp_loo",
    "sls_jes_create", "sls_jes_destroy", "sls_jes_optima", "sls_jes_terms", "sls_jes_eval", "sls_jes_maximize",
    "sls_kg_create", "sls_kg_destroy", "sls_kg_points", "sls_kg_eval", "sls_kg_maximize", "sls_kg_lines",
    "sls_gp_set_laplace", "sls_gp_clear_laplace", "sls_gp_laplace_get", "sls_gp_laplace_summary",
]


def tuning_reload():
    """Re-read the SLS_* environment variables (the library parses them once per process)."""
    lib().sls_tuning_reload()


ERR_INVALID = -1
ERR_UNSUPPORTED = -5
# selectors of GP.laplace_matrix (SLS_LAPLACE_*)
LAPLACE_W, LAPLACE_COV, LAPLACE_M = 0, 1, 2
SIGMA_EXPLICIT_INVERSE, SIGMA_CHOLESKY_SOLVE = 0, 1


class Unsupported(SlsError):
    """SLS_ERR_UNSUPPORTED: the problem is outside what the entry point runs on the device (use the general path)."""


def _ck(rc):
    if rc != 0:
        # SLS_ERR_UNSUPPORTED has a class of its own (a subclass: callers that catch SlsError see no difference)
        err = (Unsupported if rc == ERR_UNSUPPORTED else SlsError)(f"libsls_hip error {rc}: {lib().sls_last_error().decode()}")
        err.code = rc
        raise err


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(_dp)


def _eval_call(call, block, rows, want_grad, *extras):
    """call(block, M, val, grad, *extras) at the M columns of block: values (M,), then with want_grad the gradient (rows, M), then
    those of `extras` (further output arrays of the call; None: not asked for) that were asked for.  The values alone are not a tuple."""
    M = block.shape[1]
    val = np.empty(M)
    grad = np.empty((rows, M), order="F") if want_grad else None
    _ck(call(_p(block), M, _p(val), _p(grad) if want_grad else None,
             *(None if e is None else e.ctypes.data_as(C.c_void_p) for e in extras)))
    out = (val,) + tuple(a for a in (grad,) + extras if a is not None)
    return out if len(out) > 1 else val


def _maximize_call(call, block, rows, n_local, offset, want_all, opts):
    """call(starts, S, n_local, opts, offset, x, value, index, x_stars, y_stars) from the S columns of block (rows x S)."""
    S = block.shape[1]
    x, val, idx = np.empty(rows), C.c_double(), C.c_long()
    xs = np.empty((rows, S), order="F") if want_all else None
    ys = np.empty(S) if want_all else None
    _ck(call(_p(block), S, int(n_local), C.byref(opts) if opts is not None else None, C.c_long(offset), _p(x), C.byref(val),
             C.byref(idx), _p(xs) if want_all else None, _p(ys) if want_all else None))
    return dict(index=idx.value, x=x, value=val.value, x_stars=xs, y_stars=ys)


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._gps = []
        _ck(lib().sls_ctx_create(int(device), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            for ref in self._gps:          # handles must not outlive their context
                gp = ref()
                if gp is not None:
                    gp.close()
            self._gps = []
            lib().sls_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _ck(lib().sls_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        _ck(lib().sls_ctx_synchronize(self.h))

    def set_candidate_chunk(self, chunk):
        _ck(lib().sls_ctx_set_candidate_chunk(self.h, int(chunk)))

    def prof_enable(self, on=True):
        _ck(lib().sls_prof_enable(self.h, int(on)))

    def prof_reset(self):
        _ck(lib().sls_prof_reset(self.h))

    def prof_get(self, name):
        ms, n = C.c_double(), C.c_long()
        _ck(lib().sls_prof_get(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def random_normal(self, seed, offset, n):
        """Standard normal numbers offset .. offset + n - 1 of stream `seed` (Philox4x64-10 + Box-Muller, sls_random_normal)."""
        out = np.empty(int(n))
        _ck(lib().sls_random_normal(self.h, C.c_ulonglong(int(seed)), C.c_long(int(offset)), C.c_long(int(n)),
                                    _p(out) if n > 0 else None))
        return out

    def mes_terms(self, t):
        """(g(t), g'(t)) of max-value entropy search for an array of t (sls_mes_terms)."""
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
        g, dg = np.empty(t.size), np.empty(t.size)
        _ck(lib().sls_mes_terms(self.h, _p(t), C.c_long(t.size), _p(g), _p(dg)))
        return g, dg

    def jes_terms(self, t):
        """(tau(t), tau'(t)) of joint entropy search, the variance factor of a unit normal truncated above at t and its derivative, for
        an array of t (sls_jes_terms)."""
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
        tau, dtau = np.empty(t.size), np.empty(t.size)
        _ck(lib().sls_jes_terms(self.h, _p(t), C.c_long(t.size), _p(tau), _p(dtau)))
        return tau, dtau

    def kg_lines(self, a, B, a_self=None, b_self=None, want_beta=True, want_prob=True):
        """The knowledge-gradient combiner alone on caller-supplied lines (sls_kg_lines): intercepts a (K,), slopes B (M, K), optionally
        one own line per candidate (a_self, b_self (M,)).  Returns val (M,), then with want_beta beta (M, K), then with want_prob pi
        (M, K), then with a self line (beta_K, pi_K) as an (M, 2) array."""
        a, B = _f(a).ravel(), _f(B)
        if B.ndim != 2 or B.shape[1] != a.size:
            raise SlsError(f"kg_lines: B must be M x K = M x {a.size}, got {B.shape}")
        M, K = B.shape
        own = a_self is not None
        if own:
            a_self, b_self = _f(a_self).ravel(), _f(b_self).ravel()
            if a_self.size != M or b_self.size != M:
                raise SlsError(f"kg_lines: a_self and b_self must have M = {M} entries")
        val = np.empty(M)
        beta = np.empty((M, K), order="F") if want_beta else None
        prob = np.empty((M, K), order="F") if want_prob else None
        so = np.empty((M, 2), order="F") if own else None
        _ck(lib().sls_kg_lines(self.h, _p(a), _p(B), _p(a_self) if own else None, _p(b_self) if own else None, K, M, _p(val),
                               _p(beta) if want_beta else None, _p(prob) if want_prob else None, _p(so) if own else None))
        return (val,) + ((beta,) if want_beta else ()) + ((prob,) if want_prob else ()) + ((so,) if own else ())

    def logei_terms(self, u):
        """(log h(u), Phi/h, phi/h) of log expected improvement, h = phi + u Phi, for an array of u (sls_logei_terms)."""
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).ravel())
        log_h, b1, b2 = np.empty(u.size), np.empty(u.size), np.empty(u.size)
        _ck(lib().sls_logei_terms(self.h, _p(u), C.c_long(u.size), _p(log_h), _p(b1), _p(b2)))
        return log_h, b1, b2

    def qlognei_terms(self, a):
        """(L(a), R(a)) = (log softplus(a), its derivative) of log-space noisy expected improvement for an array of a
        (sls_qlognei_terms)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
        L, R = np.empty(a.size), np.empty(a.size)
        _ck(lib().sls_qlognei_terms(self.h, _p(a), C.c_long(a.size), _p(L), _p(R)))
        return L, R

    # ---- free functions (src/regressor.cpp) ----
    def gram(self, X, theta, b, kernel):
        X, theta = _f(X), _f(theta)
        D, N = X.shape
        K = np.empty((N, N), order="F")
        _ck(lib().sls_gram(self.h, _p(X), D, N, _p(theta), C.c_double(b), int(kernel), _p(K)))
        return K

    def gram_cross(self, X, Xs, theta, kernel):
        X, Xs, theta = _f(X), _f(Xs), _f(theta)
        D, N = X.shape
        M = Xs.shape[1]
        Ks = np.empty((N, M), order="F")
        _ck(lib().sls_gram_cross(self.h, _p(X), D, N, _p(Xs), M, _p(theta), int(kernel), _p(Ks)))
        return Ks

    def potrf(self, A):
        A = _f(A).copy(order="F")
        _ck(lib().sls_potrf(self.h, _p(A), A.shape[0]))
        return A

    def potrs(self, L, B):
        L = _f(L)
        B = _f(B).copy(order="F")
        nrhs = 1 if B.ndim == 1 else B.shape[1]
        _ck(lib().sls_potrs(self.h, _p(L), L.shape[0], _p(B), nrhs))
        return B

    def potri(self, L):
        L = _f(L)
        out = np.empty_like(L, order="F")
        _ck(lib().sls_potri(self.h, _p(L), L.shape[0], _p(out)))
        return out


class GP:
    """Device-resident GP state (GaussianProcessRegressor with fixed hyper-parameters / PreferenceRegressor post-MAP)."""

    def __init__(self, ctx, X, y, theta, b, kernel=KERNEL_MATERN52):
        self.ctx = ctx
        X, y, theta = _f(X), _f(y), _f(theta)
        self.D, self.N = X.shape
        assert y.shape == (self.N,) and theta.shape == (self.D + 1,)
        self.h = C.c_void_p()
        _ck(lib().sls_gp_create(ctx.h, _p(X), self.D, self.N, _p(y), _p(theta), C.c_double(b), int(kernel), C.byref(self.h)))
        ctx._gps.append(weakref.ref(self))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_gp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sigma_mode(self, mode):
        """SIGMA_EXPLICIT_INVERSE (GaussianProcessRegressor, default) or SIGMA_CHOLESKY_SOLVE (PreferenceRegressor)."""
        _ck(lib().sls_gp_set_sigma_mode(self.h, int(mode)))

    def generation(self):
        """A number that changes whenever the predictor behind the handle changes (fit, refit, appended point, sigma mode)."""
        g = C.c_long(0)
        _ck(lib().sls_gp_generation(self.h, C.byref(g)))
        return int(g.value)

    def set_laplace(self, prefs, btl_scale=0.01):
        """Laplace posterior of the goodness values at the handle's y (sls_gp_set_laplace): prefs is a sequence of index tuples, the
        first index of a tuple the chosen point.  From here on every sigma route of the handle returns the Laplace variance and the
        fit is frozen (set_sigma_mode, append_point, refit_dev raise Unsupported) until clear_laplace()."""
        flat = np.array([i for p in prefs for i in p], dtype=np.uint32)
        offs = np.zeros(len(prefs) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in prefs])
        _ck(lib().sls_gp_set_laplace(self.h, flat.ctypes.data_as(C.POINTER(C.c_uint)), offs.ctypes.data_as(C.POINTER(C.c_int)),
                                     len(prefs), C.c_double(btl_scale)))

    def clear_laplace(self):
        """Back to the plain handle: every call returns the bits it returned before set_laplace."""
        _ck(lib().sls_gp_clear_laplace(self.h))

    def laplace_matrix(self, what):
        """LAPLACE_W (the BTL Hessian), LAPLACE_COV (Sigma_g, the posterior covariance of the goodness values) or LAPLACE_M (the
        effective inverse that stands in the place of K_y^-1): N x N each."""
        out = np.empty((self.N, self.N), order="F")
        _ck(lib().sls_gp_laplace_get(self.h, int(what), _p(out)))
        return out

    def laplace_summary(self):
        """dict(log_lik, logdet_B, log_evidence): sum_t log p_t0, log|I + L^T W L| and log Z = log_lik - y.alpha / 2 - log|B| / 2."""
        ll, ld, ev = C.c_double(), C.c_double(), C.c_double()
        _ck(lib().sls_gp_laplace_summary(self.h, C.byref(ll), C.byref(ld), C.byref(ev)))
        return dict(log_lik=ll.value, logdet_B=ld.value, log_evidence=ev.value)

    def append_point(self, x, y):
        x = _f(x)
        assert x.shape == (self.D,)
        _ck(lib().sls_gp_append_point(self.h, _p(x), C.c_double(y)))
        self.N += 1

    def loo(self):
        """Leave-one-out predictions (mu, variance, log density; N each) at the handle's own hyper-parameters and data (sls_gp_loo)."""
        mu, var, logp = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        _ck(lib().sls_gp_loo(self.h, _p(mu), _p(var), _p(logp)))
        return mu, var, logp

    def matrix(self, what):
        out = np.empty((self.N, self.N), order="F") if what in (GP_K_Y, GP_K_Y_INV, GP_CHOL_L) else np.empty(self.N)
        _ck(lib().sls_gp_get_matrix(self.h, int(what), _p(out)))
        return out

    def summary(self):
        bi, mb, ld = C.c_int(), C.c_double(), C.c_double()
        _ck(lib().sls_gp_get_summary(self.h, C.byref(bi), C.byref(mb), C.byref(ld)))
        return dict(best_index=bi.value, mu_best=mb.value, logdet=ld.value)

    def predict(self, Xs):
        Xs = _f(Xs)
        M = Xs.shape[1]
        mu, sg = np.empty(M), np.empty(M)
        _ck(lib().sls_gp_predict(self.h, _p(Xs), M, _p(mu), _p(sg)))
        return mu, sg

    def predict_cov(self, Xs):
        """Joint posterior of the latent function at the columns of Xs (D x M): (mu (M,), cov (M, M)), sls_gp_predict_cov."""
        Xs = _f(Xs)
        M = Xs.shape[1]
        mu, cov = np.empty(M), np.empty((M, M), order="F")
        _ck(lib().sls_gp_predict_cov(self.h, _p(Xs), M, _p(mu), _p(cov)))
        return mu, cov

    def sample_posterior(self, Xs, n_samples, seed):
        """n_samples draws of the latent function at the columns of Xs: (F (M, n_samples), jitter), sls_gp_sample_posterior."""
        Xs = _f(Xs)
        M = Xs.shape[1]
        F = np.empty((M, int(n_samples)), order="F")
        jit = C.c_double(0.0)
        _ck(lib().sls_gp_sample_posterior(self.h, _p(Xs), M, int(n_samples), C.c_ulonglong(int(seed)), _p(F), C.byref(jit)))
        return F, jit.value

    def predict_grad(self, Xs):
        Xs = _f(Xs)
        M = Xs.shape[1]
        dm, ds = np.empty((self.D, M), order="F"), np.empty((self.D, M), order="F")
        _ck(lib().sls_gp_predict_grad(self.h, _p(Xs), M, _p(dm), _p(ds)))
        return dm, ds

    def acq_eval(self, Xs, acq=ACQ_EI, ucb_h=1.0, want_grad=True):
        return _eval_call(lambda *a: lib().sls_acq_eval(self.h, int(acq), C.c_double(ucb_h), *a), _f(Xs), self.D, want_grad)

    def acq_maximize(self, starts, n_local, acq=ACQ_EI, ucb_h=1.0, offset=0, want_all=True, opts=None):
        return _maximize_call(lambda *a: lib().sls_acq_maximize(self.h, int(acq), C.c_double(ucb_h), *a), _f(starts), self.D, n_local,
                              offset, want_all, opts)

    def acq_eval_pair(self, sigma_gp, Xs, acq=ACQ_EI, ucb_h=1.0, want_grad=True):
        """objective_for_multiple_points: mean (and mu+) from this handle, deviation from `sigma_gp`."""
        return _eval_call(lambda *a: lib().sls_acq_eval_pair(self.h, sigma_gp.h, int(acq), C.c_double(ucb_h), *a), _f(Xs), self.D,
                          want_grad)

    def acq_maximize_pair(self, sigma_gp, starts, n_local, acq=ACQ_EI, ucb_h=1.0):
        starts = _f(starts)
        x, val, idx = np.empty(self.D), C.c_double(), C.c_long()
        _ck(lib().sls_acq_maximize_pair(self.h, sigma_gp.h, int(acq), C.c_double(ucb_h), _p(starts), starts.shape[1], int(n_local),
                                        None, _p(x), C.byref(val), C.byref(idx)))
        return dict(index=idx.value, x=x, value=val.value)

    def acq_maximize_dev(self, starts_dev_ptr, S, n_local, acq=ACQ_EI, ucb_h=1.0, offset=0, opts=None):
        x, val, idx = np.empty(self.D), C.c_double(), C.c_long()
        _ck(lib().sls_acq_maximize_dev(self.h, int(acq), C.c_double(ucb_h), C.c_void_p(starts_dev_ptr), int(S), int(n_local),
                                       C.byref(opts) if opts is not None else None, C.c_long(offset), _p(x), C.byref(val),
                                       C.byref(idx)))
        return dict(index=idx.value, x=x, value=val.value)

    def mes_eval(self, y_star, Xs, want_grad=True):
        """Max-value entropy search at the columns of Xs on the samples y_star of the maximum value (sls_mes_eval)."""
        y_star = _f(y_star).ravel()
        return _eval_call(lambda *a: lib().sls_mes_eval(self.h, _p(y_star), y_star.size, *a), _f(Xs), self.D, want_grad)

    def mes_maximize(self, y_star, starts, n_local, offset=0, want_all=True, opts=None):
        """acq_maximize with max-value entropy search on the samples y_star as the objective (sls_mes_maximize)."""
        y_star = _f(y_star).ravel()
        return _maximize_call(lambda *a: lib().sls_mes_maximize(self.h, _p(y_star), y_star.size, *a), _f(starts), self.D, n_local, offset,
                              want_all, opts)

    def jes_create(self, x_star, f_star, star_noise=0.0):
        """The snapshot of K sampled optima (x_star (D, K), f_star (K,)) joint entropy search conditions on (sls_jes_create)."""
        return JesOptima(self, x_star, f_star, star_noise)

    def kg_create(self, x_ref):
        """The snapshot of K fixed points (x_ref (D, K)) the knowledge gradient maximises the future mean over (sls_kg_create)."""
        return KnowledgeGradient(self, x_ref)

    def eubo_eval(self, pairs, want_grad=True):
        """Expected utility of the best option E[max(f(x), f(x'))] at the columns of pairs (2D x M: rows 0..D-1 = x, D..2D-1 = x'),
        sls_eubo_eval; the gradient is 2D x M in the same row order."""
        pairs = _f(pairs)
        if pairs.ndim != 2 or pairs.shape[0] != 2 * self.D:
            raise SlsError(f"eubo_eval: pairs must be 2D x M = {2 * self.D} x M, got {pairs.shape}")
        return _eval_call(lambda *a: lib().sls_eubo_eval(self.h, *a), pairs, 2 * self.D, want_grad)

    def eubo_maximize(self, starts, n_local, offset=0, want_all=True, opts=None):
        """acq_maximize over [0,1]^(2D) with the pair objective of eubo_eval (sls_eubo_maximize): starts 2D x S, x and x_stars have
        2D rows."""
        starts = _f(starts)
        if starts.ndim != 2 or starts.shape[0] != 2 * self.D:
            raise SlsError(f"eubo_maximize: starts must be 2D x S = {2 * self.D} x S, got {starts.shape}")
        return _maximize_call(lambda *a: lib().sls_eubo_maximize(self.h, *a), starts, 2 * self.D, n_local, offset, want_all, opts)

    # ---- maximisation over affine subspaces (sls_*_sub): maps is a SubMaps (or its C struct), Z / starts_z are d x M / d x S
    def _eval_sub(self, call, maps, Z, want_grad, want_x):
        s = _sub_struct(maps)
        Z = _f(Z)
        X = np.empty((self.D, Z.shape[1]), order="F") if want_x else None
        return _eval_call(lambda *a: call(C.byref(s), *a), Z, max(1, s.d), want_grad, X)

    def _maximize_sub(self, call, maps, starts_z, n_local, offset, want_all, opts):
        s = _sub_struct(maps)
        starts_z = _f(starts_z)
        rows, S = max(1, s.d), starts_z.shape[1]
        z, x, val, idx = np.empty(rows), np.empty(self.D), C.c_double(), C.c_long()
        zs = np.empty((rows, S), order="F") if want_all else None
        xs = np.empty((self.D, S), order="F") if want_all else None
        ys = np.empty(S) if want_all else None
        _ck(call(C.byref(s), _p(starts_z), S, int(n_local), C.byref(opts) if opts is not None else None, C.c_long(offset), _p(z), _p(x),
                 C.byref(val), C.byref(idx), _p(zs) if want_all else None, _p(xs) if want_all else None, _p(ys) if want_all else None))
        return dict(index=idx.value, z=z, x=x, value=val.value, z_stars=zs, x_stars=xs, y_stars=ys)

    def acq_eval_sub(self, maps, Z, acq=ACQ_EI, ucb_h=1.0, want_grad=True, want_x=False):
        """acq_eval at x = c + A z (sls_acq_eval_sub): values (M,), then with want_grad the gradient in z (d, M), then with want_x the
        expanded points (D, M)."""
        return self._eval_sub(lambda *a: lib().sls_acq_eval_sub(self.h, int(acq), C.c_double(ucb_h), *a), maps, Z, want_grad, want_x)

    def acq_maximize_sub(self, maps, starts_z, n_local, acq=ACQ_EI, ucb_h=1.0, offset=0, want_all=True, opts=None):
        """acq_maximize over z in [0,1]^d with x = c + A z (sls_acq_maximize_sub): z / x of the winner, z_stars (d, S) / x_stars (D, S) /
        y_stars of every start."""
        return self._maximize_sub(lambda *a: lib().sls_acq_maximize_sub(self.h, int(acq), C.c_double(ucb_h), *a), maps, starts_z, n_local,
                                  offset, want_all, opts)

    def mes_eval_sub(self, y_star, maps, Z, want_grad=True, want_x=False):
        """mes_eval at x = c + A z (sls_mes_eval_sub)."""
        y_star = _f(y_star).ravel()
        return self._eval_sub(lambda *a: lib().sls_mes_eval_sub(self.h, _p(y_star), y_star.size, *a), maps, Z, want_grad, want_x)

    def mes_maximize_sub(self, y_star, maps, starts_z, n_local, offset=0, want_all=True, opts=None):
        """mes_maximize over z in [0,1]^d with x = c + A z (sls_mes_maximize_sub)."""
        y_star = _f(y_star).ravel()
        return self._maximize_sub(lambda *a: lib().sls_mes_maximize_sub(self.h, _p(y_star), y_star.size, *a), maps, starts_z, n_local,
                                  offset, want_all, opts)

    def last_stats(self):
        """Evaluation counts of the last acq_maximize* call (sls_acq_last_stats)."""
        issued, cap, rounds, live = C.c_long(), C.c_long(), C.c_int(), C.c_int()
        _ck(lib().sls_acq_last_stats(self.h, C.byref(issued), C.byref(cap), C.byref(rounds), C.byref(live)))
        return dict(evals_issued=issued.value, evals_cap=cap.value, rounds=rounds.value, live_at_end=live.value)

    def refit_dev(self, X_dev_ptr, y_dev_ptr):
        _ck(lib().sls_gp_refit_dev(self.h, C.c_void_p(X_dev_ptr), C.c_void_p(y_dev_ptr)))


JES_MAX_OPTIMA = 1024     # SLS_JES_MAX_OPTIMA


class JesOptima:
    """K sampled optima (x*_k, f*_k) of a fitted GP handle, conditioned on for joint entropy search (sls_jes_*).  A snapshot: after
    the handle is refitted, grown or switched in sigma mode every call is refused; it must be closed before its handle."""

    def __init__(self, gp, x_star, f_star, star_noise=0.0):
        x_star, f_star = _f(x_star), _f(f_star).ravel()
        if x_star.ndim != 2 or x_star.shape != (gp.D, f_star.size):
            raise SlsError(f"JesOptima: x_star must be D x K = {gp.D} x {f_star.size}, got {x_star.shape}")
        self.gp, self.D, self.K = gp, gp.D, f_star.size
        self.h = C.c_void_p()
        _ck(lib().sls_jes_create(gp.h, _p(x_star), _p(f_star), self.K, C.c_double(star_noise), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_jes_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optima(self):
        """(mu*_k, v_k): the posterior mean at the optima and the variance they are conditioned with."""
        mu, v = np.empty(self.K), np.empty(self.K)
        _ck(lib().sls_jes_optima(self.h, _p(mu), _p(v)))
        return mu, v

    def eval(self, Xs, noise_var, want_grad=True, want_cov=False):
        """alpha at the columns of Xs: values (M,), then with want_grad the gradient (D, M), then with want_cov the posterior
        covariances c_k(x_m) (M, K)."""
        Xs = _f(Xs)
        cov = np.empty((Xs.shape[1], self.K), order="F") if want_cov else None
        return _eval_call(lambda *a: lib().sls_jes_eval(self.h, C.c_double(noise_var), *a), Xs, self.D, want_grad, cov)

    def maximize(self, starts, n_local, noise_var, offset=0, want_all=True, opts=None):
        """acq_maximize with joint entropy search as the objective (sls_jes_maximize)."""
        return _maximize_call(lambda *a: lib().sls_jes_maximize(self.h, C.c_double(noise_var), *a), _f(starts), self.D, n_local, offset,
                              want_all, opts)


KG_MAX_POINTS = 1024      # SLS_KG_MAX_POINTS


class KnowledgeGradient:
    """K fixed points x_k of a fitted GP handle for the knowledge gradient on a discrete set (sls_kg_*).  A snapshot: after the handle
    is refitted, grown or switched in sigma mode every call is refused; it must be closed before its handle."""

    def __init__(self, gp, x_ref):
        x_ref = _f(x_ref)
        if x_ref.ndim != 2 or x_ref.shape[0] != gp.D:
            raise SlsError(f"KnowledgeGradient: x_ref must be D x K = {gp.D} x K, got {x_ref.shape}")
        self.gp, self.D, self.K = gp, gp.D, x_ref.shape[1]
        self.h = C.c_void_p()
        _ck(lib().sls_kg_create(gp.h, _p(x_ref), self.K, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_kg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points(self):
        """(a_k, a_max, arg max): the posterior mean at the points, its maximum and the (lowest) index of the maximum."""
        mu, mx, am = np.empty(self.K), C.c_double(), C.c_int()
        _ck(lib().sls_kg_points(self.h, _p(mu), C.byref(mx), C.byref(am)))
        return mu, mx.value, am.value

    def eval(self, Xs, noise_var, include_self=True, want_grad=False, want_slopes=False):
        """KG at the columns of Xs: values (M,), then with want_grad the gradient (D, M), then with want_slopes the slopes b_k(x_m)
        (M, K)."""
        Xs = _f(Xs)
        slope = np.empty((Xs.shape[1], self.K), order="F") if want_slopes else None
        return _eval_call(lambda *a: lib().sls_kg_eval(self.h, C.c_double(noise_var), int(bool(include_self)), *a), Xs, self.D, want_grad,
                          slope)

    def maximize(self, starts, n_local, noise_var, include_self=True, offset=0, want_all=True, opts=None):
        """acq_maximize with the knowledge gradient as the objective (sls_kg_maximize)."""
        return _maximize_call(lambda *a: lib().sls_kg_maximize(self.h, C.c_double(noise_var), int(bool(include_self)), *a), _f(starts),
                              self.D, n_local, offset, want_all, opts)


QEUBO_MAX_OPTIONS = 16   # SLS_QEUBO_MAX_OPTIONS
LINE_MIN_POSITIONS = 2   # SLS_LINE_MIN_POSITIONS
PATCH_MIN_POSITIONS = 2  # SLS_PATCH_MIN_POSITIONS
QEUBO_FLOOR = -1.0e300   # SLS_QEUBO_FLOOR
QLOGNEI_TAU_RELU, QLOGNEI_TAU_MAX = 1e-6, 1e-2   # SLS_QLOGNEI_TAU_RELU, SLS_QLOGNEI_TAU_MAX
QBALD_SCALE = 0.010      # SLS_QBALD_SCALE: the reference's default btl_scale


class PathSamples:
    """n_draws pathwise posterior function draws of a fitted GP handle (sls_path_*): F = n_freq shared random frequencies, normal
    stream `seed`.  A draw can be evaluated anywhere and maximised over [0,1]^D (Thompson sampling)."""

    def __init__(self, gp, n_draws, n_freq=2048, seed=0):
        self.gp, self.D, self.n_draws, self.n_freq = gp, gp.D, int(n_draws), int(n_freq)
        self.h = C.c_void_p()
        _ck(lib().sls_path_create(gp.h, self.n_draws, self.n_freq, C.c_ulonglong(int(seed)), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_path_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, Xs, draw_of_point, want_grad=True):
        """f_{draw_of_point[m]}(Xs[:, m]): values (M,) and, with want_grad, gradients (D, M)."""
        Xs = _f(Xs)
        M = Xs.shape[1]
        dr = np.ascontiguousarray(np.asarray(draw_of_point, dtype=np.int32))
        assert dr.shape == (M,)
        val = np.empty(M)
        grad = np.empty((self.D, M), order="F") if want_grad else None
        _ck(lib().sls_path_eval(self.h, _p(Xs), M, dr.ctypes.data_as(C.POINTER(C.c_int)), _p(val), _p(grad) if want_grad else None))
        return (val, grad) if want_grad else val

    def eval_all(self, Xs):
        """Every draw at every column of Xs: (M, n_draws)."""
        Xs = _f(Xs)
        M = Xs.shape[1]
        val = np.empty((M, self.n_draws), order="F")
        _ck(lib().sls_path_eval(self.h, _p(Xs), M, None, _p(val), None))
        return val

    def maximize(self, starts, n_local, opts=None):
        """starts (D, n_draws * S), columns [s S, (s + 1) S) for draw s: per draw (x (D, n_draws), value (n_draws,), start index
        within the draw (n_draws,))."""
        starts = _f(starts)
        T = starts.shape[1]
        assert T % self.n_draws == 0
        S = T // self.n_draws
        x = np.empty((self.D, self.n_draws), order="F")
        val = np.empty(self.n_draws)
        idx = np.empty(self.n_draws, dtype=np.int64)
        _ck(lib().sls_path_maximize(self.h, _p(starts), S, int(n_local), C.byref(opts) if opts is not None else None, _p(x), _p(val),
                                    idx.ctypes.data_as(C.POINTER(C.c_long))))
        return dict(x=x, value=val, index=idx)

    def eval_sub(self, maps, Z, draw_of_point, want_grad=True, want_x=False):
        """eval at x = c + A z (sls_path_eval_sub): values (M,), then with want_grad the gradient in z (d, M), then with want_x the
        expanded points (D, M)."""
        Z = _f(Z)
        dr = None if draw_of_point is None else np.ascontiguousarray(np.asarray(draw_of_point, dtype=np.int32))
        assert dr is None or dr.shape == (Z.shape[1],)
        drp = dr.ctypes.data_as(C.POINTER(C.c_int)) if dr is not None else None
        return self.gp._eval_sub(lambda s, z, M, *out: lib().sls_path_eval_sub(self.h, s, z, M, drp, *out), maps, Z, want_grad, want_x)

    def maximize_sub(self, maps, starts_z, n_local, opts=None):
        """maximize over z in [0,1]^d with x = c + A z (sls_path_maximize_sub): starts_z (d, n_draws * S), columns [s S, (s + 1) S) for
        draw s; per draw z (d, n_draws), x (D, n_draws), value and the start index within the draw."""
        s = _sub_struct(maps)
        starts_z = _f(starts_z)
        T = starts_z.shape[1]
        assert T % self.n_draws == 0
        rows = max(1, s.d)
        z = np.empty((rows, self.n_draws), order="F")
        x = np.empty((self.D, self.n_draws), order="F")
        val = np.empty(self.n_draws)
        idx = np.empty(self.n_draws, dtype=np.int64)
        _ck(lib().sls_path_maximize_sub(self.h, C.byref(s), _p(starts_z), T // self.n_draws, int(n_local),
                                        C.byref(opts) if opts is not None else None, _p(z), _p(x), _p(val),
                                        idx.ctypes.data_as(C.POINTER(C.c_long))))
        return dict(z=z, x=x, value=val, index=idx)

    # ---- the set-shaped objectives (sls_qeubo_*, sls_qnei_*, sls_qlognei_*, sls_line_*, sls_patch_*): one body per kind of call
    def _set_block(self, who, q, block, what, qmin=1):
        """q within its range and, for a block of sets (block None: the range alone), its qD rows."""
        q = int(q)
        if not qmin <= q <= QEUBO_MAX_OPTIONS:
            raise SlsError(f"{who}: q = {q} ({qmin} .. {QEUBO_MAX_OPTIONS})")
        if block is not None and (block.ndim != 2 or block.shape[0] != q * self.D):
            n = "M" if what == "sets" else "S"
            raise SlsError(f"{who}: {what} must be qD x {n} = {q * self.D} x {n}, got {block.shape}")
        return q

    def _set_eval(self, call, rows, q, block, want_grad, want_wins, *lead_args, grid=None):
        """call(h, q, *lead_args, block, M, val, grad, wins) at the M columns of block (with grid = (qs, qt) in the place of q = qs qt):
        values (M,), then with want_grad the gradient (rows, M), then with want_wins the win counts (q, M) int32."""
        wins = np.zeros((q, block.shape[1]), dtype=np.int32, order="F") if want_wins else None
        return _eval_call(lambda *a: call(self.h, *(grid or (q,)), *lead_args, *a), block, rows, want_grad, wins)

    def _set_maximize(self, call, rows, block, n_local, offset, want_all, opts, *lead_args):
        """call(h, *lead_args, starts, S, n_local, opts, offset, x, value, index, x_stars, y_stars) from the S columns of block."""
        return _maximize_call(lambda *a: call(self.h, *lead_args, *a), block, rows, n_local, offset, want_all, opts)

    def qeubo_eval(self, sets, q, want_grad=True, want_wins=False):
        """Expected utility of the best of q options on the draws (sls_qeubo_eval) at the columns of sets (qD x M: rows iD..iD+D-1 =
        option i): values (M,), then with want_grad the gradient (qD, M), then with want_wins the win counts (q, M) int32."""
        sets = _f(sets)
        q = self._set_block("qeubo_eval", q, sets, "sets")
        return self._set_eval(lib().sls_qeubo_eval, q * self.D, q, sets, want_grad, want_wins)

    def qeubo_maximize(self, starts, q, n_local, offset=0, want_all=True, opts=None):
        """acq_maximize over [0,1]^(qD) with the set objective of qeubo_eval (sls_qeubo_maximize): starts qD x S, x and x_stars have
        qD rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        q = self._set_block("qeubo_maximize", q, starts, "starts")
        return self._set_maximize(lib().sls_qeubo_maximize, q * self.D, starts, n_local, offset, want_all, opts, q)

    def max_over_points(self, Xb):
        """Per draw, the maximum over the columns of Xb (D x Mb, Mb >= 1) and the lowest column that attains it
        (sls_path_max_over_points): (t (n_draws,), arg (n_draws,) int32).  A NaN among a draw's values gives (NaN, -1)."""
        Xb = _f(Xb)
        if Xb.ndim != 2 or Xb.shape[0] != self.D or Xb.shape[1] < 1:
            raise SlsError(f"max_over_points: Xb must be D x Mb = {self.D} x Mb with Mb >= 1, got {Xb.shape}")
        t = np.empty(self.n_draws)
        arg = np.empty(self.n_draws, dtype=np.int32)
        _ck(lib().sls_path_max_over_points(self.h, _p(Xb), Xb.shape[1], _p(t), arg.ctypes.data_as(C.POINTER(C.c_int))))
        return t, arg

    def _baseline(self, who, baseline):
        t = np.ascontiguousarray(np.asarray(baseline, dtype=np.float64))
        if t.shape != (self.n_draws,):
            raise SlsError(f"{who}: baseline must hold n_draws = {self.n_draws} values, got shape {t.shape}")
        return t

    def qnei_eval(self, sets, q, baseline, want_grad=True, want_wins=False):
        """Noisy expected improvement of q points on the draws over the per-draw baseline (sls_qnei_eval) at the columns of sets (qD x
        M: rows iD..iD+D-1 = point i): values (M,), then with want_grad the gradient (qD, M), then with want_wins the win counts
        (q, M) int32."""
        sets = _f(sets)
        q = self._set_block("qnei_eval", q, sets, "sets")
        t = self._baseline("qnei_eval", baseline)
        return self._set_eval(lib().sls_qnei_eval, q * self.D, q, sets, want_grad, want_wins, _p(t))

    def qnei_maximize(self, starts, q, n_local, baseline, offset=0, want_all=True, opts=None):
        """acq_maximize over [0,1]^(qD) with the set objective of qnei_eval (sls_qnei_maximize): starts qD x S, x and x_stars have qD
        rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        q = self._set_block("qnei_maximize", q, starts, "starts")
        t = self._baseline("qnei_maximize", baseline)
        return self._set_maximize(lib().sls_qnei_maximize, q * self.D, starts, n_local, offset, want_all, opts, q, _p(t))

    @staticmethod
    def _temperatures(who, tau_relu, tau_max):
        t0, tm = float(tau_relu), float(tau_max)
        if not (np.isfinite(t0) and t0 > 0.0):
            raise SlsError(f"{who}: tau_relu = {t0} (finite, > 0)")
        if not (np.isfinite(tm) and tm > 0.0):
            raise SlsError(f"{who}: tau_max = {tm} (finite, > 0)")
        return C.c_double(t0), C.c_double(tm)

    def qlognei_eval(self, sets, q, baseline, tau_relu=QLOGNEI_TAU_RELU, tau_max=QLOGNEI_TAU_MAX, want_grad=True, want_wins=False):
        """Log-space noisy expected improvement of q points on the draws over the per-draw baseline (sls_qlognei_eval) at the columns
        of sets (qD x M: rows iD..iD+D-1 = point i): values (M,), then with want_grad the gradient (qD, M), then with want_wins the
        hard win counts of qnei_eval (q, M) int32."""
        sets = _f(sets)
        q = self._set_block("qlognei_eval", q, sets, "sets")
        t = self._baseline("qlognei_eval", baseline)
        t0, tm = self._temperatures("qlognei_eval", tau_relu, tau_max)
        return self._set_eval(lib().sls_qlognei_eval, q * self.D, q, sets, want_grad, want_wins, _p(t), t0, tm)

    def qlognei_maximize(self, starts, q, n_local, baseline, tau_relu=QLOGNEI_TAU_RELU, tau_max=QLOGNEI_TAU_MAX, offset=0,
                         want_all=True, opts=None):
        """acq_maximize over [0,1]^(qD) with the set objective of qlognei_eval (sls_qlognei_maximize): starts qD x S, x and x_stars
        have qD rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        q = self._set_block("qlognei_maximize", q, starts, "starts")
        t = self._baseline("qlognei_maximize", baseline)
        t0, tm = self._temperatures("qlognei_maximize", tau_relu, tau_max)
        return self._set_maximize(lib().sls_qlognei_maximize, q * self.D, starts, n_local, offset, want_all, opts, q, _p(t), t0, tm)

    @staticmethod
    def _scale(who, scale):
        t = float(scale)
        if not (np.isfinite(t) and t >= np.finfo(np.float64).tiny):
            raise SlsError(f"{who}: scale = {t} (finite, > 0, not subnormal)")
        return C.c_double(t)

    def qbald_eval(self, sets, q, scale=QBALD_SCALE, want_grad=True, want_prob=False, want_wins=False):
        """Information gain of a q-option choice query under the BTL likelihood of the given scale, on the draws (sls_qbald_eval), at
        the columns of sets (qD x M: rows iD..iD+D-1 = option i): values (M,), then with want_grad the gradient (qD, M), then with
        want_prob the predicted choice probabilities (q, M), then with want_wins the hard win counts of qeubo_eval (q, M) int32."""
        sets = _f(sets)
        q = self._set_block("qbald_eval", q, sets, "sets")
        tau = self._scale("qbald_eval", scale)
        M = sets.shape[1]
        prob = np.zeros((q, M), order="F") if want_prob else None
        wins = np.zeros((q, M), dtype=np.int32, order="F") if want_wins else None
        return _eval_call(lambda *a: lib().sls_qbald_eval(self.h, q, tau, *a), sets, q * self.D, want_grad, prob, wins)

    def qbald_maximize(self, starts, q, n_local, scale=QBALD_SCALE, offset=0, want_all=True, opts=None):
        """acq_maximize over [0,1]^(qD) with the set objective of qbald_eval (sls_qbald_maximize): starts qD x S, x and x_stars have
        qD rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        q = self._set_block("qbald_maximize", q, starts, "starts")
        tau = self._scale("qbald_maximize", scale)
        return self._set_maximize(lib().sls_qbald_maximize, q * self.D, starts, n_local, offset, want_all, opts, q, tau)

    def _line_args(self, who, q, anchor, baseline, block, what):
        q = self._set_block(who, q, None, what, LINE_MIN_POSITIONS)
        a = None
        if anchor is not None:
            a = np.ascontiguousarray(np.asarray(anchor, dtype=np.float64))
            if a.shape != (self.D,):
                raise SlsError(f"{who}: anchor must hold D = {self.D} values, got shape {a.shape}")
        rows = self.D if a is not None else 2 * self.D
        if block.ndim != 2 or block.shape[0] != rows:
            raise SlsError(f"{who}: {what} must be {'D' if a is not None else '2D'} x M = {rows} x M, got {block.shape}")
        t = self._baseline(who, baseline) if baseline is not None else None
        return q, a, t, rows

    @staticmethod
    def _opt(a):
        return _p(a) if a is not None else None

    def line_eval(self, lines, q, anchor=None, baseline=None, want_grad=True, want_wins=False):
        """Expected utility of the best of q grid positions on the slider from a to b (sls_line_eval) at the columns of lines (2D x M:
        rows 0..D-1 = a, D..2D-1 = b; with anchor (D,) every line starts there and lines is D x M = b).  With baseline (n_draws,) the
        qNEI form.  Values (M,), then with want_grad the gradient (2D or D, M), then with want_wins the win counts (q, M) int32."""
        lines = _f(lines)
        q, a, t, rows = self._line_args("line_eval", q, anchor, baseline, lines, "lines")
        return self._set_eval(lib().sls_line_eval, rows, q, lines, want_grad, want_wins, self._opt(t), self._opt(a))

    def line_maximize(self, starts, q, n_local, anchor=None, baseline=None, offset=0, want_all=True, opts=None):
        """acq_maximize over the ends of a slider with the objective of line_eval (sls_line_maximize): starts 2D x S (D x S with
        anchor), x and x_stars have as many rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        q, a, t, rows = self._line_args("line_maximize", q, anchor, baseline, starts, "starts")
        return self._set_maximize(lib().sls_line_maximize, rows, starts, n_local, offset, want_all, opts, q, self._opt(t), self._opt(a))

    def _patch_args(self, who, qs, qt, anchor, baseline, block, what):
        qs, qt = int(qs), int(qt)
        if qs < PATCH_MIN_POSITIONS or qt < PATCH_MIN_POSITIONS or qs * qt > QEUBO_MAX_OPTIONS:
            raise SlsError(f"{who}: grid {qs} x {qt} (at least {PATCH_MIN_POSITIONS} per axis, at most {QEUBO_MAX_OPTIONS} cells)")
        a = None
        if anchor is not None:
            a = np.ascontiguousarray(np.asarray(anchor, dtype=np.float64))
            if a.shape != (self.D,):
                raise SlsError(f"{who}: anchor must hold D = {self.D} values, got shape {a.shape}")
        rows = (3 if a is not None else 4) * self.D
        if block.ndim != 2 or block.shape[0] != rows:
            raise SlsError(f"{who}: {what} must be {'3D' if a is not None else '4D'} x M = {rows} x M, got {block.shape}")
        t = self._baseline(who, baseline) if baseline is not None else None
        return qs, qt, a, t, rows

    def patch_eval(self, patches, qs, qt, anchor=None, baseline=None, want_grad=True, want_wins=False):
        """Expected utility of the best cell of a qs x qt grid on the bilinear patch spanned by four corners (sls_patch_eval) at the
        columns of patches (4D x M: rows in blocks of D = c00, c10, c01, c11; with anchor (D,) every patch has c00 there and patches is
        3D x M = c10, c01, c11).  With baseline (n_draws,) the qNEI form.  Values (M,), then with want_grad the gradient (4D or 3D, M),
        then with want_wins the win counts (qs qt, M) int32, cell (i, j) in row i + qs j."""
        patches = _f(patches)
        qs, qt, a, t, rows = self._patch_args("patch_eval", qs, qt, anchor, baseline, patches, "patches")
        return self._set_eval(lib().sls_patch_eval, rows, qs * qt, patches, want_grad, want_wins, self._opt(t), self._opt(a),
                              grid=(qs, qt))

    def patch_maximize(self, starts, qs, qt, n_local, anchor=None, baseline=None, offset=0, want_all=True, opts=None):
        """acq_maximize over the corners of a patch with the objective of patch_eval (sls_patch_maximize): starts 4D x S (3D x S with
        anchor), x and x_stars have as many rows.  GP.last_stats() of the path's handle reports the run."""
        starts = _f(starts)
        qs, qt, a, t, rows = self._patch_args("patch_maximize", qs, qt, anchor, baseline, starts, "starts")
        return self._set_maximize(lib().sls_patch_maximize, rows, starts, n_local, offset, want_all, opts, qs, qt, self._opt(t),
                                  self._opt(a))


class PrefCfg(C.Structure):
    _fields_ = [("use_map_hyperparams", C.c_int), ("default_a", C.c_double), ("default_r", C.c_double),
                ("default_b", C.c_double), ("prior_var", C.c_double), ("btl_scale", C.c_double), ("noiseless", C.c_int)]


class Nll:
    """Device state for the MAP objectives on a fixed design matrix (sls_nll_* / sls_gp_nll_grad / sls_pref_objective)."""

    def __init__(self, ctx, X, kernel=KERNEL_MATERN52):
        self.ctx = ctx
        X = _f(X)
        self.D, self.N = X.shape
        self.h = C.c_void_p()
        _ck(lib().sls_nll_create(ctx.h, _p(X), self.D, self.N, int(kernel), C.byref(self.h)))
        ctx._gps.append(weakref.ref(self))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_nll_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self, y, theta, b, want_grad=True):
        y, theta = _f(y), _f(theta)
        quad, logdet, gb = C.c_double(), C.c_double(), C.c_double()
        alpha = np.empty(self.N)
        gth = np.empty(self.D + 1)
        _ck(lib().sls_nll_eval(self.h, _p(y), _p(theta), C.c_double(b), C.byref(quad), C.byref(logdet), _p(alpha),
                               _p(gth) if want_grad else None, C.byref(gb) if want_grad else None))
        return dict(quad=quad.value, logdet=logdet.value, alpha=alpha, grad_theta=gth if want_grad else None,
                    grad_b=gb.value if want_grad else None)

    def gp_objective(self, y, x, want_grad=True):
        y, x = _f(y), _f(x)
        val = C.c_double()
        g = np.empty(self.D + 2) if want_grad else None
        _ck(lib().sls_gp_nll_grad(self.h, _p(y), _p(x), C.byref(val), _p(g) if want_grad else None))
        return (val.value, g) if want_grad else val.value

    def loo(self, y, theta, b, want_grad=True, want_mu=True, want_var=True, want_logp=True, want_value=True, want_grad_theta=None,
            want_grad_b=None):
        """Leave-one-out cross-validation at (theta, b) (sls_nll_loo): per-point mean, variance and log density, their sum
        `value`, and (want_grad) its gradient in theta = (a, r_1..r_D) and b.  Every output can be switched off on its own (the
        C entry gets NULL for it, the dict None); want_grad_theta and want_grad_b default to want_grad."""
        y, theta = _f(y), _f(theta)
        want_grad_theta = want_grad if want_grad_theta is None else want_grad_theta
        want_grad_b = want_grad if want_grad_b is None else want_grad_b
        val, gb = C.c_double(), C.c_double()
        mu, var, logp = (np.empty(self.N) if w else None for w in (want_mu, want_var, want_logp))
        gth = np.empty(self.D + 1) if want_grad_theta else None
        _ck(lib().sls_nll_loo(self.h, _p(y), _p(theta), C.c_double(b), _p(mu) if want_mu else None, _p(var) if want_var else None,
                              _p(logp) if want_logp else None, C.byref(val) if want_value else None, _p(gth) if want_grad_theta else None,
                              C.byref(gb) if want_grad_b else None))
        return dict(mu=mu, var=var, logp=logp, value=val.value if want_value else None, grad_theta=gth,
                    grad_b=gb.value if want_grad_b else None)

    def gp_loo_objective(self, y, x, want_grad=True):
        """The LOO log pseudo-likelihood plus the log-normal priors at x = (a, b, r_1..r_D) (sls_gp_loo_grad)."""
        y, x = _f(y), _f(x)
        val = C.c_double()
        g = np.empty(self.D + 2) if want_grad else None
        _ck(lib().sls_gp_loo_grad(self.h, _p(y), _p(x), C.byref(val), _p(g) if want_grad else None))
        return (val.value, g) if want_grad else val.value

    def gp_objective_batch(self, y, xs):
        """Values of the GP MAP objective at the rows of xs (B x (D + 2): a, b, r_1..r_D), one device call (sls_gp_nll_batch)."""
        y = _f(y)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        assert xs.ndim == 2 and xs.shape[1] == self.D + 2
        out = np.empty(xs.shape[0])
        _ck(lib().sls_gp_nll_batch(self.h, _p(y), _p(xs), xs.shape[0], _p(out)))
        return out

    def pref_objective(self, prefs, x, use_map=False, a=0.5, r=0.5, b=0.005, prior_var=0.25, btl_scale=0.01,
                       noiseless=False, want_grad=True):
        x = _f(x)
        flat = np.array([i for p in prefs for i in p], dtype=np.uint32)
        offs = np.zeros(len(prefs) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in prefs])
        cfg = PrefCfg(int(use_map), a, r, b, prior_var, btl_scale, int(noiseless))
        val = C.c_double()
        g = np.empty(len(x)) if want_grad else None
        _ck(lib().sls_pref_objective(self.h, flat.ctypes.data_as(C.POINTER(C.c_uint)), offs.ctypes.data_as(C.POINTER(C.c_int)),
                                     len(prefs), _p(x), C.byref(cfg), C.byref(val), _p(g) if want_grad else None))
        return (val.value, g) if want_grad else val.value


    def set_tolerances(self, ftol_rel, xtol_rel):
        """NLopt's relative stopping tests for this handle's MAP fits (sls_nll_set_tolerances); 0 = off (the default)."""
        _ck(lib().sls_nll_set_tolerances(self.h, C.c_double(ftol_rel), C.c_double(xtol_rel)))

    def pref_map_fit(self, prefs, z0, lower, upper, max_evals, evals_per_launch=0, use_map=False, a=0.5, r=0.5, b=0.005,
                     prior_var=0.25, btl_scale=0.01, noiseless=False):
        """PreferenceRegressor::PerformMapEstimation on the device (sls_pref_map_fit): z = (y [, log a, log b, log r..]).
        Returns dict(z, value, evals); raises Unsupported outside the device-resident limits."""
        z0, lower, upper = _f(z0), _f(lower), _f(upper)
        flat = np.array([i for p in prefs for i in p], dtype=np.uint32)
        offs = np.zeros(len(prefs) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in prefs])
        cfg = PrefCfg(int(use_map), a, r, b, prior_var, btl_scale, int(noiseless))
        z = np.empty(len(z0))
        val, ev = C.c_double(), C.c_int()
        rc = lib().sls_pref_map_fit(self.h, flat.ctypes.data_as(C.POINTER(C.c_uint)), offs.ctypes.data_as(C.POINTER(C.c_int)),
                                    len(prefs), C.byref(cfg), _p(z0), _p(lower), _p(upper), int(max_evals), int(evals_per_launch),
                                    _p(z), C.byref(val), C.byref(ev))
        if rc == ERR_UNSUPPORTED:
            raise Unsupported(lib().sls_last_error().decode())
        _ck(rc)
        return dict(z=z, value=val.value, evals=ev.value)

    def gp_map_fit(self, y, z0, lower, upper, max_evals, evals_per_launch=0):
        """Local phase of GaussianProcessRegressor::PerformMapEstimation on the device (sls_gp_map_fit): z = log (a, b, r..)."""
        y, z0, lower, upper = _f(y), _f(z0), _f(lower), _f(upper)
        z = np.empty(len(z0))
        val, ev = C.c_double(), C.c_int()
        rc = lib().sls_gp_map_fit(self.h, _p(y), _p(z0), _p(lower), _p(upper), int(max_evals), int(evals_per_launch), _p(z),
                                  C.byref(val), C.byref(ev))
        if rc == ERR_UNSUPPORTED:
            raise Unsupported(lib().sls_last_error().decode())
        _ck(rc)
        return dict(z=z, value=val.value, evals=ev.value)


class Multi:
    """One process driving several GPUs (sls_multi_*): replicated fit, starts sharded, one ncclAllGather."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        self.h = C.c_void_p()
        _ck(lib().sls_multi_create(arr, len(self.devices), C.byref(self.h)))
        lib().sls_multi_exchange.restype = C.c_char_p
        self._gps = []

    @property
    def exchange(self):
        return lib().sls_multi_exchange(self.h).decode()

    def close(self):
        if getattr(self, "h", None):
            for ref in self._gps:
                gp = ref()
                if gp is not None:
                    gp.close()
            self._gps = []
            lib().sls_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGP:
    def __init__(self, multi, X, y, theta, b, kernel=KERNEL_MATERN52):
        X, y, theta = _f(X), _f(y), _f(theta)
        self.D, self.N = X.shape
        self.h = C.c_void_p()
        _ck(lib().sls_multi_gp_create(multi.h, _p(X), self.D, self.N, _p(y), _p(theta), C.c_double(b), int(kernel), C.byref(self.h)))
        multi._gps.append(weakref.ref(self))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_multi_gp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def acq_maximize(self, starts, n_local, acq=ACQ_EI, ucb_h=1.0, opts=None):
        starts = _f(starts)
        x, val, idx, issued = np.empty(self.D), C.c_double(), C.c_long(), C.c_long()
        _ck(lib().sls_multi_acq_maximize(self.h, int(acq), C.c_double(ucb_h), _p(starts), starts.shape[1], int(n_local),
                                         C.byref(opts) if opts is not None else None, _p(x), C.byref(val), C.byref(idx),
                                         C.byref(issued)))
        return dict(index=idx.value, x=x, value=val.value, evals_issued=issued.value)

    def predict(self, Xs):
        """PredictMu / PredictSigma at the M columns of Xs, the columns sharded over the devices (sls_multi_gp_predict)."""
        Xs = _f(Xs)
        M = Xs.shape[1]
        mu, sigma = np.empty(M), np.empty(M)
        _ck(lib().sls_multi_gp_predict(self.h, _p(Xs), M, _p(mu), _p(sigma)))
        return mu, sigma


class MultiNll:
    """GP MAP objective over the devices of a Multi: the points of a batch dealt round-robin (sls_multi_gp_nll_batch)."""

    def __init__(self, multi, X, kernel=KERNEL_MATERN52):
        X = _f(X)
        self.D, self.N = X.shape
        self.h = C.c_void_p()
        _ck(lib().sls_multi_nll_create(multi.h, _p(X), self.D, self.N, int(kernel), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_multi_nll_destroy(self.h)
            self.h = None

    def gp_objective_batch(self, y, xs):
        y = _f(y)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        out = np.empty(xs.shape[0])
        _ck(lib().sls_multi_gp_nll_batch(self.h, _p(y), _p(xs), xs.shape[0], _p(out)))
        return out


class Comm:
    """One process per GPU: RCCL communicator inside the library (sls_comm_*).  `unique_id()` on rank 0, distribute the 128
    bytes, then Comm(ctx, id, rank, world) on every rank."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _ck(lib().sls_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, uid, rank, world):
        assert len(uid) == 128
        self.h = C.c_void_p()
        _ck(lib().sls_comm_create(ctx.h, uid, int(rank), int(world), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().sls_comm_destroy(self.h)
            self.h = None

    def allgather_best(self, value, index, x):
        x = _f(x)
        xo, vo, io = np.empty_like(x), C.c_double(), C.c_long()
        _ck(lib().sls_comm_allgather_best(self.h, C.c_double(value), C.c_long(index), _p(x), len(x), C.byref(vo), C.byref(io), _p(xo)))
        return vo.value, io.value, xo


def mes_terms(ctx, t):
    """(g(t), g'(t)) of max-value entropy search, evaluated on the device of `ctx` (sls_mes_terms)."""
    return ctx.mes_terms(t)


def merge_rank_results(results):
    """Global argmax over per-rank (value, global_index, x) triples: highest value, ties -> lowest global index
    (Eigen maxCoeff 'first maximum', src/acquisition-function.cpp:146-153).  `results` is an iterable of
    (value, index, x) with x a length-D array."""
    best = None
    for v, i, x in results:
        if best is None or v > best[0] or (v == best[0] and i < best[1]):
            best = (float(v), int(i), np.asarray(x, dtype=np.float64))
    return best


def shard_range(n_starts, rank, world):
    """Contiguous slice [lo, hi) of the global start set owned by `rank` (the last ranks get the remainder-free part)."""
    base, rem = divmod(int(n_starts), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def exchange_best(value, index, x, device=None, group=None):
    """The single collective of a multi-GPU maximisation: all-gather (value, global index, x[D]) over the ranks of a
    torch.distributed group (RCCL on GPUs, gloo on CPU) and take the first maximum on every rank.
    Returns (value, index, x) -- identical on all ranks.  The global index travels as float64 (exact below 2**53)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    x = np.asarray(x, dtype=np.float64)
    mine = torch.from_numpy(np.concatenate([[float(value), float(index)], x]))
    if device is not None:
        mine = mine.to(device)
    gathered = torch.empty(world * mine.numel(), dtype=torch.float64, device=mine.device)
    dist.all_gather_into_tensor(gathered, mine, group=group)
    g = gathered.cpu().numpy().reshape(world, mine.numel())
    return merge_rank_results((row[0], int(row[1]), row[2:]) for row in g)
