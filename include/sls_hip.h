/*
 * sls_hip.h -- C ABI of the MI355X-native GP regression + acquisition-maximisation
 * hot path (drop-in for the compute behind sequential-line-search's Regressor /
 * GaussianProcessRegressor / PreferenceRegressor / acquisition_func surface).
 *
 * The reference has no FFI layer: its "operator API" is the C++
 * public surface itself.  Each entry point below names the reference function(s)
 * whose arithmetic it replaces (paths relative to the reference tree).  The C++
 * classes in include/sequential-line-search/ and the tests bind exactly these.
 *
 * Conventions
 *   - plain C types only; every matrix is column-major double (Eigen::MatrixXd
 *     layout).  X is D x N: one data point per column, D contiguous doubles.
 *   - theta = (a, l_1..l_D)  (kernel_hyperparams), b = noise level.
 *   - pointers are HOST pointers unless the parameter name ends in _dev.
 *   - return 0 on success, <0 on error; sls_last_error() describes the last
 *     failure of the calling thread.  There is NO CPU fallback: every entry point
 *     runs hand-written gfx950 kernels and fails if no GPU is present.
 *   - a context owns one HIP stream and one (recursive) lock; a context and its
 *     handles may be shared by any number of host threads -- the reference shares one
 *     const regressor across hardware_concurrency worker threads
 *     (src/acquisition-function.cpp:125-144).  Two kinds of calls:
 *       * const evaluations of at most 64 points on a small handle (N <= 512, D <= 128:
 *         sls_gp_predict, sls_gp_predict_grad, sls_acq_eval) do NOT take the context's
 *         lock: each borrows one of the context's evaluation slots (own stream, own
 *         mapped result block) under a SHARED lock on the handle's fitted state and
 *         runs concurrently with the others (SLS_EVAL_SLOTS=0 restores the lock);
 *       * everything else -- fits, refits, sls_gp_append_point, sls_gp_set_sigma_mode,
 *         maximisers, MAP fits, larger evaluations -- holds the context's lock for the
 *         whole call (mutators also take the handle's state lock exclusively) and is
 *         SERIALISED in arrival order.
 *     A handle must outlive every call in flight on it: sls_gp_destroy waits for
 *     the evaluations that hold its state lock, but a call that STARTS after the
 *     destroy is a use after free, as with any C handle.  For independent streams of
 *     large work use one context per thread (or sls_multi, one per GPU).
 */
#ifndef SLS_HIP_H
#define SLS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* include/sequential-line-search/kernel-type.hpp:8-12 */
#define SLS_KERNEL_ARD_SQUARED_EXPONENTIAL 0
#define SLS_KERNEL_ARD_MATERN52 1
/* include/sequential-line-search/acquisition-function.hpp:11-15 */
#define SLS_ACQ_EXPECTED_IMPROVEMENT 0
#define SLS_ACQ_GP_UCB 1
/* not in the reference: log-space expected improvement ("log expected improvement" below); ucb_h is ignored */
#define SLS_ACQ_LOG_EXPECTED_IMPROVEMENT 2

#define SLS_OK 0
#define SLS_ERR_INVALID (-1)
#define SLS_ERR_HIP (-2)
#define SLS_ERR_NOT_SPD (-3)
#define SLS_ERR_NO_DEVICE (-4)
#define SLS_ERR_UNSUPPORTED (-5) /* the problem is outside what this entry point runs on the device; use the general path */

typedef struct sls_ctx sls_ctx;
typedef struct sls_gp sls_gp;

const char* sls_last_error(void);
int sls_version(void);

/* ---- context ------------------------------------------------------------ */
int sls_ctx_create(int device, sls_ctx** out);
/* Handles created from a context (sls_gp, sls_nll, sls_comm) may be destroyed after it: with live handles sls_ctx_destroy only
 * marks the context, the handles keep working, and the last one to go frees it (garbage-collected bindings finalise
 * objects in no particular order). */
int sls_ctx_destroy(sls_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores the own stream. */
int sls_ctx_set_stream(sls_ctx* ctx, void* hip_stream);
int sls_ctx_synchronize(sls_ctx* ctx);
/* Upper bound on candidates evaluated per device pass (workspace = 3 * chunk * N_pad doubles). Default 16384.
 * The pair objective (sls_eubo_*) evaluates max(128, chunk / 2 rounded down to 128) PAIRS per pass -- two cross-covariance blocks,
 * their difference and one product block per pair --, so its workspace stays at about what a single-point acquisition uses at the
 * same setting. */
int sls_ctx_set_candidate_chunk(sls_ctx* ctx, int chunk);

/* Device blocks released by handles and calls are cached per device (exact-size reuse; at most SLS_POOL_MB, default 16384,
 * MB): re-creating a regressor of the same shape costs no hipMalloc.  This returns every cached block of `device` to the
 * driver. */
int sls_device_trim_cache(int device);

/* ---- free functions of src/regressor.cpp --------------------------------- */
/* CalcLargeKY (src/regressor.cpp:61-71); b = 0 gives CalcLargeKF (:73-89).  K_out is N x N. */
int sls_gram(sls_ctx* ctx, const double* X, int D, int N, const double* theta, double b, int kernel, double* K_out);
/* CalcSmallK (src/regressor.cpp:45-59) for M query points at once: Ks_out is N x M, column m = k(Xs[:,m], X). */
int sls_gram_cross(sls_ctx* ctx, const double* X, int D, int N, const double* Xs, int M, const double* theta, int kernel,
                   double* Ks_out);

/* ---- dense factorisation (Eigen::LLT / MatrixXd::inverse stand-ins) ------ */
/* Eigen::LLT<MatrixXd>(K) (src/preference-regressor.cpp:162,290): A (N x N, symmetric, lower read) -> lower factor L
 * (upper zeroed).  SLS_ERR_NOT_SPD if a pivot is not positive. */
int sls_potrf(sls_ctx* ctx, double* A, int N);
/* LLT::solve (src/preference-regressor.cpp:165,296,309,320,329): B (N x nrhs) <- (L L^T)^-1 B. */
int sls_potrs(sls_ctx* ctx, const double* L, int N, double* B, int nrhs);
/* K^-1 from its Cholesky factor (replaces m_K_y.inverse(), src/gaussian-process-regressor.cpp:159,211,231). */
int sls_potri(sls_ctx* ctx, const double* L, int N, double* Ainv);

/* ---- GP handle ----------------------------------------------------------- */
/* GaussianProcessRegressor(X, y, kernel_hyperparams, noise, kernel_type) (src/gaussian-process-regressor.cpp:214-232) and the
 * post-MAP state of PreferenceRegressor (src/preference-regressor.cpp:289-290): builds K_y, its Cholesky factor, K_y^-1,
 * alpha = K_y^-1 y and the hoisted PredictMaximumPointFromData (src/regressor.cpp:29-43) on the device. */
int sls_gp_create(sls_ctx* ctx, const double* X, int D, int N, const double* y, const double* theta, double b, int kernel,
                  sls_gp** out);
int sls_gp_destroy(sls_gp* gp);
/* Append one observation (x, y) to a fitted handle in O(N^2) (Schur-complement update of K_y^-1, one new row of the
 * Cholesky factor): what FindNextPoints needs after every accepted point instead of re-building the dummy regressor
 * (src/acquisition-function.cpp:280-293). */
int sls_gp_append_point(sls_gp* gp, const double* x, double y);

#define SLS_GP_K_Y 0        /* N x N  m_K_y / m_K          (gaussian-process-regressor.hpp:31, preference-regressor.hpp:57) */
#define SLS_GP_K_Y_INV 1    /* N x N  m_K_y_inv            (gaussian-process-regressor.hpp:32) */
#define SLS_GP_CHOL_L 2     /* N x N  m_K_llt.matrixL()    (preference-regressor.hpp:60) */
#define SLS_GP_ALPHA 3      /* N      K_y^-1 y */
#define SLS_GP_MU_DATA 4    /* N      PredictMu at every data point (regressor.cpp:34-37) */
int sls_gp_get_matrix(sls_gp* gp, int what, double* out);
/* How the predictive deviation is formed.  The two reference classes differ (and so do the two modes, by rounding only):
 *   SLS_SIGMA_EXPLICIT_INVERSE (default)  sigma^2 = a - k^T K_y^-1 k with the explicit inverse, GaussianProcessRegressor::PredictSigma
 *                                         (src/gaussian-process-regressor.cpp:241-255, m_K_y_inv);
 *   SLS_SIGMA_CHOLESKY_SOLVE              sigma^2 = a - k . LLT.solve(k) = a - |L^-1 k|^2, PreferenceRegressor::PredictSigma
 *                                         (src/preference-regressor.cpp:299-313); the sigma gradient uses L^-T (L^-1 k) (:323-330).
 * For ill-conditioned K_y (cond >= 1e6, sigma <= 3e-3) the first form is only accurate to cond(K_y) eps a / (2 sigma), the second to
 * ~1e-12; a handle that stands for a PreferenceRegressor should therefore use the second, as the reference does. */
#define SLS_SIGMA_EXPLICIT_INVERSE 0
#define SLS_SIGMA_CHOLESKY_SOLVE 1
int sls_gp_set_sigma_mode(sls_gp* gp, int mode);
/* best_index / x_best: PredictMaximumPointFromData (src/regressor.cpp:29-43); mu_best = PredictMu(x_best);
 * logdet = CalcLogDetOfSymmetricPositiveDefiniteMatrix(K_y).  Any out pointer may be NULL. */
int sls_gp_get_summary(sls_gp* gp, int* best_index, double* mu_best, double* logdet);
/* A number that changes whenever the predictor behind the handle changes (fit, sls_gp_refit_dev, sls_gp_append_point,
 * sls_gp_set_sigma_mode) and is never repeated within the process, not even by a new handle at a recycled address: callers that
 * cache something derived from the handle (the host layer's replicas on other GPUs) compare it instead of the pointer. */
int sls_gp_generation(sls_gp* gp, long* generation);

/* PredictMu / PredictSigma for M points (gaussian-process-regressor.cpp:234-255, preference-regressor.cpp:293-313). */
int sls_gp_predict(sls_gp* gp, const double* Xs, int M, double* mu, double* sigma);
/* PredictMuDerivative / PredictSigmaDerivative (:257-272 / :315-330) for M points: dmu, dsigma are D x M. */
int sls_gp_predict_grad(sls_gp* gp, const double* Xs, int M, double* dmu, double* dsigma);
/* acquisition_func::CalcAcquisitionValue / CalcAcquisitionValueDerivative (src/acquisition-function.cpp:170-230)
 * for M points; grad (D x M) may be NULL. */
int sls_acq_eval(sls_gp* gp, int acq_type, double ucb_h, const double* Xs, int M, double* val, double* grad);

/* ---- joint posterior at a set of query points (not in the reference) --------------------------------------------------
 * sklearn's GaussianProcessRegressor.predict(return_cov=True) / sample_y for the latent function of a fitted handle.  For the
 * handle's data X (D x N), theta = (a, l), and M query points Xs (D x M):
 *   mu_m  = the posterior mean (the quantity of sls_gp_predict);
 *   cov   = K(Xs, Xs) - V^T V with V = L^-1 K*, K* = k(X, Xs), L = chol(K_y): the LATENT covariance (no b on the diagonal; its
 *           diagonal is the sigma^2 of PredictSigma), always in this triangular form whatever the handle's sigma mode (the
 *           form of PreferenceRegressor, SLS_SIGMA_CHOLESKY_SOLVE).  Full M x M column-major, EXACTLY symmetric (lower tiles
 *           computed, mirrored).  The diagonal is NOT clamped at 0 (sls_gp_predict clamps sigma^2): rounding may leave it at
 *           -O(eps a) where the posterior variance vanishes.
 * 1 <= M <= 8192 (the largest factorisation measured in this library); larger M returns SLS_ERR_UNSUPPORTED, M = 0 is a no-op.
 * Both GP calls hold the context's lock and the handle's state lock (shared) for the whole call, as the other evaluations of
 * more than a few points do. */
/* Joint posterior of the latent function at M query points (D x M): mu (M, may be NULL), cov (M x M column-major, full). */
int sls_gp_predict_cov(sls_gp* gp, const double* Xs, int M, double* mu, double* cov);
/* n_samples draws of f ~ N(mu, cov + j I) at the M points: samples M x n_samples column-major, one draw per column;
   jitter_used (may be NULL) = j.
 * F = mu 1^T + L_S Z with L_S = chol(cov + j I): j = 0 first; on a non-positive pivot j = 1e-12 a, then ten times that up to
 * 1e-6 a (the factorisation restarts from a kept copy of cov each time); SLS_ERR_NOT_SPD if 1e-6 a fails too.  A pivot
 * L_ii^2 <= M 2^-52 a counts as non-positive: duplicate query points make cov exactly singular, and the sign of the pivot that
 * rounding leaves there is an accident; with this rule such a cov always takes the jitter.  Z[j, s] = normal number s M + j of stream `seed`
 * (sls_random_normal): the bits depend on neither launch geometry nor the internal chunking over samples, the first k columns of an
 * n-sample call equal a k-sample call, and equal inputs give equal bits.  Any n_samples >= 1. */
int sls_gp_sample_posterior(sls_gp* gp, const double* Xs, int M, int n_samples, unsigned long long seed,
                            double* samples, double* jitter_used);
/* out[i] = standard normal number offset + i of stream `seed` (the generator behind sls_gp_sample_posterior).
 * Number t: Philox4x64-10 keyed by (seed, 0) on the block counter (t / 4, 0, 0, 0); each 64-bit output x becomes
 * u = ((x >> 11) + 0.5) 2^-53; Box-Muller on the outputs (0, 1) and (2, 3) gives r01 cos, r01 sin, r23 cos, r23 sin for
 * t mod 4 = 0, 1, 2, 3 (r = sqrt(-2 log u_even), angle 2 pi u_odd).  offset >= 0, n >= 0. */
int sls_random_normal(sls_ctx* ctx, unsigned long long seed, long offset, long n, double* out);

/* ---- multi-start maximiser ------------------------------------------------ */
/* FindGlobalSolution, parallelised multi-start branch (src/acquisition-function.cpp:121-153): S bounded L-BFGS runs
 * on [0,1]^D from the explicit starts (D x S), n_local objective evaluations each, all S advanced in lock step on the
 * device; returns the first maximum over the end points (Eigen maxCoeff semantics).
 * idx_out is the winning start's index plus start_index_offset (so that ranks sharding one global start set report
 * global indices).  x_stars (D x S) / y_stars (S) may be NULL. */
typedef struct sls_lbfgs_opts {
    /* sizeof(sls_lbfgs_opts) as the CALLER's header declares it (sls_lbfgs_default_opts fills it in).  The struct is caller-
     * allocated and has grown once already (ftol_rel / xtol_rel, round 5): the library reads struct_size bytes and takes its
     * defaults for members beyond them, and refuses a size it does not know (0, or larger than its own). */
    int struct_size;
    int history;        /* L-BFGS memory m (1..8), default 6 */
    double c1;          /* Armijo constant, default 1e-4 */
    double shrink;      /* backtracking factor, default 0.5 */
    double gtol;        /* projected-gradient inf-norm stop, default 0 */
    int max_backtracks; /* default 20 */
    /* NLopt's relative stopping tests (nlopt/src/util/stop.c, relstop), applied to every ACCEPTED step x -> x', f -> f'; 0 = off
     * (the default of this ABI: a start then runs until it cannot move or reaches its cap).  The reference's searches go through
     * nloptutil::solve, whose defaults are ftol_rel = xtol_rel = 1e-6: the host layer passes those.
     *   ftol_rel: stop when |f' - f| < ftol_rel (|f'| + |f|) / 2 or f' == f
     *   xtol_rel: stop when for every d  |x'_d - x_d| < xtol_rel (|x'_d| + |x_d|) / 2 or x'_d == x_d
     * The accepted point is kept; the start leaves the batch. */
    double ftol_rel;
    double xtol_rel;
} sls_lbfgs_opts;
void sls_lbfgs_default_opts(sls_lbfgs_opts* o);
int sls_acq_maximize(sls_gp* gp, int acq_type, double ucb_h, const double* starts, int S, int n_local,
                     const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                     double* x_stars, double* y_stars);
/* Statistics of the last sls_acq_maximize* call on this handle.  The starts advance in lock step over an ACTIVE SET: a start
 * that can no longer move (stationary projected gradient, null step, exhausted backtracking) is finished and leaves the
 * batch -- NLopt's max_evals is a cap per start, not a quota (src/acquisition-function.cpp:128-129).
 *   evals_issued  objective evaluations actually performed (sum over rounds of the live starts)
 *   evals_cap     S * n_local
 *   rounds        lock-step rounds executed (<= n_local)
 *   live_at_end   starts still moving when the cap was reached
 * Any out pointer may be NULL.  (The single-launch wavefront path for small problems counts, inside the kernel, the evaluations
 * of starts that were still moving, and reports rounds = n_local.) */
int sls_acq_last_stats(sls_gp* gp, long* evals_issued, long* evals_cap, int* rounds, int* live_at_end);
/* Same, with the starts already resident in HBM (D x S column-major device buffer) -- the timed path of bench.py. */
int sls_acq_maximize_dev(sls_gp* gp, int acq_type, double ucb_h, const double* starts_dev, int S, int n_local,
                         const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                         long* idx_out);
/* objective_for_multiple_points (src/acquisition-function.cpp:63-110), the inner objective of FindNextPoints (:246-298):
 * predictive mean (and mu+) from gp_mean, predictive deviation from gp_sigma (the variance-updated dummy regressor). */
int sls_acq_eval_pair(sls_gp* gp_mean, sls_gp* gp_sigma, int acq_type, double ucb_h, const double* Xs, int M, double* val,
                      double* grad);
int sls_acq_maximize_pair(sls_gp* gp_mean, sls_gp* gp_sigma, int acq_type, double ucb_h, const double* starts, int S, int n_local,
                          const sls_lbfgs_opts* opts, double* x_out, double* val_out, long* idx_out);
/* Re-fit an existing handle in place from device-resident X (D x N), y (N): the timed "GP fit" of bench.py.  D, N, theta, b, the
 * kernel and the sigma mode stay those of the handle; X_dev / y_dev are read on the context's stream (sls_ctx_set_stream) and copied:
 * the caller's buffers are free again on return.
 * On an error from the fit (SLS_ERR_NOT_SPD: K_y is not positive definite) the handle's data are the new X, y but its fitted state is
 * UNDEFINED until the next successful sls_gp_refit_dev: the matrices, the summary and every evaluation may mix the old fit and the
 * failed one, and the evaluation entry points do not detect this (they return SLS_OK).  sls_gp_generation has changed, so objects
 * derived from the old fit (sls_path) are refused.  The handle stays valid for sls_gp_refit_dev and sls_gp_destroy, the context for
 * everything. */
int sls_gp_refit_dev(sls_gp* gp, const double* X_dev, const double* y_dev);

/* ---- Laplace posterior for preference data (not in the reference) -------------------------------------------------------------
 * A handle that stands for a PreferenceRegressor was fitted to the MAP goodness values y as if they had been OBSERVED with noise b: its
 * variance a - k*^T K_y^-1 k* is that of a GP that has seen y, not of a model that has only seen choices.  The Laplace approximation at
 * y (Chu & Ghahramani 2005; Rasmussen & Williams 3.4) replaces it.  With K_y = K_f + b I = L L^T, alpha = K_y^-1 y, the tuples in the
 * CSR form of sls_pref_objective (first index of a tuple = the chosen point) and s = btl_scale:
 *   per tuple (i_0 .. i_{m-1}):  p = softmax(y_i / s), the maximum subtracted (no overflow at any y, s);  H = (diag(p) - p p^T) / s^2
 *   W        N x N, the scatter-sum of every H at (i_j, i_k); an index repeated inside a tuple adds.  Symmetric PSD, singular.
 *   B        = I + L^T W L                      eigenvalues >= 1;  B = L_B L_B^T
 *   Sigma_g  = (K_y^-1 + W)^-1 = L B^-1 L^T     posterior covariance of the goodness values
 *   T        = I - B^-1 = B^-1 (L^T W L)        formed as that PRODUCT, eigenvalues in [0, 1)
 *   M        = L^-T T L^-1 = L^-T B^-1 (L^T W)  the effective inverse (= K_y^-1 - K_y^-1 Sigma_g K_y^-1, never formed as a difference)
 *   mean     k*^T alpha (unchanged)             sigma^2 = max(0, a - k*^T M k*)          grad sigma = -(1 / sigma) J M k*
 *   cov      = K(Xs, Xs) - V T V^T, V = K* L^-T (sls_gp_predict_cov's V)
 *   path     r_s = (y + L L_B^-T z_s) - sqrt(b) eps_s - f_prior,s(X),  v_s = K_y^-1 r_s:  Matheron's rule with a sampled goodness vector
 *   evidence log_lik = sum_t log p_{t,0};  log Z = log_lik - 1/2 y^T alpha - 1/2 log|B|
 * M, T, L^T W L and Sigma_g are symmetric products: their lower 128 x 128 tiles are computed and the upper triangle is the exact mirror.
 * W is assembled without floating-point atomics (one lane per row, tuples in increasing order), log_lik and log|B| are reduced in one
 * fixed order: equal inputs give equal bits in every matrix and in the summary.  All device work runs on the context's stream.
 *
 * sls_gp_set_laplace: n_prefs >= 1, every tuple of length >= 2 (pref_offsets[0] = 0, increasing), every index < N, btl_scale > 0 and
 * finite: else SLS_ERR_INVALID before any launch, the handle unchanged.  It works at any y (the handle's y need not be a mode) and in
 * either sigma mode: the Laplace variance takes the place of both.  Setting twice replaces the state.  Set and clear change
 * sls_gp_generation, so objects derived from the handle before (sls_path, sls_jes, sls_kg) are refused afterwards.  After
 * sls_gp_clear_laplace every call returns the bits it returned before the set.  Memory: five N x N matrices while set.
 * While the state is set the fit is frozen: sls_gp_set_sigma_mode, sls_gp_append_point and sls_gp_refit_dev return SLS_ERR_UNSUPPORTED
 * and change nothing.
 *
 * What a Laplace handle does, per entry point ("tiled": the explicit-inverse route of the tiled evaluation with M in the place of K_y^-1;
 * the one-wavefront path, the evaluation slots, the zero-copy path and the triangular value-only form are switched off for it, so mu
 * is bit-equal to the plain handle's mu ON THE TILED ROUTE):
 *   sls_gp_predict, sls_gp_predict_grad, sls_acq_eval                    honour (tiled)
 *   sls_acq_maximize, sls_acq_maximize_dev                               honour (tiled, lock-step L-BFGS)
 *   sls_acq_eval_sub, sls_acq_maximize_sub                               honour
 *   sls_mes_eval, sls_mes_maximize, sls_mes_eval_sub, sls_mes_maximize_sub   honour
 *   sls_gp_predict_cov, sls_gp_sample_posterior                          honour (cov = K - V T V^T)
 *   sls_path_create                                                      honour; draw s takes 2F + 2N normal numbers from B0 + s (2F + 2N)
 *                                                                        in the order w, w', eps, z (plain handles keep 2F + N); the first
 *                                                                        k draws of an n-draw object stay a k-draw object bit for bit
 *   sls_path_*, sls_qeubo_*, sls_qnei_*, sls_qlognei_*, sls_qbald_*, sls_line_*, sls_patch_*   unchanged: they consume the object's (W, V)
 *   sls_multi_acq_maximize, sls_multi_gp_predict                         refuse when any shard carries the state (the borrowed primary of
 *                                                                        sls_multi_gp_create_from after a later sls_gp_set_laplace, or a
 *                                                                        shard of sls_multi_gp_shard): the other shards are plain fits
 *   sls_eubo_eval, sls_eubo_maximize                                     refuse (SLS_ERR_UNSUPPORTED)
 *   sls_acq_eval_pair, sls_acq_maximize_pair (either handle)             refuse
 *   sls_jes_create, sls_kg_create                                        refuse
 *   sls_gp_loo                                                           refuse
 *   sls_multi_gp_create_from                                             refuse (sls_multi_gp_create builds plain replicas: no state)
 *   sls_gp_get_matrix, sls_gp_get_summary                                the plain fit's K_y, K_y^-1, L, alpha, mu_best, log|K_y| (no variance)
 * No entry point uses the plain variance on a Laplace handle. */
int sls_gp_set_laplace(sls_gp* gp, const unsigned* prefs_flat, const int* pref_offsets, int n_prefs, double btl_scale);
int sls_gp_clear_laplace(sls_gp* gp);                 /* back to the plain handle: bit-equal to before the set; no state: a no-op */
#define SLS_LAPLACE_W 0      /* N x N */
#define SLS_LAPLACE_COV 1    /* N x N  Sigma_g (formed on demand: two N^3 products per call) */
#define SLS_LAPLACE_M 2      /* N x N  effective inverse */
/* SLS_ERR_INVALID on a handle without the state */
int sls_gp_laplace_get(sls_gp* gp, int what, double* out);
int sls_gp_laplace_summary(sls_gp* gp, double* log_lik, double* logdet_B, double* log_evidence);   /* any may be NULL */

/* ---- pathwise posterior function draws (not in the reference) ---------------------------------------------------------
 * Thompson sampling needs a draw of the latent function that can be evaluated -- and maximised -- anywhere in [0,1]^D.  Pathwise
 * conditioning (Wilson et al. 2020) gives each draw s in closed form:
 *   f_s(x) = sqrt(a/F) sum_l [ w_{s,l} cos(om_l . x~) + w'_{s,l} sin(om_l . x~) ]  +  sum_i v_{s,i} k(x, x_i)
 *   v_s    = K_y^-1 ( y - f_prior,s(X) - sqrt(b) eps_s )
 * with x~ = (x - 0.5) o inv_ell, F random frequencies om_l, w, w' ~ N(0, I), eps_s ~ N(0, I_N).  SE: om ~ N(0, I);
 * Matern 5/2: om = z sqrt(5 / u), z ~ N(0, I), u ~ chi^2_5.  A PreferenceRegressor handle works unchanged (y = MAP latent, b its
 * noise).
 * ONE frequency set is shared by all draws of an object: each draw is an exact draw from the random-feature-approximate posterior,
 * but the approximation error of the prior (O(a / sqrt(F))) is common to all draws, not independent between them.
 * Generator (sls_random_normal of stream `seed`; part of the contract):
 *   frequency l uses numbers l D .. l D + D - 1 (z);  Matern only: u_l = sum_{j<5} z^2 over numbers F D + 5 l + j;
 *   B0 = F D (SE) or F D + 5 F (Matern) is the length of this draw-independent block;
 *   draw s starts at B0 + s (2F + N): w_s (F numbers), then w'_s (F), then eps_s (N).
 * So the first k draws of an n-draw object equal a k-draw object bit for bit, and equal inputs give equal bits.
 * The object keeps v (N x n_draws), W (2F x n_draws) and om (F x D) on the device and records sls_gp_generation: a call after the
 * handle was refitted, grown (sls_gp_append_point) or switched in sigma mode returns SLS_ERR_INVALID and uses no stale state.
 * Locks as the handle's other large calls: the context's lock and the handle's state lock (shared) for the whole call.  The
 * object must not outlive its handle.
 * Limits: 1 <= n_draws <= 4096, 1 <= n_freq <= 16384 (padding is internal); anything else is SLS_ERR_INVALID.
 * Memory: the object keeps om, W and v only (about 8 (F D + 2 F n_draws + N n_draws) bytes, padded).  Each eval / maximize call takes
 * its workspace from the device pool and returns it at the end: per candidate chunk about 3 chunk N + 2 chunk F doubles (chunk <=
 * min(16384, 2^26 / max(N, 2F))), i.e. up to 2 GB at N = 8192; sls_device_trim_cache gives the pool's blocks back to the driver. */
typedef struct sls_path sls_path;
/* n_draws posterior function draws of the fitted handle gp, F = n_freq random frequencies (2F features), stream `seed`. */
int sls_path_create(sls_gp* gp, int n_draws, int n_freq, unsigned long long seed, sls_path** out);
int sls_path_destroy(sls_path* p);
/* draw_of_point == NULL: val is M x n_draws (every draw at every point, column-major), grad must be NULL.
   otherwise: val[m] = f_{draw_of_point[m]}(Xs[:,m]), grad D x M (may be NULL).  Xs is D x M.  A point's bits depend neither on its
   column nor on the other points of the call. */
int sls_path_eval(sls_path* p, const double* Xs, int M, const int* draw_of_point, double* val, double* grad);
/* starts D x (n_draws * S): columns [s*S, (s+1)*S) belong to draw s.  One lock-step bounded L-BFGS over all of them (n_local
   evaluations per start, the maximiser of sls_acq_maximize with f_s as the objective); per draw the first maximum over its own
   end points: x_out D x n_draws, val_out n_draws, idx_out n_draws (start index within the draw).  Any out pointer may be NULL.
   A draw's result does not depend on the other draws or their starts. */
int sls_path_maximize(sls_path* p, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts, double* x_out,
                      double* val_out, long* idx_out);

/* ---- max-value entropy search (not in the reference) -------------------------------------------------------------------
 * MES (Wang & Jegelka, ICML 2017): the expected reduction of the entropy of the maximum VALUE y* of the latent function, estimated
 * on K samples y*_1..y*_K of that maximum -- the per-draw maxima val_out of sls_path_maximize are such a sample.  For a point x
 * with mu = PredictMu(x) and sigma = PredictSigma(x) in the handle's current sigma mode (the quantities of sls_gp_predict, formed as
 * sls_acq_eval forms them on the tiled evaluation; sls_gp_predict's other routes agree with them to cond(K_y) eps, not to the bit):
 *   gamma_k       = (y*_k - mu) / sigma
 *   g(t)          = 1/2 t r(t) - log Phi(t),   r = phi / Phi        g'(t) = -1/2 r(t) (1 + t (t + r(t)))
 *   alpha(x)      = (1/K) sum_k g(gamma_k)                          (every sum over k in increasing k)
 *   grad alpha(x) = -(1/sigma) [ A1 grad mu + A2 grad sigma ],  A1 = (1/K) sum_k g'(gamma_k),  A2 = (1/K) sum_k gamma_k g'(gamma_k)
 * There is no mu - mu_best term that can underflow.  Guard (the one of expected improvement): sigma < 1e-10, or a NaN in the value or
 * in any gradient component, gives the value 0 and the zero gradient.
 * Phi never underflows: for t < 0, with e = erfcx(-t / sqrt 2), r = sqrt(2/pi) / e and log Phi = log(e / 2) - t^2 / 2; for t >= 0
 * Phi = erfc(-t / sqrt 2) / 2 and log Phi = log1p(-erfc(t / sqrt 2) / 2).  c = 1 + t (t + r) cancels to ~2 / t^2 for large negative t
 * (the direct form loses ~t^4 eps / 2 relative): for t < -30, c = u (2 + u (-10 + u (74 + u (-706 + 8162 u)))) with u = 1 / t^2.
 * g is accurate to a few eps max(1, t^2) (for t << 0 it is the O(log |t|) difference of two O(t^2) terms), g' to ~1e-10 relative.
 * One lane per point and fixed summation orders: a point's bits depend on neither its column, the other points of the call nor the
 * candidate chunk.  Both GP calls always take the tiled evaluation (never the single-launch path of small problems or the
 * evaluation slots) and hold the context's lock for the whole call, as the handle's other large calls do; y_star is uploaded once
 * per call. */
#define SLS_MES_MAX_SAMPLES 4096
/* g[i] = g(t[i]), dg[i] = g'(t[i]); either out pointer may be NULL; n >= 0.  The scalar terms on their own (a test hook, as
 * sls_random_normal is for the generator). */
int sls_mes_terms(sls_ctx* ctx, const double* t, long n, double* g, double* dg);
/* alpha at the M points Xs (D x M): val (M), grad (D x M, may be NULL); 1 <= K <= SLS_MES_MAX_SAMPLES and every y_star finite: else
 * SLS_ERR_INVALID; M = 0 is a no-op. */
int sls_mes_eval(sls_gp* gp, const double* y_star, int K, const double* Xs, int M, double* val, double* grad);
/* sls_acq_maximize with alpha as the objective: same outputs, same semantics of idx_out / x_stars / y_stars / sls_acq_last_stats. */
int sls_mes_maximize(sls_gp* gp, const double* y_star, int K, const double* starts, int S, int n_local,
                     const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                     double* x_stars, double* y_stars);

/* ---- joint entropy search (not in the reference) ----------------------------------------------------------------------
 * JES (Hvarfner et al., NeurIPS 2022; Tu et al., NeurIPS 2022): the expected reduction of the entropy of the optimum PAIR (x*, f*),
 * estimated on K sampled optima (x*_k, f*_k) -- x_out / val_out of sls_path_maximize are such a sample.  MES uses the values f*_k alone;
 * JES conditions the posterior on each pair and asks how much an observation at x shrinks what is left.
 * mu(x), sigma(x): the tiled evaluation's mean and deviation in the handle's sigma mode (the quantities of max-value entropy search
 * above).  star_noise >= 0: the variance with which an optimum value counts as observed.  noise_var > 0: the observation-noise variance
 * of a future measurement (the host layer passes the handle's b).
 * Per optimum, fixed when the object is created (x*_k clamped into [0,1]^D first, as starts are):
 *   mu*_k = mu(x*_k)     v_k = max(sigma^2(x*_k), 0) + star_noise     d_k = f*_k - mu*_k     w_k = K_y^-1 k(X, x*_k)
 * (mu(x*_k), sigma(x*_k) >= 0 are what sls_gp_predict's tiled route returns at x*_k, bit for bit; v_k is formed from that clamped
 * deviation as sigma sigma + star_noise, the square rounded on its own).
 * k(X, x*_k) and k(x, x*_k) are formed from the differences of the raw coordinates on EVERY handle (relative error (D + O(1)) eps in the
 * scaled distance at any length scale), also where the handle's own Gram routes use the norm expansion: on such a handle the
 * right-hand side of w_k is not the Gram the factor of K_y was built from, entry for entry, but agrees with it within the guard's
 * bound (1e-11 absolute in the scaled squared distance), which is below what cond(K_y) eps leaves of w_k.
 * Per candidate and optimum:
 *   c_k(x) = k(x, x*_k) - k*(x)^T w_k            posterior covariance of f(x) and f(x*_k)
 *   m_k    = mu + (c_k / v_k) d_k                 s_k^2 = sigma^2 - c_k (c_k / v_k)          (c_k / v_k formed as c_k (1 / v_k))
 *   gamma_k = (f*_k - m_k) / s_k
 *   tau(t) = 1 - r(t) (t + r(t)),  r = phi / Phi  variance factor of a unit normal truncated above at t
 *   q_k    = noise_var + s_k^2 tau(gamma_k)
 *   alpha(x) = 1/2 log(sigma^2 + noise_var) - (1 / 2K) sum_k log q_k                         (every sum over k in increasing k)
 * Gradient, with tau'(t) = r [(t + r)(t + 2 r) - 1]:
 *   grad alpha = A_mu grad mu + A_sigma grad sigma + sum_k h_k grad c_k(x)
 *   grad c_k(x) = grad_x k(x, x*_k) - sum_i W_ik grad_x k(x, X_i)
 *   dq_k/dmu = -s_k tau'     dq_k/dsigma = 2 sigma tau - gamma_k sigma tau'
 *   dq_k/dc  = -(2 c_k / v_k) tau + tau' (gamma_k c_k / v_k - s_k d_k / v_k)
 *   A_mu = -(1 / 2K) sum_k (dq_k/dmu) / q_k     A_sigma = sigma / (sigma^2 + noise_var) - (1 / 2K) sum_k (dq_k/dsigma) / q_k
 *   h_k  = -(1 / 2K) (dq_k/dc) / q_k
 * Rules that make the value a function:
 *   uninformative optimum: v_k < 1e-20 takes c_k / v_k as 0 (m_k = mu, s_k = sigma, dq_k/dc = 0);
 *   collapsed conditional: s_k^2 < 1e-20 makes the term log noise_var and adds nothing to A_mu, A_sigma or h_k;
 *   the guard of expected improvement: sigma < 1e-10, or a NaN in the value or any gradient component: value 0, gradient 0.
 * Numerics of tau: Phi never appears alone.  t < 0: r = sqrt(2/pi) / erfcx(-t / sqrt 2), w = r + t (LogEI's), c = 1 + t w (MES's),
 * tau = c - w^2, tau' = r (w^2 - tau); for t < -30 c comes from MES's series in u = 1 / t^2 and w = (c - 1) / t (the direct forms
 * cancel to ~1 / t^2).  t >= 0: Phi = erfc(-t / sqrt 2) / 2, w = r + t, tau = 1 - r w, tau' = r (w^2 - tau).  tau' is the difference of two
 * O(1 / t^2) terms that leaves O(1 / t^4): its relative error grows to ~t^6 eps / 2 just above t = -30 (DESIGN.md has the measured figures).
 * The object is a snapshot, as sls_path is: it keeps W (N x K, padded), the clamped optima, mu*, v, d, f* on the device and records
 * sls_gp_generation: a call after the handle was refitted, grown (sls_gp_append_point) or switched in sigma mode returns SLS_ERR_INVALID
 * and uses no stale state.  It must not outlive its handle.  Every call holds the context's lock for its whole length, as the handle's
 * other large calls do, always takes the tiled evaluation (never the single-launch path of small problems or the evaluation slots) and
 * forms mu, sigma as the gradient evaluations do, whether or not grad is asked for.
 * Stages per candidate chunk: the tiled evaluation (mu, sigma, grad mu, grad sigma); k(x, x*_k) from the raw coordinate differences and
 * c = k(x, x*) - K* W on the tile GEMM (fixed k order); the combiner, one lane per candidate; for the gradient U = -H W^T on the tile
 * GEMM, P = C* o U, the P-pass of grad_gemm (or the raw-difference contraction beyond the Gram guard), the optima term and the finish.
 * A point's bits depend on neither its column, the other points of the call, the candidate chunk nor active-set compaction.
 * sls_prof_get names: "jes_setup" (create: k(X, X*), the solve, mu*, v), "jes_cov" (the candidate-optima stage and K* W), "jes" (the
 * combiner and the finish: two entries per chunk), "jes_agg" (U = -H W^T), "jes_grad" (P = C* o U and the optima term),
 * "jes_grad_gemm" (the second gradient contraction, P X~ or its raw-difference form); the tiled evaluation counts under its own names. */
typedef struct sls_jes sls_jes;
#define SLS_JES_MAX_OPTIMA 1024
/* x_star D x K, f_star K, 1 <= K <= SLS_JES_MAX_OPTIMA, all finite; star_noise >= 0 and finite: else SLS_ERR_INVALID. */
int sls_jes_create(sls_gp* gp, const double* x_star, const double* f_star, int K, double star_noise, sls_jes** out);
int sls_jes_destroy(sls_jes* j);
/* mu_star[k] = mu*_k, var_star[k] = v_k; either may be NULL. */
int sls_jes_optima(sls_jes* j, double* mu_star, double* var_star);
/* tau[i] = tau(t[i]), dtau[i] = tau'(t[i]); either out pointer may be NULL; n >= 0 (n < 0: SLS_ERR_INVALID).  A test hook, as
 * sls_mes_terms is. */
int sls_jes_terms(sls_ctx* ctx, const double* t, long n, double* tau, double* dtau);
/* alpha at the M points Xs (D x M): val (M), grad (D x M, may be NULL), cov (M x K column-major, cov[m + k*M] = c_k(x_m), may be NULL).
 * noise_var > 0 and finite, val != NULL when M > 0: else SLS_ERR_INVALID; M = 0 is a no-op. */
int sls_jes_eval(sls_jes* j, double noise_var, const double* Xs, int M, double* val, double* grad, double* cov);
/* sls_acq_maximize with alpha as the objective: same outputs, same semantics of idx_out / x_stars / y_stars; the statistics go to
 * sls_acq_last_stats of the handle. */
int sls_jes_maximize(sls_jes* j, double noise_var, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                     long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars);

/* ---- knowledge gradient on a discrete set (not in the reference) ----------------------------------------------------------
 * The library recommends the point of highest posterior mean; the knowledge gradient (Frazier, Powell & Dayanik 2009) values a
 * measurement at x by what it does to that recommendation, KG(x) = E_y[max_x' mu_{n+1}(x')] - max_x' mu_n(x'), with the inner maximum
 * over a finite set: K fixed points x_k, optionally plus the candidate itself (KGCP, Scott, Frazier & Powell 2011).
 * The object: K fixed points x_k, 1 <= K <= SLS_KG_MAX_POINTS, clamped into [0,1]^D at creation (as joint entropy search clamps its
 * optima); a_k = mu(x_k) is what sls_gp_predict's tiled route returns there, bit for bit; a_max = max_k a_k (the lowest k wins ties);
 * w_k = K_y^-1 k(X, x_k) from raw coordinate differences, as in sls_jes_create.
 * Per candidate x: mu, sigma from the tiled evaluation in the handle's sigma mode, formed as the gradient evaluations form them whether
 * or not grad is asked for; noise_var >= 0 and finite; c_k(x) = k(x, x_k) - k*(x)^T w_k as joint entropy search forms it.
 *   s      = sqrt(sigma sigma + noise_var)
 *   b_k    = c_k(x) / s                slope of the future mean at x_k per unit z:  mu_{n+1}(x_k) = a_k + b_k z,  z ~ N(0,1)
 *   include_self != 0 adds line K:   a_K = mu(x),   b_K = sigma sigma / s
 *   KG(x)  = E_z max_j (a_j + b_j z)  -  a_max
 * The baseline is the constant a_max of the fixed set, not max(a_max, mu(x)): the value is smooth in x, >= 0, and differs from KGCP by
 * max(0, mu(x) - a_max) only.
 * Evaluation (Frazier's algorithm): the lines ordered by (b ascending, a descending, index ascending); among equal slopes the first
 * stays; a stack scan leaves the envelope lines e_0 .. e_{E-1} with breakpoints t_1 < .. < t_{E-1},
 * t_i = (a_{e_{i-1}} - a_{e_i}) / (b_{e_i} - b_{e_{i-1}}), t_0 = -inf, t_E = +inf; a line whose breakpoint with the new line is <= its own
 * breakpoint is popped.
 *   E max - max_j a_j = sum_{i=1..E-1} (b_{e_i} - b_{e_{i-1}}) f(-|t_i|),   f(-t) = phi(t) - t Phi(-t), 0 at t = inf    (envelope order)
 *   KG                = that + (include_self ? max(0, mu - a_max) : 0)
 *   beta_j = dKG/db_j = phi(t_i) - phi(t_{i+1})   for j = e_i, 0 off the envelope
 *   pi_j   = dKG/da_j = Phi(t_{i+1}) - Phi(t_i)   for j = e_i, 0 off the envelope      (sum_j pi_j = 1)
 * Phi(-t) = erfc(t / sqrt 2) / 2; pi is a difference of the smaller tails: Phi(t_{i+1}) - Phi(t_i) for t_{i+1} <= 0, Phi(-t_i) -
 * Phi(-t_{i+1}) for t_i >= 0, (1 - Phi(t_i)) - Phi(-t_{i+1}) across 0.  E = 1 gives exactly 0, beta = 0, pi = 1.  Every product is rounded
 * on its own (no fused multiply-add in the combiner).
 * Gradient, of the shape of joint entropy search's (everything after the combiner is shared with it):
 *   grad KG = A_mu grad mu + A_sigma grad sigma + sum_k h_k grad c_k(x)
 *   h_k     = beta_k / s                   A_mu = pi_K  (0 without the self line)
 *   A_sigma = (beta_K (sigma sigma + 2 noise_var) - sum_k beta_k c_k) (sigma / s^3)          (the sum over k < K in increasing k)
 * Guard (expected improvement's, as joint entropy search applies it): sigma < 1e-10, or a NaN in the value or any gradient component:
 * value 0, gradient 0.  A NaN among a candidate's lines makes its value NaN before the guard.
 * The combiner works per candidate cooperatively (one workgroup per candidate: the lines sorted in LDS, the scan by one lane, the
 * weights by all lanes); the comparison is the total order above and both sums have one fixed order that depends on the candidate's
 * lines alone, so a point's bits depend on neither its column, the other points of the call, the candidate chunk nor active-set
 * compaction.  The object is a snapshot, as sls_jes is (W, the clamped points, a_k, a_max, sls_gp_generation): a call after the handle
 * was refitted, grown or switched in sigma mode returns SLS_ERR_INVALID.  It must not outlive its handle.  Every call holds the
 * context's lock for its whole length and always takes the tiled evaluation.
 * sls_prof_get names: "kg_setup" (create), "kg" (the combiner and the finish: two entries per chunk); the stages shared with joint
 * entropy search keep its names "jes_cov", "jes_agg", "jes_grad" and "jes_grad_gemm". */
typedef struct sls_kg sls_kg;
#define SLS_KG_MAX_POINTS 1024
/* x_ref D x K, 1 <= K <= SLS_KG_MAX_POINTS, all finite: else SLS_ERR_INVALID. */
int sls_kg_create(sls_gp* gp, const double* x_ref, int K, sls_kg** out);
int sls_kg_destroy(sls_kg* k);
/* mu_ref[k] = a_k, *mu_max = a_max, *arg_max = its (lowest) index; any may be NULL. */
int sls_kg_points(sls_kg* k, double* mu_ref, double* mu_max, int* arg_max);
/* KG at the M points Xs (D x M): val (M), grad (D x M, may be NULL), slope (M x K column-major, slope[m + k*M] = b_k(x_m), may be NULL).
 * noise_var >= 0 and finite, val != NULL when M > 0: else SLS_ERR_INVALID; M = 0 is a no-op. */
int sls_kg_eval(sls_kg* k, double noise_var, int include_self, const double* Xs, int M, double* val, double* grad, double* slope);
/* sls_acq_maximize with KG as the objective: same outputs, same semantics of idx_out / x_stars / y_stars; the statistics go to
 * sls_acq_last_stats of the handle. */
int sls_kg_maximize(sls_kg* k, double noise_var, int include_self, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                    long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars);
/* A test hook, as sls_jes_terms is: the combiner alone on caller-supplied lines.  a (K), B (M x K, [m + k*M]); a_self, b_self (M each,
 * both NULL or both given); val (M) = E max - max_k a_k (+ max(0, a_self - max_k a_k) with a self line); beta, prob (M x K), self_out
 * (M x 2: beta_K at [m], pi_K at [m + M]) may be NULL.  Every input finite, 1 <= K <= SLS_KG_MAX_POINTS: else SLS_ERR_INVALID. */
int sls_kg_lines(sls_ctx* ctx, const double* a, const double* B, const double* a_self, const double* b_self, int K, int M,
                 double* val, double* beta, double* prob, double* self_out);

/* ---- log expected improvement (not in the reference) -------------------------------------------------------------------
 * acq_type SLS_ACQ_LOG_EXPECTED_IMPROVEMENT, accepted wherever an acq_type is taken (sls_acq_eval, sls_acq_maximize,
 * sls_acq_maximize_dev, sls_acq_eval_pair, sls_acq_maximize_pair, sls_multi_acq_maximize); every returned value (val, val_out,
 * y_stars, the record gathered across GPUs) is then a LogEI value.  Expected improvement diff Phi + sigma phi underflows to exactly 0
 * with its gradient once u = (mu - mu_best) / sigma < ~-38.6 and cancels before that; LogEI = log EI is formed without Phi.
 * With mu, sigma as the tiled evaluation forms them in the handle's sigma mode (see max-value entropy search above), diff = mu -
 * mu_best, u = diff / sigma and r = phi / Phi as MES forms it:
 *   u <  0: e = erfcx(-u / sqrt 2), r = sqrt(2/pi) / e, log Phi = log(e / 2) - u^2 / 2;   u >= 0: Phi = erfc(-u / sqrt 2) / 2, r = phi / Phi
 *   w(u)     = h / Phi = r + u      direct for u >= -30; for u < -30 (r + u cancels to ~1/|u| and the direct form loses u^2 eps of it)
 *                                   w = (c - 1) / u, c = t (2 + t (-10 + t (74 + t (-706 + 8162 t)))), t = 1 / u^2 (the series of MES)
 *   log h(u) = log Phi + log w      (u < 0);    log(phi + u Phi)   (u >= 0, no cancellation),      h = phi + u Phi
 *   B1 = 1 / w (= Phi / h),  B2 = r / w (= phi / h)
 *   LogEI      = log sigma + log h(u)
 *   grad LogEI = (1 / sigma) (B1 grad mu + B2 grad sigma)
 * Guard (the conditions of expected improvement): sigma < 1e-10, or a NaN in the value or in any gradient component, gives the value
 * SLS_LOG_EI_FLOOR and the zero gradient.  The floor is finite on purpose: the Armijo test, the relative stopping tests and DIRECT's
 * rectangle selection stay in finite arithmetic; a start on the floor is stationary and leaves the batch, a trial step onto it is
 * rejected.  The guard looks for NaN only, as expected improvement's does: every result is finite for |u| < 1e154, which sigma >= 1e-10
 * gives for any |mu - mu_best| < 1e144; beyond that u^2 overflows, an infinite mu gives u = -inf, and the value is -inf (with an
 * infinite B1), which is not caught.  log h is accurate to a few eps max(1, u^2), B1 and B2 to ~2e-13 relative (the series' first omitted term at u = -30).
 * One lane per point and a fixed operation order: a point's bits depend on neither its column, the other points of the call nor the
 * candidate chunk.  LogEI always takes the tiled evaluation plus one combiner launch (never the single-launch path of small
 * problems, the zero-copy path or the evaluation slots) and holds the context's lock for the whole call, as the handle's other
 * large calls do. */
#define SLS_LOG_EI_FLOOR (-1.0e300)
/* log_h[i] = log h(u[i]), b1[i] = Phi / h, b2[i] = phi / h; any out pointer may be NULL; n >= 0 (n < 0: SLS_ERR_INVALID).  The scalar
 * terms on their own (a test hook, as sls_mes_terms is). */
int sls_logei_terms(sls_ctx* ctx, const double* u, long n, double* log_h, double* b1, double* b2);

/* ---- expected utility of the best option of a query pair (not in the reference) -----------------------------------------
 * EUBO for a pair, the q = 2 case of qEUBO (Astudillo et al., AISTATS 2023): EUBO(x, x') = E[ max(f(x), f(x')) ] under the
 * posterior, in closed form.  It is the one-step-optimal criterion for a two-option preference query and the only acquisition here
 * that uses the posterior covariance BETWEEN two candidates.  The handle has data X, theta = (a, l), K_y and alpha; a pair (x, x')
 * lies in [0,1]^D x [0,1]^D:
 *   k_x = k(X, x),  k_x' = k(X, x'),  d = k_x - k_x',  w = K_y^-1 d
 *   mu = k_x . alpha,  mu' = k_x' . alpha,  delta = mu - mu'
 *   s^2 = Var[f(x) - f(x')] = 2a - 2 k(x, x') - d^T K_y^-1 d      (latent covariance, no b on the diagonal: cov00 + cov11 - 2 cov01
 *                                                                   of sls_gp_predict_cov at the two points)
 *   u = delta / s,  Phi = erfc(-u / sqrt 2) / 2,  Phi' = erfc(u / sqrt 2) / 2,  phi = exp(-u^2 / 2) / sqrt(2 pi)
 *   EUBO = mu Phi + mu' Phi' + s phi
 * Gradients, with dk(x, x_i)/dx_d = -c_i (x~_d - x~_i,d) inv_ell_d, x~ = (x - 0.5) o inv_ell, and c12 the derivative weight of
 * k(x, x'):
 *   T_x,d   = inv_ell_d ( x~_d sum_i c_x,i w_i - sum_i c_x,i w_i x~_i,d ),   T_x',d likewise with c_x', x~'
 *   e_d     = c12 (x~_d - x~'_d) inv_ell_d
 *   ds^2/dx_d = 2 e_d + 2 T_x,d         ds^2/dx'_d = -2 e_d - 2 T_x',d
 *   grad_x EUBO  = Phi  grad mu(x)  + phi grad_x  s^2 / (2 s)
 *   grad_x' EUBO = Phi' grad mu(x') + phi grad_x' s^2 / (2 s)
 * Guard: !(s^2 > 0), or s < 1e-10, or a NaN in the value or in any of the 2D gradient components, gives the value fmax(mu, mu') --
 * the limit as s -> 0 -- and the zero gradient (of all 2D components).  A collapsed pair (x = x') is therefore stationary and leaves
 * the maximiser's batch, as the guarded points of expected improvement do.  The gradient is formed, and looked at by the guard,
 * whether or not it is asked for: a pair's value does not depend on that.
 * No log form is needed: far below the other option (|u| >~ 38) Phi or Phi' is exactly 0 and that option gets no mean gradient, but
 * the value carries the other option's mean itself and stays correct.
 * w and d^T K_y^-1 d are formed from d exactly as the tiled evaluation forms K_y^-1 k and k^T K_y^-1 k from k in the handle's sigma
 * mode: the explicit inverse (mode 0), or |L^-1 d|^2 and w = L^-T (L^-1 d) (mode 1, the handles of a PreferenceRegressor).
 * The value's three products and two sums are separate operations (no fused multiply-add), and every other operation is symmetric
 * in the two options: (x, x') and (x', x) give values within the rounding of the final sum and mirrored gradients.
 * One lane per pair and fixed summation orders: a pair's bits depend on neither its column, the other pairs of the call, the
 * candidate chunk nor SLS_COMPACT.  Both calls always take the tiled evaluation (never the single-launch path of small problems,
 * the zero-copy path or the evaluation slots) and hold the context's lock and the handle's state lock (shared) for the whole call.
 * Per pass max(128, candidate chunk / 2 rounded down to 128) pairs are evaluated (sls_ctx_set_candidate_chunk). */
/* pairs: 2D x M column-major, rows 0..D-1 = x, D..2D-1 = x'.  val (M, may be NULL), grad (2D x M, may be NULL).  M = 0 is a no-op;
 * a NULL handle, NULL pairs or M < 0 is SLS_ERR_INVALID. */
int sls_eubo_eval(sls_gp* gp, const double* pairs, int M, double* val, double* grad);
/* sls_acq_maximize over [0,1]^(2D) with EUBO as the objective: starts 2D x S, x_out 2D, x_stars 2D x S; idx_out / y_stars /
 * start_index_offset / sls_acq_last_stats as sls_acq_maximize.  S < 1 or n_local < 1 is SLS_ERR_INVALID. */
int sls_eubo_maximize(sls_gp* gp, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                      long start_index_offset, double* x_out, double* val_out, long* idx_out,
                      double* x_stars, double* y_stars);

/* ---- expected utility of the best of q options on posterior draws (not in the reference) -----------------------------------
 * qEUBO (Astudillo et al., AISTATS 2023) for any number of options: E[ max_i f(x_i) ] has no closed form beyond q = 2; the estimator
 * is a sample average over FIXED posterior draws, maximised as a deterministic function.  The draws are those of a path object p
 * (n_draws = S draws f_s, F frequencies): they share one feature basis and are linear in their weights (W, V).  For a set of q
 * options (x_0..x_{q-1}), each in [0,1]^D:
 *   v_{i,s} = f_s(x_i)                                  (the function sls_path_eval evaluates; formed here on tile GEMMs, see below)
 *   i*(s)   = the LOWEST i with v_{i,s} = max_j v_{j,s}  (strictly-greater scan over i = 0..q-1: first wins on ties)
 *   wins_i  = #{ s : i*(s) = i }
 *   qEUBO   = ( sum_s v_{i*(s),s} ) / S                  (one lane per set, from zero, increasing s, ONE division at the end)
 *   m_i     = 0/1 indicator vector of { s : i*(s) = i }  (length S; padded draws are 0)
 *   Wbar_i  = W m_i  (2F),   Vbar_i = V m_i  (N)         (aggregated weights: plain sums of the winners' columns)
 *   grad_{x_i} qEUBO = ( grad fbar_i(x_i) ) / S,  fbar_i = the path function with weights (Wbar_i, Vbar_i)
 * An option that wins no draw gets an exactly zero gradient; q = 1 gives the mean of the draws.  wins_i / S estimates the probability
 * that the user picks option i.
 * Guard: a NaN among the set's q S values or its qD gradient components gives the value SLS_QEUBO_FLOOR (finite for the reasons
 * SLS_LOG_EI_FLOOR is) and the zero gradient.  The gradient is formed, and looked at by the guard, whether or not it is asked for.
 * Route per pass: cross_gram for the q points of every set; every draw at every point as Phi^T W + K* V on the tile GEMM (so the
 * summation order differs from sls_path_eval's gathered data term: the two agree to rounding, not to the bit); one lane per set picks
 * the winners and writes the 0/1 mask; Wbar = W mask and Vbar = V mask on the tile GEMM (depth n_draws); the gathered route of
 * sls_path_eval on (Wbar, Vbar) gives grad fbar_i(x_i).  No q x q factorisation per set.
 * A set's bits depend on neither its column, the other sets of the call, the number of sets per pass nor SLS_COMPACT.  Permuting the
 * options of a set permutes wins and the gradient blocks and leaves the value's bits unchanged.
 * Sets per pass: points = min(candidate chunk (sls_ctx_set_candidate_chunk, counted in POINTS), 2^26 / max(Rp, Np + 2 Fp)) with Np, Fp,
 * Rp = N, F, n_draws rounded up to 128 -- every block of a pass (values and mask: points x Rp; Wbar, Vbar; K*, C*, [Pm | G]) stays
 * below 2^26 doubles -- and sets = max(128, points / q rounded down to 128).  The floor of 128 sets (one tile) is the one exception to
 * both bounds: a pass then holds 128 q points whatever the candidate chunk or the 2^26 rule say (a chunk below 128 q; or q = 16 with
 * Np + 2 Fp > 32768), and its blocks may exceed 2^26 doubles (at most 2048 points; indices are 64-bit).
 * Locks are those of sls_path_eval / sls_path_maximize; a path whose handle was refitted, grown or switched in sigma mode is refused
 * (SLS_ERR_INVALID), as by the other sls_path_* calls. */
#define SLS_QEUBO_MAX_OPTIONS 16
#define SLS_QEUBO_FLOOR (-1.0e300)
/* sets: qD x M column-major, rows iD..iD+D-1 = option i.  val (M), grad (qD x M), wins (q x M ints): each may be NULL.  M = 0 is a
 * no-op; q outside 1..SLS_QEUBO_MAX_OPTIONS, M < 0, NULL p or NULL sets is SLS_ERR_INVALID. */
int sls_qeubo_eval(sls_path* p, int q, const double* sets, int M, double* val, double* grad, int* wins);
/* sls_acq_maximize over [0,1]^(qD) with qEUBO as the objective: starts qD x S_starts, x_out qD, x_stars qD x S_starts; idx_out /
 * y_stars / start_index_offset / sls_acq_last_stats (of the path's handle) as sls_acq_maximize.  S_starts < 1 or n_local < 1 is
 * SLS_ERR_INVALID. */
int sls_qeubo_maximize(sls_path* p, int q, const double* starts, int S_starts, int n_local, const sls_lbfgs_opts* opts,
                       long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars);

/* ---- noisy expected improvement on posterior draws (not in the reference) -------------------------------------------------
 * qNEI (Letham et al., Bayesian Analysis 2019), the joint improvement of a batch of q points over an incumbent that is itself
 * uncertain -- the targets of a PreferenceRegressor are MAP estimates of a latent function, so the best value seen so far is not a
 * known number.  The estimator is a sample average over the FIXED draws of a path object p (n_draws = S draws f_s), with the incumbent
 * taken per draw, from the same draw that evaluates the candidates:
 *   t_s     = max_j f_s(X_j)                              (sls_path_max_over_points at the data, or any point set; any finite
 *                                                          baseline may be passed: a constant one gives Monte-Carlo qEI)
 *   v_{i,s} = f_s(x_i)                                    (formed as by sls_qeubo_eval: Phi^T W + K* V on the tile GEMM)
 *   per draw, the scan  best = t_s, arg = none; for i = 0..q-1: if v_{i,s} > best then best = v_{i,s}, arg = i
 *   wins_i  = #{ s : arg(s) = i }                         (sum_i wins_i <= S: a draw that nobody improves has no winner)
 *   qNEI    = ( sum_s (best_s - t_s) ) / S                (one lane per set, from zero, increasing s, ONE division; a draw without
 *                                                          a winner adds exactly +0)
 *   m_i     = 0/1 indicator vector of { s : arg(s) = i }  (the column of a draw without a winner is all zero)
 *   grad_{x_i} qNEI = ( grad fbar_i(x_i) ) / S,  fbar_i = the path function with weights (W m_i, V m_i), exactly as qEUBO forms it
 * An option that wins no draw has an exactly zero gradient; a set that no draw improves has the value exactly 0 and the zero gradient.
 * Guard: a NaN among the set's q S values or its qD gradient components gives the value 0 and the zero gradient (expected
 * improvement's guard; the value is bounded below by 0, so no floor constant is needed).  The gradient is formed, and looked at by
 * the guard, whether or not it is asked for.
 * The pass, its route, the sets per pass and the bit contract are sls_qeubo_eval's (one pass function, the selection kernel apart): a
 * set's bits depend on neither its column, the other sets of the call, the number of sets per pass nor SLS_COMPACT; permuting the
 * options of a set permutes wins and the gradient blocks and leaves the value's bits unchanged.
 * A start set that no draw improves is stationary (value 0, zero gradient) and leaves the maximiser's batch at once, as expected
 * improvement's underflowed starts do; sls_qlognei_eval / sls_qlognei_maximize below are the log form, which has a gradient there.
 * Locks are those of sls_path_eval / sls_path_maximize; a path whose handle was refitted, grown or switched in sigma mode is refused
 * (SLS_ERR_INVALID), as by the other sls_path_* calls. */
/* t_out[s] = max_j f_s(Xb[:, j]), arg_out[s] = the LOWEST j that attains it; s < n_draws, Xb is D x Mb (host), Mb >= 1.  The values
 * are formed on the every-draw route of the qEUBO pass (Phi^T W + K* V on the tile GEMM), in passes of points bounded as that pass
 * bounds the points of one-option sets (candidate chunk, 2^26 rule, whole 128-point tiles); a running (max, argmax) per draw is merged
 * across the passes, and only the live rows of the last pass take part.  Either out pointer may be NULL.  A NaN among a draw's Mb
 * values gives t_out[s] = NaN, arg_out[s] = -1.  Max and lowest-index argmax do not depend on order: the result's bits depend on
 * neither the pass split, the launch geometry nor the position of a point among the others (beyond the index reported).  There is no
 * NULL-means-data shortcut: the handle keeps only scaled data on the device, so the caller passes X.  Mb < 1, NULL p or NULL Xb is
 * SLS_ERR_INVALID. */
int sls_path_max_over_points(sls_path* p, const double* Xb, int Mb, double* t_out, int* arg_out);
/* baseline: n_draws host doubles, uploaded once per call; all must be finite (else SLS_ERR_INVALID).  sets, val, grad, wins, q and M
 * as sls_qeubo_eval. */
int sls_qnei_eval(sls_path* p, int q, const double* baseline, const double* sets, int M, double* val, double* grad, int* wins);
/* sls_qeubo_maximize with this objective; the baseline is validated and uploaded once, before the first round. */
int sls_qnei_maximize(sls_path* p, int q, const double* baseline, const double* starts, int S_starts, int n_local,
                      const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                      double* x_stars, double* y_stars);

/* ---- log-space noisy expected improvement on posterior draws (not in the reference) -----------------------------------------
 * qLogNEI: the log form of the criterion above after Ament et al. (NeurIPS 2023, qLogEI) -- a softplus for the ReLU, a temperature
 * log-sum-exp for the max over the q points, a log-sum-exp over the draws.  It is smooth, and a set that no draw improves keeps a
 * finite value and a nonzero gradient.  For a path object p (S = n_draws draws), a per-draw baseline t_s, temperatures
 * tau_relu = T0 > 0 and tau_max = Tm > 0, and a set of q points:
 *   a_{i,s} = (v_{i,s} - t_s) / T0                        v_{i,s} = f_s(x_i), formed exactly as sls_qnei_eval forms it
 *   L(a)    = log softplus(a):   a >= 0       : log(a + log1p(exp(-a)))
 *                                -36 <= a < 0 : log(log1p(exp(a)))
 *                                a < -36      : a                      (the neglected term is < exp(-36)/2)
 *   R(a)    = dL/da:             a >= 0       : 1 / ((1 + exp(-a)) (a + log1p(exp(-a))))
 *                                -36 <= a < 0 : exp(a) / ((1 + exp(a)) log1p(exp(a)))
 *                                a < -36      : 1
 *   l_{i,s} = log T0 + L(a_{i,s}),   rho_{i,s} = R(a_{i,s}) / T0
 *   m_s     = Mq_s + Tm log sum_i exp((l_{i,s} - Mq_s)/Tm),  Mq_s = max_i l_{i,s};   pi_{i,s} = exp((l_{i,s} - Mq_s)/Tm) / (that sum)
 *   value   = Mx + log sum_s exp(m_s - Mx) - log S,  Mx = max_s m_s;   omega_s = exp(m_s - Mx) / (that sum)
 *   c_{i,s} = omega_s pi_{i,s} rho_{i,s}                  (= d value / d v_{i,s}; all > 0 before rounding: a factor pi or omega more
 *                                                          than 745 below its maximum underflows to 0)
 *   grad_{x_i} value = grad fbar_i(x_i),  fbar_i = the path function with weights (W c_i, V c_i)      -- no division by S
 *   wins_i  = sls_qnei_eval's wins (hard, strictly-greater against t_s), bit for bit
 * The sum over i does not depend on the order of the options: Mq_s is taken at the largest v_{i,s}, every term lies in [0, 1] and is
 * rounded to a multiple of 2^-58, and the terms are added as 64-bit integers (q <= 16 of them stay below 2^62; the sum is >= 1, so this
 * rounding moves it by less than eps / 4 relative).  The log-sum-exp over the draws is accumulated online (a running maximum, the sum
 * rescaled when the maximum moves), over s increasing inside slices of 16 draws, over the slices increasing.
 * Bounds: qNEI <= exp(value) <= q^Tm (qNEI + T0 ln 2), from softplus in [relu, relu + T0 ln 2] and log-sum-exp in [max, max + Tm ln q].
 * Guard: a NaN among the set's q S values or its qD gradient components gives the value SLS_QEUBO_FLOOR and the zero gradient; the
 * scan runs before any write and whether or not the gradient is asked for.
 * Bits: a set's value, gradient and wins depend on neither its column, the other sets of the call, the number of sets per pass nor
 * SLS_COMPACT.  Permuting the options of a set permutes wins and the gradient blocks exactly, because the sum over i above has no order and
 * the draws keep theirs; for the value, rely on no more than unchanged to rounding.
 * tau_relu or tau_max not finite or <= 0, and a non-finite baseline, are SLS_ERR_INVALID (checked once per call, before any upload);
 * q, M, NULL arguments, locks and the staleness rule are as sls_qnei_eval.  The slider form (sls_line_*) has no log variant. */
#define SLS_QLOGNEI_TAU_RELU 1e-6
#define SLS_QLOGNEI_TAU_MAX 1e-2
/* L[i] = L(a[i]), R[i] = R(a[i]) for i < n on the device of ctx (a test hook, as sls_logei_terms is); either output may be NULL. */
int sls_qlognei_terms(sls_ctx* ctx, const double* a, long n, double* L, double* R);
int sls_qlognei_eval(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* sets, int M,
                     double* val, double* grad, int* wins);
/* sls_qnei_maximize with this objective; temperatures and baseline are validated once, before the first round. */
int sls_qlognei_maximize(sls_path* p, int q, const double* baseline, double tau_relu, double tau_max, const double* starts,
                         int S_starts, int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out,
                         double* val_out, long* idx_out, double* x_stars, double* y_stars);

/* ---- information gain of a choice query on posterior draws (not in the reference) -------------------------------------------
 * qBALD: the mutual information between the user's answer to a q-option choice query and the latent function (Houlsby et al. 2011,
 * "Bayesian active learning by disagreement", there for pairs), under the Bradley-Terry-Luce likelihood the preference model is fitted
 * with (PreferenceRegressor's btl_scale; CalcBtl of the reference).  Where qEUBO asks where the best option probably is, this asks
 * which query teaches the model most; its by-product is the predicted choice probability of every option, the quantity a held-out
 * preference log-loss is computed from.  For a path object p (S = n_draws draws f_s), a BTL scale tau > 0 and a set of q options:
 *   v_{i,s}  = f_s(x_i)                                  formed exactly as sls_qeubo_eval forms it
 *   z_{i,s}  = (v_{i,s} - max_j v_{j,s}) / tau           subtract first, then divide: <= 0, exactly 0 at the largest value
 *   Z_s      = sum_i exp(z_{i,s})                        the order-free sum of sls_qlognei_eval: terms in [0,1] rounded to multiples of
 *                                                        2^-58, added as 64-bit integers; Z_s >= 1
 *   p_{i,s}  = exp(z_{i,s}) / Z_s                        the BTL probability that option i is chosen under draw s
 *   pbar_i   = ( sum_s p_{i,s} ) / S                     from zero, s increasing inside slices of 16 draws, slices increasing, ONE
 *                                                        division: the predicted choice probability of option i (prob)
 *   l_{i,s}  = log p_{i,s} - log pbar_i                  both logarithms of the numbers as formed; taken as 0 where p_{i,s} = 0
 *   KL_s     = sum_i p_{i,s} l_{i,s}                     a signed sum in increasing i
 *   value    = ( sum_s KL_s ) / S                        = H(pbar) - mean_s H(p_s) = I(choice; f); the same fixed order over s
 *   c_{i,s}  = p_{i,s} (l_{i,s} - KL_s) / (S tau)        = d value / d v_{i,s};  sum_i c_{i,s} = 0 for every draw
 *   grad_{x_i} value = grad fbar_i(x_i),  fbar_i = the path function with weights (W c_i, V c_i)      -- no further division
 *   wins_i   = sls_qeubo_eval's wins (hard, strictly greater, lowest index on ties), bit for bit
 * The criterion is smooth everywhere.  0 <= value <= ln q to rounding (the value may be -O(eps)).  q = 1 gives value and gradient
 * exactly 0 and prob exactly 1; S = 1 gives value and gradient exactly 0, because l is then exactly 0; an option with pbar_i = 0
 * gets an exactly zero gradient block; sum_i prob_i = 1 to q eps.
 * The saturated regime: when tau is far below the spread of the draws at the options, every p_s is one-hot, the value tends to the
 * entropy of the win frequencies wins / S, and the weights tend to 0 because l - KL_s vanishes at the winner.  Such a start is
 * stationary and leaves the maximiser's batch, as a start with expected improvement exactly 0 does.  That is a property of the
 * criterion -- with a near-deterministic user every query whose winner is uncertain is worth the same one answer -- not of the
 * estimator.
 * Guard: a NaN among the set's q S values or its qD gradient components gives the value SLS_QEUBO_FLOOR, the zero gradient, a zero prob
 * column, and wins as sls_qeubo_eval reports them for that set; the scan runs before any write and whether or not the gradient is
 * asked for.
 * Bits: a set's value, gradient, prob and wins depend on neither its column, the other sets of the call, the number of sets per pass
 * nor SLS_COMPACT.  Permuting the options of a set permutes wins and prob exactly (Z_s has no order and each pbar_i has its own fixed
 * order over s); KL_s is a signed sum over the options in index order, so the value and the gradient are unchanged to rounding only.
 * scale not finite, <= 0 or subnormal is SLS_ERR_INVALID (checked once per call, before any upload); q, M, NULL arguments, M = 0, the
 * locks and the staleness rule are as sls_qeubo_eval.  The slider and gallery forms have no such variant. */
#define SLS_QBALD_SCALE 0.010 /* the reference's default btl_scale */
/* prob: q x M column-major, prob[i + n q] = pbar_i of set n.  val, grad, prob and wins may each be NULL. */
int sls_qbald_eval(sls_path* p, int q, double scale, const double* sets, int M, double* val, double* grad, double* prob, int* wins);
/* sls_qeubo_maximize with this objective; the scale is validated once, before the first round. */
int sls_qbald_maximize(sls_path* p, int q, double scale, const double* starts, int S_starts, int n_local, const sls_lbfgs_opts* opts,
                       long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars, double* y_stars);

/* ---- expected utility of the best slider position on posterior draws (not in the reference) --------------------------------
 * Line EUBO: the query of SequentialLineSearchOptimizer is a slider from a to b, and the user picks the best point anywhere on it.
 * The one-step criterion of that query is E[ max_t f((1-t) a + t b) ], estimated on a grid of q positions over the FIXED draws of a
 * path object p.  A line is its ends (a, b), each in [0,1]^D, with SLS_LINE_MIN_POSITIONS <= q <= SLS_QEUBO_MAX_OPTIONS:
 *   u_i = (q-1-i)/(q-1),  t_i = i/(q-1)             (each ONE double division of two exact integers, on the device)
 *   x_i = u_i a + t_i b,  i = 0..q-1                (two products and one sum per coordinate, separate roundings, NO fused
 *                                                    multiply-add, no clamp: Slider::GetValue on the grid; x_0 = a, x_{q-1} = b)
 *   value  = sls_qeubo_eval at the set (x_0..x_{q-1}); with a per-draw baseline (n_draws finite doubles) sls_qnei_eval at it
 *   wins_i = as there: wins_i / n_draws estimates the probability that the user stops at position i
 *   grad_a = sum_i u_i g_i,  grad_b = sum_i t_i g_i  (g_i = the set gradient's block of option i; product and sum separate roundings;
 *                                                    grad_a from zero in INCREASING i, grad_b from zero in DECREASING i -- the
 *                                                    mirror image of grad_a's order, which is what makes the mirror contract below
 *                                                    hold to the bit: one order for both cannot, a sum of q > 3 terms depends on it)
 * Guard: the set's guard passes through -- a guarded set gives SLS_QEUBO_FLOOR (0 with a baseline) and an exactly zero line gradient.
 * Anchored form: with `anchor` (D host doubles, all finite, else SLS_ERR_INVALID; uploaded once per call) a = anchor for every line of
 * the call, a line is b alone (D variables) and only grad_b is returned.  This is the slider through x+.
 * Contract:
 *   - A line's value and wins are bit for bit those of sls_qeubo_eval / sls_qnei_eval at the expanded set, and its gradient is bit for
 *     bit the fold above of that call's gradient.
 *   - A line's bits depend on neither its column, the other lines of the call, the lines per pass nor SLS_COMPACT.
 *   - Mirror symmetry: swapping a and b leaves the value's bits unchanged, reverses wins and swaps the two gradient blocks, with or
 *     without a baseline: u_i = t_{q-1-i} to the bit and the sum of two products commutes, so the expanded set is the reversed set bit
 *     for bit, and the permutation contract of sls_qeubo_eval gives the reversed set gradient bit for bit; the swapped line's grad_b
 *     then adds, in decreasing i, exactly the products this line's grad_a adds in increasing i (and the other way round), so the
 *     blocks swap bit for bit for every q.
 *   - Degenerate line a = b: wherever the expansion reproduces a at every position (always for q = 2 and q = 3, where the weights are
 *     0, 1/2, 1; for other q whenever u_i a + t_i a rounds back to a in every coordinate, e.g. coordinates with few mantissa bits and
 *     q - 1 a power of two) all options tie, position 0 wins every draw, grad_b is exactly zero and grad_a = g_0.  Elsewhere the
 *     positions differ from a by a rounding and an inner position may win a draw by that much.
 * Route per pass: line_expand (lines -> the candidate-major set block), ONE pass of the qEUBO evaluation unchanged, line_fold (set
 * gradient -> line gradient).  Lines per pass are the sets per pass of sls_qeubo_eval, and the expanded sets and their gradient are
 * held for one pass only (qD x pass doubles each, never qD x M).  The maximiser runs L-BFGS over 2D variables (D anchored) whatever q.
 * Locks and the staleness rule are those of sls_qeubo_eval. */
#define SLS_LINE_MIN_POSITIONS 2
/* lines: (anchor ? D : 2D) x M column-major, rows 0..D-1 = a (free form), last D rows = b.  baseline NULL: EUBO form; else n_draws
 * finite doubles.  val (M), grad ((anchor ? D : 2D) x M), wins (q x M ints): each may be NULL.  M = 0 is a no-op; q outside
 * SLS_LINE_MIN_POSITIONS..SLS_QEUBO_MAX_OPTIONS, M < 0, NULL p, NULL lines, a non-finite anchor or baseline is SLS_ERR_INVALID. */
int sls_line_eval(sls_path* p, int q, const double* baseline, const double* anchor, const double* lines, int M,
                  double* val, double* grad, int* wins);
/* sls_qeubo_maximize over [0,1]^(2D) (or [0,1]^D anchored) with this objective: starts, x_out, x_stars have 2D (D) rows; the other
 * outputs and sls_acq_last_stats as there.  Anchor and baseline are validated and uploaded once, before the first round.  S_starts < 1
 * or n_local < 1 is SLS_ERR_INVALID. */
int sls_line_maximize(sls_path* p, int q, const double* baseline, const double* anchor, const double* starts, int S_starts,
                      int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                      long* idx_out, double* x_stars, double* y_stars);

/* ---- expected utility of the best gallery cell on posterior draws (not in the reference) -------------------------------------
 * Gallery EUBO: the query of the sequential gallery (Koyama et al. 2020) is a two-dimensional patch of designs shown as a grid, and
 * the user picks the best cell.  The one-step criterion of that query is E[ max_{s,t} f(x(s,t)) ], estimated on a qs x qt grid of the
 * bilinear patch spanned by four corners over the FIXED draws of a path object p -- line EUBO (above) one dimension up.
 * Patch and grid: a patch is its corners c00, c10, c01, c11, each in [0,1]^D; qs >= SLS_PATCH_MIN_POSITIONS, qt >=
 * SLS_PATCH_MIN_POSITIONS and qs qt <= SLS_QEUBO_MAX_OPTIONS cells.  The weights are the line's along each axis, each ONE double
 * division of two exact integers, on the device:
 *   u_i = (qs-1-i)/(qs-1),  s_i = i/(qs-1),  v_j = (qt-1-j)/(qt-1),  t_j = j/(qt-1)
 * Expansion: option k = i + qs j is
 *   lo = u_i c00 + s_i c10,  hi = u_i c01 + s_i c11,  x_k = v_j lo + t_j hi
 * each of the three two products and one sum per coordinate, rounded separately, NO fused multiply-add, no clamp.  The patch is
 * bilinear: every cell is a convex combination of the corners, so it lies in the cube whenever the corners do; cells (0,0), (qs-1,0),
 * (0,qt-1), (qs-1,qt-1) are c00, c10, c01, c11 exactly.  The patch is planar exactly when c11 = c10 + c01 - c00.
 *   value  = sls_qeubo_eval at the expanded set of q = qs qt options; with a per-draw baseline (n_draws finite doubles)
 *            sls_qnei_eval at it
 *   wins   = as there, (qs qt) x M, indexed by k: wins_k / n_draws estimates the probability that the user picks cell k
 * Fold: with g_k the set gradient's block of option k, per grid row j
 *   A_j = sum_i u_i g_{i + qs j}  from zero in INCREASING i,   B_j = sum_i s_i g_{i + qs j}  from zero in DECREASING i
 *   grad_c00 = sum_j v_j A_j,  grad_c10 = sum_j v_j B_j        from zero in INCREASING j
 *   grad_c01 = sum_j t_j A_j,  grad_c11 = sum_j t_j B_j        from zero in DECREASING j
 * every step a product and a sum rounded separately.  The orders are the line's along each axis: the sums with the weights that fall
 * along an axis run up it, those with the weights that rise run down it, so that a mirror of the axis maps each sum onto its partner
 * term by term.
 * Guard: the set's guard passes through -- a guarded set gives SLS_QEUBO_FLOOR (0 with a baseline) and an exactly zero patch gradient.
 * Anchored form: with `anchor` (D host doubles, all finite, else SLS_ERR_INVALID; uploaded once per call) c00 = anchor for every patch
 * of the call, a patch is (c10, c01, c11) (3D variables) and only those three gradients are returned.  This is the gallery with the
 * current best point x+ in its corner.
 * Contract:
 *   - A patch's value and wins are bit for bit those of sls_qeubo_eval / sls_qnei_eval at the expanded set, and its gradient is bit
 *     for bit the fold above of that call's gradient.
 *   - A patch's bits depend on neither its column, the other patches of the call, the patches per pass nor SLS_COMPACT.
 *   - s-mirror (c00 <-> c10, c01 <-> c11) and t-mirror (c00 <-> c01, c10 <-> c11): the value's bits are unchanged, wins are reversed
 *     along i (along j), and the gradient blocks swap the same way, bit for bit, with or without a baseline (ties aside: a tie goes to
 *     the lowest k on either side).
 *   - Transposition (c10 <-> c01 together with qs <-> qt) describes the same cells but is NOT bit-exact: the two nestings of the
 *     expansion round differently, so value and gradient agree to rounding only.
 *   - Degenerate rows: with qt = 2, c01 = c00, c11 = c10 the two grid rows are the same points bit for bit (the weights along t are
 *     exactly 0 and 1), every draw's winner lies in row 0, and the value is bit for bit sls_line_eval of the line (c00, c10) with q =
 *     qs, wins of row 0 are the line's and wins of row 1 are zero, (grad_c00, grad_c10) are the line's (grad_a, grad_b) bit for bit and
 *     grad_c01, grad_c11 are exactly zero.
 * Route per pass: patch_expand (patches -> the candidate-major set block), ONE pass of the qEUBO evaluation unchanged, patch_fold (set
 * gradient -> patch gradient).  Patches per pass are the sets per pass of sls_qeubo_eval for q = qs qt, and the expanded sets and
 * their gradient are held for one pass only.  The maximiser runs L-BFGS over 4D variables (3D anchored) whatever the grid.  Locks
 * and the staleness rule are those of sls_qeubo_eval.
 * Out of scope: grids above SLS_QEUBO_MAX_OPTIONS = 16 cells (the selection kernels are written for that limit and the pass-size
 * rules are stated for it; a finer gallery is shown by the caller zooming -- a sub-patch is again four corners); a log form; _sub
 * forms; sls_multi_*; and the centre-anchored parallelogram of the 2020 paper as a SEARCH parametrisation (its reflected corners can
 * leave the cube; sls_patch_eval scores any four corners, so such a gallery can be evaluated). */
#define SLS_PATCH_MIN_POSITIONS 2
/* patches: (anchor ? 3D : 4D) x M column-major, rows in blocks of D: c00 (free form only), c10, c01, c11.  baseline NULL: EUBO form;
 * else n_draws finite doubles.  val (M), grad ((anchor ? 3D : 4D) x M, the blocks of patches), wins ((qs qt) x M ints): each may be
 * NULL.  M = 0 is a no-op; qs or qt below SLS_PATCH_MIN_POSITIONS, qs qt > SLS_QEUBO_MAX_OPTIONS, M < 0, NULL p, NULL patches, a
 * non-finite anchor or baseline is SLS_ERR_INVALID, checked before any launch. */
int sls_patch_eval(sls_path* p, int qs, int qt, const double* baseline, const double* anchor, const double* patches, int M,
                   double* val, double* grad, int* wins);
/* sls_qeubo_maximize over [0,1]^(4D) (or [0,1]^(3D) anchored) with this objective: starts, x_out, x_stars have 4D (3D) rows; the
 * other outputs and sls_acq_last_stats as there.  Anchor and baseline are validated and uploaded once, before the first round.
 * S_starts < 1 or n_local < 1 is SLS_ERR_INVALID. */
int sls_patch_maximize(sls_path* p, int qs, int qt, const double* baseline, const double* anchor, const double* starts, int S_starts,
                       int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                       long* idx_out, double* x_stars, double* y_stars);

/* ---- maximisation over affine subspaces: boxes, lines, embeddings (not in the reference) ---------------------------------
 * Every maximiser above searches [0,1]^D.  Trust regions (x = lo + diag(hi - lo) z), line and plane searches (x = a + (b - a) z)
 * and random embeddings (x = c + A z, d << D) all search the affine image of a small box instead.  The *_sub entry points take the
 * VARIABLES z in [0,1]^d, 1 <= d <= D, and a set of maps; a column (a query point, a start) with map k stands for the point
 *   x = c_k + A_k z.
 * Arithmetic (part of the contract: numpy restates it to the bit):
 *   expand  x_r = c_r, then for j = 0..d-1 in increasing order  x_r = x_r + (A_rj z_j);    no clamp
 *   fold    gz_j = 0,  then for r = 0..D-1 in increasing order  gz_j = gz_j + (A_rj gx_r)
 * the product and the sum of every step rounded separately (never fused).  Between the two, the evaluation of the corresponding
 * plain call runs unchanged on the expanded points: val is bit for bit what sls_acq_eval / sls_mes_eval / sls_path_eval return at
 * X_out, grad_z the fold of their gradient.  A column's bits depend only on its own z and its own map -- not on the column it sits
 * in, the tile, the compaction of the maximiser or the other maps.
 * The maximisers clamp z to [0,1]^d exactly as the plain ones clamp x (the step kernels are the same); nothing requires the image
 * to lie in [0,1]^D: the evaluations are defined on all of R^D and do not clamp.  (The host layer's constructors, SearchSubspace::Box /
 * Segment / Centered, only produce maps whose image is inside the cube.)
 * SLS_ERR_INVALID, checked on the host before any launch: a struct_size other than sizeof(sls_submaps), d < 1 or d > D, n_maps < 1,
 * a NULL A or c, a non-finite entry of A or c, a map_of_column entry outside [0, n_maps).  M = 0 is a no-op.  Locks, generation
 * checks (sls_path) and sls_acq_last_stats behave exactly as in the corresponding plain call.
 * These routes NEVER take the one-wavefront kernel of small problems, the evaluation slots or the zero-copy path: always the tiled
 * evaluation, as LogEI does (compare against plain calls under SLS_WAVE_PATH=0 when bits matter).
 * Memory: A, c and map_of_column are uploaded once per call into one device block (8 n_maps D (d + 1) + 4 columns bytes); the expanded
 * points and their gradient are two blocks of D x round_up(columns, 128) doubles, kept with the handle (sls_acq_*_sub, sls_mes_*_sub)
 * or taken from the device pool for the call (sls_path_*_sub).
 * Profiler scopes: "sub_expand" and "sub_fold", one launch each per evaluation / per round of a maximiser (plus one "sub_expand" for
 * x_out / x_stars); everything between them counts as in the plain call.
 * Out of scope: the pair and set criteria (sls_eubo_*, sls_qeubo_*, sls_qnei_*, sls_qlognei_*, sls_line_*, sls_patch_*),
 * sls_acq_maximize_pair, sls_acq_maximize_dev and sls_multi_* have no _sub form. */
typedef struct sls_submaps {
    int struct_size;            /* sizeof(sls_submaps) as the caller's header declares it, as sls_lbfgs_opts */
    int d;                      /* variables per column, 1 <= d <= D */
    int n_maps;                 /* >= 1 */
    const double* A;            /* n_maps blocks of D x d, column-major: A_k[r + j*D] */
    const double* c;            /* n_maps blocks of D */
    const int* map_of_column;   /* one entry per point / start, in [0, n_maps); NULL: every column uses map 0 */
} sls_submaps;
/* sls_acq_eval at x = c + A z: Z is d x M; val (M); grad_z (d x M, may be NULL); X_out (D x M, may be NULL) = the expanded points.
 * All three acquisition types. */
int sls_acq_eval_sub(sls_gp* gp, int acq_type, double ucb_h, const sls_submaps* maps, const double* Z, int M, double* val,
                     double* grad_z, double* X_out);
/* sls_acq_maximize over z in [0,1]^d: starts_z is d x S, map_of_column has S entries.  z_out (d) / x_out (D) are the winner's variables
 * and point, z_stars (d x S) / x_stars (D x S) every start's; x is the expansion of z (one more expand launch: x_stars is bit for
 * bit the contract's expand of z_stars).  Any out pointer may be NULL.  val_out, idx_out, y_stars, start_index_offset and
 * sls_acq_last_stats as in sls_acq_maximize. */
int sls_acq_maximize_sub(sls_gp* gp, int acq_type, double ucb_h, const sls_submaps* maps, const double* starts_z, int S, int n_local,
                         const sls_lbfgs_opts* opts, long start_index_offset, double* z_out, double* x_out, double* val_out,
                         long* idx_out, double* z_stars, double* x_stars, double* y_stars);
/* The same pair for max-value entropy search: y_star, K as in sls_mes_eval / sls_mes_maximize. */
int sls_mes_eval_sub(sls_gp* gp, const double* y_star, int K, const sls_submaps* maps, const double* Z, int M, double* val,
                     double* grad_z, double* X_out);
int sls_mes_maximize_sub(sls_gp* gp, const double* y_star, int K, const sls_submaps* maps, const double* starts_z, int S, int n_local,
                         const sls_lbfgs_opts* opts, long start_index_offset, double* z_out, double* x_out, double* val_out,
                         long* idx_out, double* z_stars, double* x_stars, double* y_stars);
/* The same pair for the path draws.  sls_path_eval_sub: the gathered form only -- draw_of_point must not be NULL;
 * val[m] = f_{draw_of_point[m]}(c + A Z[:,m]).  sls_path_maximize_sub: starts_z is d x (n_draws S), columns [s S, (s+1) S) belong to
 * draw s and map_of_column is indexed by that column (n_draws S entries); per draw, as sls_path_maximize returns them, z_out
 * (d x n_draws), x_out (D x n_draws), val_out and idx_out (n_draws each; the start index within the draw). */
int sls_path_eval_sub(sls_path* p, const sls_submaps* maps, const double* Z, int M, const int* draw_of_point, double* val,
                      double* grad_z, double* X_out);
int sls_path_maximize_sub(sls_path* p, const sls_submaps* maps, const double* starts_z, int S, int n_local, const sls_lbfgs_opts* opts,
                          double* z_out, double* x_out, double* val_out, long* idx_out);

/* ---- multi-GPU maximisation ------------------------------------------------------------------------------
 * FindGlobalSolution's multi-start loop (src/acquisition-function.cpp:121-153) shards over its starts: the iterations share
 * only the const regressor (:125-141).  Every GPU holds a replica of the fitted state, runs a contiguous slice of the starts
 * with the global index offset, and contributes (value, global index, x[D]) to ONE ncclAllGather (RCCL over xGMI); the
 * first maximum (highest value, ties -> lowest global index: Eigen maxCoeff, :146-153) is taken on the gathered records.
 * RCCL is dlopen'ed on first use; single-GPU callers never load it. */

/* (1) one process, n devices, one host thread per device.  `devices` may name a GPU more than once (logical shards on one
 * device, used by tests on a 1-GPU box): RCCL allows one rank per GPU, so the records are then merged on the host;
 * sls_multi_exchange() says which exchange is in use ("ncclAllGather" or "host merge: <why>"). */
typedef struct sls_multi sls_multi;
typedef struct sls_multi_gp sls_multi_gp;
int sls_multi_create(const int* devices, int n, sls_multi** out);
int sls_multi_destroy(sls_multi* m);
int sls_multi_size(const sls_multi* m);
const char* sls_multi_exchange(const sls_multi* m);
sls_ctx* sls_multi_ctx(sls_multi* m, int shard);
/* sls_gp_create on every device (concurrently). */
int sls_multi_gp_create(sls_multi* m, const double* X, int D, int N, const double* y, const double* theta, double b, int kernel,
                        sls_multi_gp** out);
/* Replicas of an EXISTING fitted handle (what FindNextPoint* needs when several devices are configured): the shard on the
 * primary's own device is the primary itself -- no second fit there --, the other devices fit from its data.  `primary` must outlive
 * the result and must not be refitted or grown (sls_gp_append_point) while the replicas are in use. */
int sls_multi_gp_create_from(sls_multi* m, sls_gp* primary, sls_multi_gp** out);
int sls_multi_gp_destroy(sls_multi_gp* g);
sls_gp* sls_multi_gp_shard(sls_multi_gp* g, int shard);
/* sls_acq_maximize over all devices: starts (D x S, host) are split into contiguous slices; idx_out is the global start
 * index of the winner; evals_issued (may be NULL) sums the shards' sls_acq_last_stats. */
int sls_multi_acq_maximize(sls_multi_gp* g, int acq_type, double ucb_h, const double* starts, int S, int n_local,
                           const sls_lbfgs_opts* opts, double* x_out, double* val_out, long* idx_out, long* evals_issued);
/* sls_gp_predict over all devices: the M points (D x M, host) are split into contiguous column slices, shard r predicts its
 * slice on its device and writes mu / sigma at the slice's offset (gaussian-process-regressor.cpp:234-255 for M points; no
 * collective -- the outputs are disjoint).  A point's arithmetic does not depend on its slice: bit-identical to sls_gp_predict. */
int sls_multi_gp_predict(sls_multi_gp* g, const double* Xs, int M, double* mu, double* sigma);
/* GP MAP objective over the devices of `m`: the B independent points of one DIRECT iteration of PerformMapEstimation
   (src/gaussian-process-regressor.cpp:294) dealt round-robin, point k on shard k mod n, values gathered through host memory (no
   collective; the N^3 factorisation of ONE evaluation does not shard).  Bit-identical to sls_gp_nll_batch on one device. */
typedef struct sls_multi_nll sls_multi_nll;
int sls_multi_nll_create(sls_multi* m, const double* X, int D, int N, int kernel, sls_multi_nll** out);
int sls_multi_nll_destroy(sls_multi_nll* g);
int sls_multi_gp_nll_batch(sls_multi_nll* g, const double* y, const double* xs, int B, double* values);

/* (2) one process per GPU (torch.distributed.run / mpirun).  Rank 0 calls sls_comm_unique_id and distributes the 128 bytes
 * (any side channel); every rank then calls sls_comm_create on its context.  sls_comm_allgather_best is the single exchange
 * of a step: this rank's (value, global index, x[D]) in, the global first maximum out -- identical on every rank. */
typedef struct sls_comm sls_comm;
int sls_comm_unique_id(char* out128);
int sls_comm_create(sls_ctx* ctx, const char* id128, int rank, int world, sls_comm** out);
int sls_comm_destroy(sls_comm* c);
int sls_comm_allgather_best(sls_comm* c, double value, long index, const double* x, int D, double* value_out, long* index_out,
                            double* x_out);

/* ---- MAP objectives (hyper-parameter / goodness-value estimation) -------------------------------- */
/* Device state for repeated evaluations of the GP log-likelihood terms on a fixed design matrix X (D x N). */
typedef struct sls_nll sls_nll;
int sls_nll_create(sls_ctx* ctx, const double* X, int D, int N, int kernel, sls_nll** out);
int sls_nll_destroy(sls_nll* h);
/* NLopt's relative stopping tests for the MAP fits of this handle (sls_gp_map_fit, sls_pref_map_fit): applied to every accepted step
 * exactly as sls_lbfgs_opts.ftol_rel / xtol_rel are in the acquisition maximiser (on the optimiser's own variables: the logarithms of
 * the hyper-parameters).  0 = off, the default of a new handle; the reference's fits run through nloptutil::solve with 1e-6 / 1e-6
 * (SURVEY.md Appendix A), which the host layer sets.  A GP fit reaches its optimum to machine precision within 20-40 evaluations
 * and then backtracks for another 40-300 before it can no longer move; with the tests it ends there. */
int sls_nll_set_tolerances(sls_nll* h, double ftol_rel, double xtol_rel);
/* Core of both MAP objectives, for K_y = K_f(theta) + b I and a vector y (N):
 *   quad = y^T K_y^-1 y, logdet = log|K_y| (CalcLogDetOfSymmetricPositiveDefiniteMatrix), alpha = K_y^-1 y (may be NULL),
 *   grad_theta[p] = 1/2 alpha^T (dK/dtheta_p) alpha - 1/2 tr(K_y^-1 dK/dtheta_p), p = 0..D  (may be NULL)
 *   grad_b        = the same with dK/db = I                                              (may be NULL)
 * i.e. calc_grad_theta / calc_grad_b (src/gaussian-process-regressor.cpp:66-106) and CalcObjectiveThetaDerivative /
 * CalcObjectiveNoiseLevelDerivative (src/preference-regressor.cpp:53-115) without their prior terms, computed without
 * the (D+1) x N x N tensor of CalcLargeKYThetaDerivative (src/regressor.cpp:110-134).  A repeated (theta, b) re-uses
 * the cached factorisation (the reference's cached m_K / m_K_llt, src/preference-regressor.cpp:161-162,363-371). */
int sls_nll_eval(sls_nll* h, const double* y, const double* theta, double b, double* quad, double* logdet, double* alpha,
                 double* grad_theta, double* grad_b);
/* objective(x, grad) of src/gaussian-process-regressor.cpp:141-193 with x = (a, b, r_1..r_D) and the file's fixed
 * log-normal priors (:18-24).  grad (D + 2) may be NULL. */
int sls_gp_nll_grad(sls_nll* h, const double* y, const double* x, double* value, double* grad);
/* ---- leave-one-out cross-validation (Rasmussen & Williams, GPML 5.4.2) ---------------------------------------------------------
 * For K_y = K_f(theta) + b I, Kinv = K_y^-1, alpha = Kinv y and d_i = Kinv_ii, the prediction of y_i from the other N - 1 points:
 *   loo_mu[i]   = y_i - alpha_i / d_i            loo_var[i] = 1 / d_i  (the variance of y_i: noise included)
 *   loo_logp[i] = 1/2 log d_i - alpha_i^2 / (2 d_i) - 1/2 log 2 pi                     *value = L = sum_i loo_logp[i]
 * and the gradient of the LOO log pseudo-likelihood L as one weight matrix against dK/dtheta_p (no N^3 product per parameter):
 *   u = Kinv (alpha ./ d),  c_i = 1/2 (1 + alpha_i^2 / d_i) / d_i,  M = Kinv diag(c) Kinv,  W = 1/2 (u alpha^T + alpha u^T) - M
 *   grad_theta[p] = sum_ij W_ij dK_ij/dtheta_p, p = 0..D (theta as in sls_nll_eval),   *grad_b = sum_i (u_i alpha_i - M_ii).
 * N = 1 gives the prior: mean 0, variance a + b.  Every output may be NULL.  Always the tiled pipeline (also N <= 128), through the
 * same cached factorisation as sls_nll_eval (a repeated (theta, b) re-uses it; a call of either function leaves the other's results
 * unchanged).  A call without a gradient launches neither the symmetric product M nor the weight kernel.  M costs Np^2 doubles of
 * device memory per handle from the first gradient call on.  Errors as sls_nll_eval (SLS_ERR_NOT_SPD, SLS_ERR_INVALID).
 * Contract: equal inputs give equal bits; a call on a fresh factor and a call on the cached one give equal bits; the value of a
 * value-only call equals the value of a gradient call (L is summed in one fixed order: 256 partial sums over i mod 256, then a
 * binary tree). */
int sls_nll_loo(sls_nll* h, const double* y, const double* theta, double b, double* loo_mu, double* loo_var, double* loo_logp,
                double* value, double* grad_theta, double* grad_b);
/* sls_gp_nll_grad with the log marginal likelihood replaced by L: the same x = (a, b, r_1..r_D), the same log-normal prior terms,
 * the same sign (to be maximised).  grad (D + 2) may be NULL.  An invalid x (a <= 0, b < 0, r <= 0) is refused before any launch. */
int sls_gp_loo_grad(sls_nll* h, const double* y, const double* x, double* value, double* grad);
/* The three vectors (N each, any may be NULL) for a fitted handle's own hyper-parameters and data, in either sigma mode (explicit
 * inverse: diag(Kinv); Cholesky solve: d_i = sum_k (L^-1)_ki^2) and after sls_gp_append_point.  Takes the state lock shared, as the
 * predictions do. */
int sls_gp_loo(sls_gp* gp, double* loo_mu, double* loo_var, double* loo_logp);
/* values[k] = the same objective at xs[k] = (a, b, r_1..r_D), k < B, no gradients: the B independent evaluations of one DIRECT
   iteration of PerformMapEstimation (src/gaussian-process-regressor.cpp:294 evaluates them one by one).
     N <= 128: ONE launch, one workgroup per parameter set (bit-identical to B single evaluations).
     N >  128: bordered factorisations -- row N of K_y carries y, so y^T K_y^-1 y and log|K_y| come from the factor alone (no
               inverse) --, several parameter sets per persistent launch, each on its own share of the chip (a factorisation of this
               size is bound by its serial chain and leaves most CUs idle): 3.7x the rate of one full evaluation after the other
               at N = 4096, B = 8.  Values are bit-identical to the same call with one point at a time and agree with
               sls_gp_nll_grad's value to rounding.
   Every parameter set is validated up front (a > 0, b >= 0, r > 0: SLS_ERR_INVALID otherwise); a parameter set whose K_y is not
   positive definite yields -HUGE_VAL instead of an error. */
int sls_gp_nll_batch(sls_nll* h, const double* y, const double* xs, int B, double* values);
/* objective(x, grad) of src/preference-regressor.cpp:129-259.  x = (y_1..y_M [, a, b, r_1..r_D] if use_map_hyperparams);
 * prefs_flat / pref_offsets: CSR image of std::vector<Preference> (n_prefs tuples, first index = preferred point).
 * grad (same length as x) may be NULL.  For M <= 128 the whole objective -- BTL terms (include/sequential-line-search/utils.hpp:
 * 25-52, no max-subtraction: same overflow behaviour) included -- is one single-workgroup launch; larger problems run the
 * tiled pipeline with the O(#preferences) BTL terms on the host. */
typedef struct sls_pref_cfg {
    int use_map_hyperparams;
    double default_a, default_r, default_b, prior_var, btl_scale;
    int noiseless; /* SEQUENTIAL_LINE_SEARCH_USE_NOISELESS_FORMULATION (src/preference-regressor.cpp:48-50,139-143) */
} sls_pref_cfg;
int sls_pref_objective(sls_nll* h, const unsigned* prefs_flat, const int* pref_offsets, int n_prefs, const double* x,
                       const sls_pref_cfg* cfg, double* value, double* grad);
/* PreferenceRegressor::PerformMapEstimation (src/preference-regressor.cpp:332-403) as ONE device launch for M <= 128 data points
 * and D <= 128 dimensions, with or without use_map_hyperparams: the objective above -- Bradley-Terry-Luce terms included -- is maximised on the device by
 * the bounded L-BFGS that stands in for nloptutil::solve(..., LD_TNEWTON, ..., num_iters) (:377).  Variables z = (y_1..y_M
 * [, log a, log b, log r_1..log r_D]); z0 / lower / upper / z_out have that length; max_evals = NLopt's max_evals.
 * evals_per_launch: 0 = the whole fit in one launch; k > 0 = launches of k evaluations each, continued from device-resident
 * state (same machine code, same bits: the test hook behind "one launch == one launch per evaluation").
 * Returns SLS_ERR_UNSUPPORTED (nothing computed) outside those limits: drive sls_pref_objective from the host instead. */
int sls_pref_map_fit(sls_nll* h, const unsigned* prefs_flat, const int* pref_offsets, int n_prefs, const sls_pref_cfg* cfg,
                     const double* z0, const double* lower, const double* upper, int max_evals, int evals_per_launch,
                     double* z_out, double* value, int* evals_used);
/* Local phase of GaussianProcessRegressor::PerformMapEstimation (src/gaussian-process-regressor.cpp:295: TNEWTON from the DIRECT
 * point) in one launch for N <= 128, D <= 128: maximises sls_gp_nll_grad's objective over z = (log a, log b, log r_1..log r_D). */
int sls_gp_map_fit(sls_nll* h, const double* y, const double* z0, const double* lower, const double* upper, int max_evals,
                   int evals_per_launch, double* z_out, double* value, int* evals_used);

/* ---- instrumentation ------------------------------------------------------ */
/* Per-kernel accumulated device time (ms, HIP events on the context's stream) and launch counts since the last reset.
 * Names: "gram", "potri" (N <= 4096: factor + L^-1 + K^-1 in one launch) or "potrf", "trtri", "lauum" (larger N, or
 * SLS_POTRI_FUSED=0), "fit_small" (N <= 128: the whole fit in one launch), "cross_gram", "acq_gemm", "grad_gemm", "finalize",
 * "lbfgs"; the posterior calls: "post_v" (V = K* L^-T), "post_cov" (the covariance tiles), "post_potrf" (chol(cov + j I), one launch
 * per jitter tried), "post_sample" (normals + the sample product); the path draws: "path_setup" (normals, frequencies, weights,
 * f_prior(X)), "path_solve" (v = K_y^-1 r), "path_prior" (the random-feature prior of an evaluation), "path_data" (the data term
 * on cross_gram's K*; cross_gram and grad_gemm count under their own names); "mes" (the MES combiner, one launch per evaluation of
 * sls_mes_eval / round of sls_mes_maximize); "logei" (the LogEI combiner, one launch per evaluation / round of a type-2
 * call); "eubo" (the two kernels of the pair objective, pair_diff and eubo_finalize: two launches per pass of sls_eubo_eval /
 * per pass and round of sls_eubo_maximize; its GEMMs count under "cross_gram", "acq_gemm", "var_gemm", "grad_gemm");
 * "qeubo" (qeubo_select and qeubo_finish: two launches per pass of sls_qeubo_eval / per pass and round of sls_qeubo_maximize) and
 * "qeubo_agg" (its two aggregation GEMMs Wbar = W mask, Vbar = V mask), "qeubo_data_gemm" (the data term K* V of the every-draw values
 * on the tile GEMM, where sls_path_eval runs path_data's gathered dot; the reused stages count under "cross_gram", "path_prior",
 * "path_data", "path_grad_gemm");
 * "qnei" (the same two kernels with a per-draw baseline: two launches per pass of sls_qnei_eval / per pass and round of
 * sls_qnei_maximize; every other stage counts as under qEUBO) and "path_max" (the column reduction of sls_path_max_over_points, one
 * launch per pass; its values count under "cross_gram", "path_prior", "qeubo_data_gemm");
 * "qlognei" (the selection of the log form, two kernels under one entry, and the finish under another: two entries per pass of
 * sls_qlognei_eval / per pass and round of sls_qlognei_maximize; every other stage counts as under qEUBO);
 * "qbald" (the selection under the BTL likelihood, two kernels under one entry, and its finish under another: two entries per pass of
 * sls_qbald_eval / per pass and round of sls_qbald_maximize; every other stage counts as under qEUBO);
 * "line" (line_expand and line_fold: two launches per pass of sls_line_eval -- one without a gradient -- / per pass and round of
 * sls_line_maximize; the pass between them counts as under qEUBO / qNEI);
 * "patch" (patch_expand and patch_fold: two launches per pass of sls_patch_eval -- one without a gradient -- / per pass and round of
 * sls_patch_maximize; the pass between them counts as under qEUBO / qNEI);
 * "sub_expand" and "sub_fold" (the two kernels of the *_sub calls: one launch each per evaluation / per round of a maximiser, one more
 * "sub_expand" for x_out / x_stars; the evaluation between them counts as in the plain call);
 * "loo_terms" (the per-point terms and L: one launch per sls_nll_loo / sls_gp_loo_grad / sls_gp_loo call, two in the Cholesky-solve
 * sigma mode), "loo_syrk" (the scaled copy R and M = R R^T) and "loo_weight" (the LOO weights), one entry each per gradient call;
 * "laplace_w" (the BTL Hessian W of sls_gp_set_laplace), "laplace_b" (W L and B = I + L^T W L), "laplace_potri" (chol(B) and B^-1),
 * "laplace_m" (B^-1 L^T W, M and T), one entry each per sls_gp_set_laplace;
 * "potrf_fallbacks": launches = how often a single-launch factorisation gave up and was recomputed. */
int sls_prof_enable(sls_ctx* ctx, int on);
int sls_prof_reset(sls_ctx* ctx);
int sls_prof_get(sls_ctx* ctx, const char* name, double* total_ms, long* launches);

/* The library's run-time switches (SLS_* environment variables: A/B runs and test hooks, DESIGN.md "Run-time switches") are
 * parsed ONCE per process, at first use.  This re-reads the environment: for tests that switch paths inside one process. */
int sls_tuning_reload(void);

#ifdef __cplusplus
}
#endif
#endif
