// Launch wrappers of the hand-written gfx950 kernels (definitions in kernels_*.hip).
//
// Device-side data layout: every matrix keeps its LONG dimension contiguous.
//   training points   XtT [i + d*Np]      scaled + centred  x~ = (x - 0.5) / l_d, zero padded (Np = ceil128(N))
//   candidates        XsT [n + d*Sp]      same transform, n = candidate index         (Sp = ceil128(S))
//   K, L, Linv, Kinv  [i + j*Np]          column-major Np x Np, identity-padded
//   K*, C*, P         [n + i*Sp]          candidate-major: row i (training point) is contiguous over candidates
//   G_mu, G_sigma     [n + d*Sp]
// Padding to the 128-wide GEMM tile keeps every kernel free of edge code.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include "tuning.hpp"
#include "../../include/sls_hip.h"

#include <mutex>
#include <map>
#include <set>
#include <utility>

namespace slsk {

// hipFuncAttributeMaxDynamicSharedMemorySize is per (device, function): one process may drive several GPUs (sls_multi),
// so the opt-in is recorded per current device, under a lock (launch wrappers run on one host thread per device).
inline void ensure_dyn_lds(const void* fn, int bytes) {
    static std::mutex mtx;
    static std::map<std::pair<int, const void*>, int> done;   // (device, kernel) -> largest size set so far
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mtx);
    int& have = done[{dev, fn}];
    if (bytes > have) {
        // A runtime may refuse the opt-in and launch the kernel all the same (HIP 7.0 answers hipErrorInvalidValue to the 160 KB of
        // maximize_wave_kernel).  The refusal must not stay behind as the thread's last error: an application that shares the
        // runtime and checks hipGetLastError after its own launches (PyTorch does) would report it as its own failure.
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) (void)hipGetLastError();
        have = bytes;
    }
}

// Geometry of the CURRENT device, read once per device: compute units, and the XCDs (each with its own L2) they sit in.  HIP has no
// attribute for the latter; gfx950 builds an XCD from 32 active CUs and hands out workgroups round-robin over a partition's XCDs
// (SPX: 256 CUs = 8 XCDs; a CPX partition: 32 CUs = 1).  A CU count that is not a multiple of 32 is treated as one XCD.
struct ChipGeometry {
    int n_cu, n_xcd;
};
inline ChipGeometry chip_geometry() {
    static std::mutex mtx;
    static std::map<int, ChipGeometry> table;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mtx);
    auto it = table.find(dev);
    if (it != table.end()) return it->second;
    int v = 0;
    (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    ChipGeometry g;
    g.n_cu = v > 0 ? v : 64;
    g.n_xcd = (g.n_cu % 32 == 0) ? g.n_cu / 32 : 1;
    table[dev] = g;
    return g;
}

// k and the first-argument-derivative weight c (dk/dx_d = -c (x_d - x'_d) / l_d^2) of the scaled squared distance q
// (kernels_gram.hip, kernels_post.hip)
__device__ __forceinline__ void kernel_kc(int kernel, double a, double q, double& k, double& c) {
    if (kernel == SLS_KERNEL_ARD_SQUARED_EXPONENTIAL) {
        k = a * exp(-0.5 * q);
        c = k;
    } else {
        const double s = sqrt(5.0 * q);
        const double e = exp(-s);
        k = a * (1.0 + s + (5.0 / 3.0) * q) * e;
        c = a * (5.0 / 3.0) * (1.0 + s) * e;
    }
}

struct KernelSpec {
    int kernel;   // SLS_KERNEL_*
    double a;     // signal variance theta[0]
};

// ---- the guard of the norm expansion ---------------------------------------------
// The matrix-core Gram kernels take q_ij = |x~_i|^2 + |x~_j|^2 - 2 x~_i . x~_j, x~ = (x - 0.5) / l: a cancellation error of about
// eps (|x~_i|^2 + |x~_j|^2) <= eps D / (2 l_min^2), ABSOLUTE in q, for points of the unit box.  May an evaluation with largest
// inverse length scale `ilm` use it?  ONE criterion for the one-workgroup kernels (small_mc_form_ok, on the device) and the tiled
// routes (gram_direct_form, on the host): beyond `bound` the evaluation forms q from the differences of the RAW coordinates, which are
// exact for near-duplicate points.  A candidate outside the box needs no bound of its own: an entry matters only where k is not
// negligible (q < ~500), i.e. within 23 scaled units of a training point, and there |x~*|^2 <= 2 |x~_i|^2 + 1e3.
constexpr double GRAM_GUARD_BOUND = 1e-11;
__host__ __device__ __forceinline__ bool gram_expansion_ok(double ilm, int D, double bound = GRAM_GUARD_BOUND) {
    return ilm * ilm * (0.5 * D) * 2.3e-16 <= bound;
}
// Host side: ell = the D length scales of the evaluation.  SLS_GRAM_GUARD=0 switches the guard of the tiled routes off (A/B, tests).
inline bool gram_direct_form(const double* ell, int D, double bound = GRAM_GUARD_BOUND) {
    if (!tune_on(TUNE_GRAM_GUARD)) return false;
    double ilm = 0.0;
    for (int d = 0; d < D; ++d) ilm = 1.0 / ell[d] > ilm ? 1.0 / ell[d] : ilm;
    return !gram_expansion_ok(ilm, D, bound);
}
// sls_gram / sls_gram_cross hand out the ENTRIES: held to the direct form's own error 4 (D + 8) eps a.  |dk/dq| <= a / 2, so the
// expansion may serve them while its q is good to 8 (D + 8) eps.
inline double gram_entry_bound(int D) { return 8.0 * (D + 8) * 2.2e-16; }

// ---- kernels_gram.hip -------------------------------------------------------
// X (D x M column-major, device) -> XT[i + d*ld] = (X[d,i]-0.5)*inv_ell[d] for i<M,d<D, 0 elsewhere (i<Mp, d<Dcols); norms[i].
void launch_prep_points(hipStream_t s, const double* X, int D, int M, const double* inv_ell, double* XT, long ld, int Mp,
                        int Dcols, double* norms);
// same from candidate-major raw coordinates xr[n + d*ldr]
void launch_prep_cands(hipStream_t s, const double* xr, long ldr, int D, int M, const double* inv_ell, double* XT, long ld,
                       int Mp, int Dcols, double* norms);
// XaT[i + d*ld] = alpha[i] * XT[i + d*ld]
void launch_scale_rows(hipStream_t s, const double* XT, const double* alpha, double* XaT, long ld, int Np, int Dcols);
// K[i + j*Np] = k(x_i, x_j) (+ b on the diagonal); identity in the padding.  lower_only: skip tiles above the diagonal.
void launch_gram_sym(hipStream_t s, const double* XT, long ld, int Dp, const double* nx, int Np, int N, KernelSpec ks, double b,
                     double* K, bool lower_only);
// Ks[n + i*ldk] = k(xs_n, x_i), Cs likewise with the derivative weight c (Matern; Cs == Ks for SE);
// mu_part[t*ldk + n] = sum_{i in tile t} alpha_i k, ca_part likewise with c.  alpha may be NULL (no partials).
void launch_cross_gram(hipStream_t s, const double* XsT, long lds_, const double* ns, int Sp, const double* XT, long ld,
                       const double* nx, int Np, int N, int Dp, KernelSpec ks, const double* alpha, double* Ks, double* Cs,
                       long ldk, double* mu_part, double* ca_part);
// The same two results from the direct differences ((x_id - x_jd) / l_d)^2 of the RAW coordinates, on the VALU (O(N^2 D); for the
// evaluations gram_direct_form sends here).  X[d + i*D]: the N training points; inv_ell: D values.
void launch_gram_sym_direct(hipStream_t s, const double* X, int D, const double* inv_ell, int Np, int N, KernelSpec ks, double b,
                            double* K, bool lower_only);
// xr[n*sn + d*sd]: the M raw candidates (rows M .. Sp-1 are padding: 0.5 in every dimension, as launch_prep_* leave them)
void launch_cross_gram_direct(hipStream_t s, const double* xr, long sn, long sd, int M, int Sp, const double* X, int D,
                              const double* inv_ell, int Np, int N, KernelSpec ks, const double* alpha, double* Ks, double* Cs,
                              long ldk, double* mu_part, double* ca_part);

// gram_direct_form: the gradient contractions Gs / Gm of launch_grad_gemm (kernels_acq.hip) over the differences (x_i - x*_n) / l of the
// raw coordinates instead of x~_i alone; the finalize kernels are then given ca_part = cw_part = 0 (their x~* ca, x~* cw terms vanish).
// Gm == nullptr: Gs alone (Cs and alpha are not read).
void launch_grad_direct(hipStream_t s, const double* P, const double* Cs, long ldk, int Sp, const double* xr, long sn, long sd, int M,
                        const double* X, int D, const double* inv_ell, int N, const double* alpha, double* Gs, double* Gm);

// ---- kernels_small.hip ---------------------------------------------------------
// Whole MAP-objective evaluation for N <= 128, D <= 128 in one single-workgroup launch.  Inputs a, b, l_1..l_D, y_1..y_N travel
// in the kernel argument block (D <= 32) or in in_dev = [a, b, l.., y..] (device).  out (device, NLL_SMALL_OUT_DOUBLES):
// [0] sum W.*K_f, [1] d/db, [2] y^T alpha, [3] logdet, [4] potrf info, [8..8+D) d/dl (only if want_grad),
// [136..136+N) alpha.  X: raw D x N column-major design matrix (device); XTr: its transpose [i + d * 128] (device);
// kc (want_grad only): 2 x 128 x 128 doubles of scratch per launch (kernel values and derivative weights of the pairs, written by
// the Gram pass and read back by the gradient pass of the same workgroup).
constexpr int NLL_SMALL_MAX_N = 128;
constexpr int NLL_SMALL_MAX_D = 128;
constexpr int NLL_SMALL_MAX_ARG_D = 32;    // up to here the length scales travel in the kernel argument block (no upload)
constexpr int NLL_SMALL_OUT_GL = 8, NLL_SMALL_OUT_ALPHA = 8 + NLL_SMALL_MAX_D, NLL_SMALL_OUT_DOUBLES = NLL_SMALL_OUT_ALPHA + NLL_SMALL_MAX_N;
constexpr size_t NLL_SMALL_KC_DOUBLES = 2 * 128 * 128;
struct NllSmallArgs {
    const double* X;
    const double* XTr;
    double* kc;
    int x_lds = 1;            // 0: never stage the design matrix in LDS (A/B and tests: both paths agree to rounding)
    int D, N, want_grad;
    int* info;
    double* out;
    const double* in_dev;
    // batch > 1: workgroup w evaluates the parameter set in_dev + w * in_stride (in_dev must be set) into out + w * out_stride,
    // with its own pivot-failure word info[w]
    int batch;
    long in_stride, out_stride;
    double a, b;
    double ell[NLL_SMALL_MAX_ARG_D];
    double y[NLL_SMALL_MAX_N];
};
void launch_nll_small(hipStream_t s, int kernel, const NllSmallArgs& args);

// Whole fit of a GP handle for N <= 128 (Np = 128) in one single-workgroup launch (gp_fit_small_kernel): every output of
// gp_fit_device (capi.hip).  All pointers device; matrices 128 x 128 column-major, XT / XaT [i + d * 128] with Dcols columns.
struct GpFitSmallArgs {
    const double *X, *y, *inv_ell;   // X: raw D x N column-major (its transpose passes through XaT before alpha o X~ lands there)
    int D, N, Dcols;
    double a, b;
    double *XT, *nx, *XaT, *L, *Linv, *U, *Kinv, *alpha, *mu_data, *scal;   // scal[0] = max_i mu(x_i), scal[1] = log|K_y|
    long* d_idx;                     // first arg max of mu over the data points
    int* info;                       // 1 + index of the first non-positive pivot, or 0
    double* summary = nullptr;       // mapped host memory (or nullptr): [0] scal[0], [1] scal[1], [2] d_idx[0], [3] *info, [4] 0
    int x_lds = 1;                   // as NllSmallArgs::x_lds
};
void launch_gp_fit_small(hipStream_t s, int kernel, const GpFitSmallArgs& args);

// Whole MAP FIT for N <= 128 in one single-workgroup launch (map_opt_kernel): the bounded L-BFGS of host/device.cpp
// (optim::MaximizeBounded) with the objective evaluated in place -- the preference objective of
// src/preference-regressor.cpp:129-259 (Bradley-Terry-Luce terms from a CSR / CSC image of m_D, GP term, log-normal priors)
// or the GP marginal-likelihood objective of src/gaussian-process-regressor.cpp:141-193.
// Variables z (n = ny + nh <= 320: N <= 128 goodness values + D + 2 <= 130 hyper-parameters):  z[0..ny) = goodness values y
// (ny = N or 0: y fixed = y_fixed);  z[ny..ny+nh) = (a, b, l_1..l_D) (nh = D + 2 or 0: fixed a0, b0, r0), logarithms if log_hyper.
// The optimiser state lives in registers, 64 variables per register: 3 per lane up to 192 variables (C3: 91 + 34), 5 beyond.
constexpr int MAP_OPT_MAX_VARS = 320;
constexpr int MAP_OPT_HIST = 8;
constexpr int MAP_OPT_TRACE_SLOTS = 24;
constexpr int MAP_OPT_STATE_DOUBLES = (4 + 2 * MAP_OPT_HIST) * MAP_OPT_MAX_VARS + 32;
constexpr int MAP_OPT_OUT_X = 8, MAP_OPT_OUT_G = 8 + MAP_OPT_MAX_VARS, MAP_OPT_OUT_DOUBLES = 8 + 2 * MAP_OPT_MAX_VARS;
struct MapOptArgs {
    const double* X;          // D x N column-major design matrix (device)
    const double* XTr;        // its transpose [i + d * 128] (device)
    double* kc;               // NLL_SMALL_KC_DOUBLES of scratch (nh > 0)
    int x_lds = 1;            // as NllSmallArgs::x_lds
    int D, N, ny, nh, log_hyper, noiseless;
    const double* y_fixed;    // device, N (ny == 0)
    double a0, b0, r0;        // fixed hyper-parameters (nh == 0)
    double mu_a, mu_b, mu_r, s2_a, s2_b, s2_r;   // log-normal priors of a, b, l_d (nh > 0)
    double btl_scale;
    int n_prefs, flat_len;
    const int *pref_off, *pref_flat;   // CSR of the preference tuples: members of tuple p = pref_flat[pref_off[p] .. pref_off[p+1])
    const int *csc_off, *csc_ent;      // transposed: flat positions that name data point j, in increasing order
    double* btl_scratch;               // flat_len doubles (device); used when flat_len > 640 (else the LDS scratch)
    const double *z0, *lower, *upper;  // device, n each
    int max_evals;            // cap on objective evaluations of the whole fit
    double ftol_rel, xtol_rel;   // NLopt's relative stopping tests on accepted steps (sls_nll_set_tolerances), 0 = off
    int budget;               // evaluations performed by THIS launch (>= max_evals: the whole fit in one launch)
    int eval_only;            // 1: evaluate at z0, write value and gradient, stop
    int fresh;                // 1: start from z0; 0: continue from `state`
    double* state;            // MAP_OPT_STATE_DOUBLES (device): optimiser state, stored at the end of every launch
    double* out;              // MAP_OPT_OUT_DOUBLES: [0] objective at x, [1] evaluations used, [2] finished, [3] last pivot info,
                              // [8 .. 8+n) x, [8+320 .. 8+320+n) gradient (eval_only)
    int* info;
    // optional (SLS_MAP_TRACE=1, probes): MAP_OPT_TRACE_SLOTS ticks of the 100 MHz clock thread 0 spent in [0] publishing the trial
    // point, [8] Gram, [9] Cholesky, [10] log-det, [11] inverse, [1] alpha, [12] gradient weights, [13] length-scale contraction,
    // [3] BTL terms, [4] value + gradient slots, [5] optimiser, [6] evaluations, [7] kernel
    long long* trace;
};
void launch_map_opt(hipStream_t s, int kernel, const MapOptArgs& args);

// ---- kernels_acq.hip ---------------------------------------------------------
// P[n + i*ldk] = Cs * (Kinv Ks)  and the partial column sums kw_part (Ks.*W), cw_part (Cs.*W) per 128-row tile of i.
// kw_part / cw_part: [2 tn + half][candidate] (whole tiles use the even slot).  Returns the index (in the kernel's grouped tile
// order) of the first tile that ran as two half tiles (= the tile count if none): FinalizeArgs::split_first.
int launch_acq_gemm(hipStream_t s, const double* Ks, const double* Cs, long ldk, int Sp, const double* Kinv, int Np, double* P,
                    double* kw_part, double* cw_part, int* sync = nullptr);
// kw_part = per-tile partial sums of (Linv Ks)^2 (triangular contraction), cw_part = 0: the no-gradient form of acq_gemm
void launch_var_gemm(hipStream_t s, const double* Ks, long ldk, int Sp, const double* Linv, int Np, double* kw_part,
                     double* cw_part);
// Gs[n + d*ldk] = sum_i P[n,i] XT[i,d] ;  Gm[n + d*ldk] = sum_i Cs[n,i] XaT[i,d]   (d < Dcols)
// part (D <= 64 only, may be NULL): scratch of 8 * Sp * 64 doubles; used when grad_gemm_wants_split(Sp) to spread the
// contraction of a small launch over four times as many workgroups (same bits as the unsplit form).
// Always, since round 3: four times as many workgroups of a quarter of the work each fill the 768 slots evenly at every active-set
// size (C4: 85.9 -> 79.2 ms per step including grad_reduce4_kernel).  SLS_GRAD_SPLIT_TILES=t: split only launches of fewer than
// t tiles (0: never) -- the tests run both forms against each other.
inline bool grad_gemm_wants_split(int Sp) { return !tune_set(TUNE_GRAD_SPLIT_TILES) || 2 * (Sp / 128) < tune(TUNE_GRAD_SPLIT_TILES, 0); }
void launch_grad_gemm(hipStream_t s, const double* P, const double* Cs, long ldk, int Sp, const double* XT, const double* XaT,
                      long ld, int Np, int Dcols, double* Gs, double* Gm, double* part = nullptr, int passes = 2);
// passes = 1: the Gs product only (Cs, XaT, Gm are not read or written)
struct FinalizeArgs {
    int S, D, nbt;            // candidates in this chunk, dims, number of 128-row tiles of i
    int ntm, split_first;     // candidate tiles of the chunk; first half-split tile of launch_acq_gemm (INT_MAX: none)
    long ldk;                 // candidate leading dimension of this chunk
    const double *mu_part, *ca_part, *kw_part, *cw_part, *Gs, *Gm, *XsT, *inv_ell;
    const double* kw_solve_part = nullptr;   // solve-based sigma (see WaveArgs::solve_sigma): partial sums of (L^-1 k)^2 from var_gemm
    double a, mu_best, ucb_h;
    int acq;                  // SLS_ACQ_* (used when val/grad requested)
    // outputs (any may be NULL); all candidate-major with leading dimension ldo, offset already applied
    long ldo;
    double *mu, *sigma, *dmu, *dsigma, *val, *grad;
};
void launch_finalize(hipStream_t s, const FinalizeArgs& a);

// acquisition value / gradient from separately predicted mean and deviation (objective_for_multiple_points,
// src/acquisition-function.cpp:63-110): all arrays candidate-major with leading dimension ld
void launch_combine(hipStream_t s, int S, int D, long ld, const double* mu, const double* sigma, const double* dmu,
                    const double* dsigma, int acq, double mu_best, double ucb_h, double* val, double* grad);

// ---- kernels_mes.hip: max-value entropy search (sls_mes_*) ---------------------------------------------------------------
// With gamma_k = (y_star[k] - mu[n]) / sigma[n], g(t) = 1/2 t r - log Phi, g' = -1/2 r (1 + t (t + r)), r = phi / Phi:
//   val[n] = (1/K) sum_k g(gamma_k);  grad[n + d*ld] = -(1 / sigma[n]) (A1 dmu[n + d*ld] + A2 dsigma[n + d*ld]),
//   A1 = (1/K) sum_k g'(gamma_k), A2 = (1/K) sum_k gamma_k g'(gamma_k), every sum in increasing k.
// sigma < 1e-10 or a NaN in the value or the gradient: value 0, gradient 0.  Arrays candidate-major with leading dimension ld;
// grad may be NULL (dmu, dsigma are then not read); y_star: K doubles on the device.
void launch_mes_combine(hipStream_t s, int S, int D, long ld, const double* mu, const double* sigma, const double* dmu,
                        const double* dsigma, const double* y_star, int K, double* val, double* grad);
// g[i] = g(t[i]), dg[i] = g'(t[i]), i < n; either output may be NULL
void launch_mes_terms(hipStream_t s, const double* t, long n, double* g, double* dg);

// ---- kernels_logei.hip: log expected improvement (SLS_ACQ_LOG_EXPECTED_IMPROVEMENT) --------------------------------------
// With u = (mu[n] - mu_best) / sigma[n] and log h, B1 = Phi / h, B2 = phi / h of h = phi + u Phi (include/sls_hip.h):
//   val[n] = log sigma[n] + log h(u);  grad[n + d*ld] = (1 / sigma[n]) (B1 dmu[n + d*ld] + B2 dsigma[n + d*ld]).
// sigma < 1e-10 or a NaN in the value or the gradient: value SLS_LOG_EI_FLOOR, gradient 0.  Arrays candidate-major with leading
// dimension ld; grad may be NULL (dmu, dsigma are then not read).
void launch_logei_combine(hipStream_t s, int S, int D, long ld, const double* mu, const double* sigma, const double* dmu,
                          const double* dsigma, double mu_best, double* val, double* grad);
// log_h[i], b1[i], b2[i] of u[i], i < n; any output may be NULL
void launch_logei_terms(hipStream_t s, const double* u, long n, double* log_h, double* b1, double* b2);

// ---- kernels_jes.hip: joint entropy search on the optima of posterior draws (sls_jes_*) ----------------------------------
// tau[i] = 1 - r (t + r), dtau[i] = r ((t + r)(t + 2 r) - 1), r = phi / Phi, of t[i], i < n; either output may be NULL
void launch_jes_terms(hipStream_t s, const double* t, long n, double* tau, double* dtau);
// v[k] = sg_star[k]^2 + star_noise, dd[k] = f_star[k] - mu_star[k], inv_v[k] = 1 / v[k] (0 where v[k] < 1e-20), k < K
void launch_jes_optima(hipStream_t s, int K, const double* mu_star, const double* sg_star, const double* f_star, double star_noise,
                       double* v, double* dd, double* inv_v);
// kx[m + k*ld] = k(x_m, x*_k), cx[m + k*ld] = its derivative weight (cx may be NULL) from the raw coordinate differences, for m < M,
// k < K; 0 for m in [M, Mp), k in [K, Kp).  x[m*sn + d*sd] (device), xs[d + k*D] (device), Kp a multiple of 4.
void launch_jes_cross(hipStream_t s, const double* x, long sn, long sd, int M, int Mp, const double* xs, int D, int K, int Kp,
                      const double* inv_ell, KernelSpec ks, double* kx, double* cx, long ld);
// The combiner (include/sls_hip.h "joint entropy search"): one lane per candidate, every sum over k in increasing k.  cov / H are
// candidate-major [m + k*ld]; val[n], a_mu[n], a_sg[n] for n < S (unguarded: launch_jes_finish applies the guard); H[n + k*ld] for
// n < Sp, k < K (0 for n >= S).  a_mu, a_sg and H may be NULL together (value only).
void launch_jes_combine(hipStream_t s, int S, int Sp, long ld, const double* mu, const double* sigma, const double* cov,
                        const double* f_star, const double* dd, const double* inv_v, int K, double noise_var, double* val, double* a_mu,
                        double* a_sg, double* H);
// U[m + i*ld] <- Cs[m + i*ld] U[m + i*ld] and csum[m] = their sum over i < Np as four fixed quarters of i (((q0 + q1) + q2) + q3),
// each from zero in increasing i (path_data_kernel's order), m < Sp; Np a multiple of 128
void launch_jes_weight(hipStream_t s, int Sp, int Np, long ld, const double* Cs, double* U, double* csum);
// Go[m + d*ld] = (1 / l_d) sum_k H[m + k*ld] cx[m + k*ld] (x*_kd - x_md) in increasing k < K, m < M, d < D
void launch_jes_optima_grad(hipStream_t s, const double* x, long sn, long sd, int M, const double* xs, int D, int K,
                            const double* inv_ell, const double* H, const double* cx, long ld, double* Go);
// grad[n + d*ldo] = a_mu dmu + a_sg dsigma + (Gd[n + d*ldk] - XsT[n + d*ldk] csum[n] + Go[n + d*ldk]) / l_d (XsT == nullptr: no csum
// term) and the guard (sigma < 1e-10 or a NaN in val or the gradient: val 0, gradient 0), n < S.  grad == nullptr: the guard on val.
void launch_jes_finish(hipStream_t s, int S, int D, long ldo, long ldk, const double* sigma, const double* dmu, const double* dsigma,
                       const double* a_mu, const double* a_sg, const double* Gd, const double* Go, const double* XsT, const double* csum,
                       const double* inv_ell, double* val, double* grad);

// ---- kernels_kg.hip: knowledge gradient on a discrete set (sls_kg_*) ------------------------------------------------------------
// The combiner (include/sls_hip.h "knowledge gradient"): one workgroup per candidate, the lines sorted in LDS under a total order, the
// envelope by one lane, KG summed in envelope order and sum_k beta_k c_k in increasing k.  The inputs of launch_jes_combine plus the
// fixed means a[K], a_max and include_self; val[n], a_mu[n], a_sg[n] for n < S (unguarded: launch_jes_finish applies the guard);
// H[n + k*ld] for n < Sp, k < K (0 off the envelope and for n >= S).  a_mu, a_sg and H may be NULL together (value only, same bits).
// slope[n + k*ld_slope] = b_k(x_n) for n < S, k < K (may be NULL).
void launch_kg_combine(hipStream_t s, int S, int Sp, long ld, const double* mu, const double* sigma, const double* cov, const double* a,
                       double a_max, int K, double noise_var, int include_self, double* val, double* a_mu, double* a_sg, double* H,
                       double* slope, long ld_slope);
// The same kernel on caller-supplied lines (sls_kg_lines): slopes B[m + k*ld], own line (a_self[m], b_self[m]) when a_self != NULL;
// val[m] = E max - a_max + (own line: max(0, a_self - a_max)), beta / prob [m + k*ld], self_pi / self_beta [m]; each may be NULL.
void launch_kg_lines(hipStream_t s, int M, long ld, const double* a, double a_max, const double* B, int K, const double* a_self,
                     const double* b_self, double* val, double* beta, double* prob, double* self_pi, double* self_beta);

// ---- kernels_eubo.hip: expected utility of the best option of a query pair (sls_eubo_*) ----------------------------------
// Kd[n + i*ldk] = Ka[n + i*ldk] - Kb[n + i*ldk] over the whole padded block (ldk x Np doubles, both multiples of 128)
void launch_pair_diff(hipStream_t s, const double* Ka, const double* Kb, long ldk, int Np, double* Kd);
// The pair objective on the reduced sums (include/sls_hip.h).  Index 0 of every two-element member is the option x, index 1 is x'.
// mu_part / ca_part: cross_gram's partials of each option; kw_part: acq_gemm's k.w partials of d = k_x - k_x' (d^T K_y^-1 d);
// cw_part: acq_gemm's c.w partials of (Kd, C*_x) and (Kd, C*_x'); Gs / Gm: grad_gemm's products of each option.  Half-tile slots
// from split_first on as in FinalizeArgs.  kw_solve_part != nullptr: d^T K_y^-1 d = |L^-1 d|^2 from var_gemm's sums instead.
struct EuboFinalizeArgs {
    int S, D, nbt;            // pairs in this chunk, dims of ONE option, number of 128-row tiles of i
    int ntm, split_first;
    int kernel;               // SLS_KERNEL_*: k(x, x') and its derivative weight come from kernel_kc
    long ldk;
    const double *mu_part[2], *ca_part[2], *cw_part[2], *Gs[2], *Gm[2], *XsT[2];
    const double *kw_part, *inv_ell;
    const double* kw_solve_part = nullptr;
    // beyond the guard of the norm expansion (gram_direct_form): the two options' RAW coordinates, candidate-major xr[o][n + d*ldr];
    // k(x, x') and e_d then come from (x_d - x'_d) / l_d, differenced first (XsT's scaled coordinates leave eps / l).  nullptr: XsT.
    const double* xr[2] = {nullptr, nullptr};
    long ldr = 0;
    double a;
    // outputs, candidate-major with leading dimension ldo, offset already applied: val (may be NULL), grad (may be NULL): rows
    // 0..D-1 the gradient in x, rows D..2D-1 the gradient in x'
    long ldo;
    double *val, *grad;
};
void launch_eubo_finalize(hipStream_t s, const EuboFinalizeArgs& a);

struct LbfgsState {
    int S, D, m;
    long ld;                  // Sp
    double *x, *g, *dir, *xt, *scr;   // [n + d*ld]
    double *Sh, *Yh;          // [h][d][n]
    double *rho;              // [h][n]
    double *f, *t;            // [n]
    int *hlen, *hpos, *nbt, *done;    // [n]
    double c1, shrink, gtol;
    int max_backtracks;
    double ftol_rel = 0.0, xtol_rel = 0.0;   // NLopt's relative stopping tests on accepted steps (sls_lbfgs_opts), 0 = off
    // Active set: this round evaluated `nlive` trial points; column j of (val, grad) belongs to start live[j]
    // (live == nullptr: identity, nlive == S).  ldv = leading dimension of grad.
    const int* live;
    int nlive;
    long ldv;
};
// first: (val, grad) are the objective at the starts; otherwise at the trial points xt.  Writes the next trial points into
// xt (start-indexed) and marks starts that can no longer move (null step, exhausted backtracking, stationary) as done.
void launch_lbfgs_step(hipStream_t s, const LbfgsState& st, const double* val, const double* grad, bool first);
// Stable compaction of the starts that are still moving: live_out[0..count) = { n in live_in (or 0..n_in) : !done[n] } in
// increasing order, count -> *count_out (device); then xc[j + d*ldc] = xt[live_out[j] + d*ld] (padding columns up to the
// next multiple of 128 are filled with 0.5 so that the tile kernels read finite numbers).
void launch_compact_live(hipStream_t s, const int* live_in, int n_in, const int* done, int* live_out, int* count_out,
                         int* block_counts /* (n_in + 1023) / 1024 ints of scratch */);
void launch_gather_trials(hipStream_t s, const double* xt, long ld, int D, const int* live, const int* count_dev, int n_max,
                          double* xc, long ldc);
void launch_clamp_starts(hipStream_t s, const double* starts /*D x S col-major*/, int D, int S, double* xt, long ld, int Sp);
// first maximum of y[n] = -f[n]: out[0] = value, idx_out[0] = index
// best (mapped host memory): [0] max of -f, [1] its first index, [2] *counter (or 0), [8 .. 8 + D) = x[index + d ldx]
void launch_argmax_neg_gather(hipStream_t s, const double* f, int S, const double* x, long ldx, int D, double* best,
                              const unsigned long long* counter);

// NLopt's relative stopping tests (nlopt/src/util/stop.c: relstop) as the maximisers apply them to an accepted step; tolerance 0 = off.
//   lbfgs_f_stalled: |f' - f| < tol (|f'| + |f|) / 2 or f' == f
//   lbfgs_x_moved:   1 when coordinate d still moved by more than its tolerance (summed over d: 0 = every coordinate stalled)
__host__ __device__ inline bool lbfgs_f_stalled(double f_old, double f_new, double tol) {
    return tol > 0.0 && (fabs(f_new - f_old) < tol * 0.5 * (fabs(f_new) + fabs(f_old)) || f_new == f_old);
}
__host__ __device__ inline double lbfgs_x_moved(double x_old, double x_new, double tol) {
    return (fabs(x_new - x_old) < tol * 0.5 * (fabs(x_new) + fabs(x_old)) || x_new == x_old) ? 0.0 : 1.0;
}

// ---- kernels_wave.hip: one wavefront per start, whole L-BFGS in one launch (small problems) ----
struct WaveArgs {
    int S, D, N, Np, m, n_local, acq, matern;
    int lds_per_wave, Dr;                 // filled by the launcher
    int stage_kinv, stage_xt;             // filled by the launcher: K^-1 / XT copied into LDS behind the four waves' areas
    double a, mu_best, ucb_h, c1, shrink, gtol;
    int max_backtracks;
    double ftol_rel = 0.0, xtol_rel = 0.0;   // as in LbfgsState
    const double *XT, *inv_ell, *Kinv, *alpha, *starts;   // XT [i + d*Np] scaled; starts D x S column-major (raw)
    // solve_sigma (handles of a PreferenceRegressor, sls_gp_set_sigma_mode): sigma^2 = a - |L^-1 k|^2 and w = L^-T (L^-1 k) as the
    // reference's k . LLT.solve(k) (src/preference-regressor.cpp:299-313,323-330) instead of the explicit K^-1 of
    // GaussianProcessRegressor (src/gaussian-process-regressor.cpp:241-255).  Linv = L^-1 (zero above the diagonal), U = Linv^T.
    int solve_sigma = 0;
    int stage_ld = 0, stage_cols = 0;     // filled by the launcher: leading dimension / columns of the staged first-pass matrix
    int xch = 0;                          // filled by the launcher: doubles of the cooperative form's exchange area (0: one wave per start)
    const double *Linv = nullptr, *U = nullptr;
    double *x_out, *f_out;                // x_out[n + d*ld], f_out[n] = -acq at the end point
    unsigned long long* useful;           // optional: += evaluations of starts that were still moving (the others run idle)
    long ld;
    // evaluation-only mode (n_local == 0): `starts` holds the M query points; any of these may be NULL
    double *ev_mu, *ev_sigma, *ev_dmu, *ev_dsigma, *ev_val, *ev_grad;
    // optional (SLS_WAVE_TRACE=1, probes): ticks of the 100 MHz clock wave 0 of workgroup 0 spent in [0] the kernel-vector loop,
    // [1] w = K^-1 k, [2] the four reductions, [3] the gradient loop + acquisition, [4] L-BFGS direction, [5] step bookkeeping,
    // [6] evaluations, [7] whole kernel
    long long* trace = nullptr;
};
constexpr int WAVE_PATH_MAX_NP = 512;     // 8 rows per lane
constexpr int WAVE_PATH_MAX_D = 128;      // 2 dimensions per lane
void launch_maximize_wave(hipStream_t s, WaveArgs a);

// ---- kernels_chol.hip ---------------------------------------------------------
// In-place lower Cholesky of the Np x Np matrix A (ld = Np); Linv receives the 128x128 diagonal-block inverses
// (rest of Linv untouched).  info (device int) gets 1 + index of the first non-positive pivot, or stays 0.
// nbo: 128-columns per outer block of the multi-launch schedule (1 = one-level algorithm; default from potrf_default_nbo(Np)).
constexpr int NB = 128;            // block size of the factorisation = the GEMM tile
int potrf_default_nbo(int Np);
// one 128 x 128 diagonal block: Cholesky in place + its inverse into Tout (kernels_chol.hip; the multi-launch schedule's step)
void launch_chol_diag(hipStream_t s, double* A, long lda, double* Tout, long ldt, int* info, int global_off);
void launch_potrf(hipStream_t s, double* A, int Np, double* Linv, int* info, int nbo = 0, int* dataflow_sync = nullptr);
void launch_gemm_splitk_nt(hipStream_t s, const double* A, long lda, const double* B, long ldb, double* Cpart, long ldc,
                           long part_stride, int mt, int nt, int K, int chunks);
// Single-launch factorisation (SLS_POTRF_MODE=3, default): per-tile ownership and ready flags, no grid barriers.  sync =
// potrf_dataflow_sync_ints(Np) ints of device scratch; returns false when not applicable.  info[1] != 0 afterwards: a bounded
// wait expired (the kernel aborted; results undefined).  launch_potrf takes this path when dataflow_sync != nullptr, Np >= 384
// and SLS_POTRF_MODE is not 0 (0 = multi-launch schedule).
size_t potrf_dataflow_sync_ints(int Np);
bool launch_potrf_dataflow(hipStream_t s, double* A, int Np, double* Linv, int* info, int* sync, long long* trace = nullptr);
// nprob independent Np x Np factorisations in ONE launch, each on its own share of the chip's workgroups: problem q lives at
// A + q strideA / Linv + q strideA (doubles), uses sync + q stride_sync (ints) and reports into info[2 q], info[2 q + 1].
// block_inverses = false: the 128 x 128 inverses T_jj are not formed (callers that only need L).  Same bits per problem as a
// launch of its own (a tile's arithmetic does not depend on how many workgroups take part).
int potrf_dataflow_max_problems(int Np);
bool launch_potrf_dataflow_batch(hipStream_t s, double* A, int Np, double* Linv, int* info, int* sync, int nprob, long strideA,
                                 long stride_sync, bool block_inverses, long long* trace = nullptr);
// The same launch with a second team of workgroups that builds Linv = L^-1, U = Linv^T and Kinv = A^-1 behind the factorisation
// (N <= 4096; kernels_chol.hip: potri_team).  launch_potri picks it when it applies and falls back to launch_potrf + launch_trtri
// + launch_lauum otherwise (SLS_POTRI_FUSED=0: always); returns true when the fused launch ran.
struct PotriFused {
    double* U;
    double* Kinv;
};
bool launch_potri_dataflow(hipStream_t s, double* A, int Np, double* Linv, double* U, double* Kinv, int* info, int* sync,
                           long long* trace = nullptr);
bool potri_fused_applies(int Np, bool have_sync);   // sizes / switches only: the launch itself may still decline (too few CUs)
bool launch_potri(hipStream_t s, double* A, int Np, double* Linv, double* U, double* Kinv, int* info, int* dataflow_sync,
                  bool linv_zeroed = true);   // false: Linv was not cleared by the caller (only the separate launches need it: done inside)
int potrf_default_mode(int Np);
// Linv <- L^-1 (lower) given L and the diagonal-block inverses already in Linv; tmp is an Np x Np scratch.
void launch_trtri(hipStream_t s, const double* L, int Np, double* Linv, double* tmp, double* U);   // U <- (L^-1)^T
void launch_transpose_full(hipStream_t s, const double* src, double* dst, int Np);   // dst = src^T (Np x Np)
// diagonal-block inverses only (for potrs / potri on a caller-supplied factor)
void launch_diag_inverse(hipStream_t s, const double* L, int Np, double* Linv);
// Kinv <- Linv^T Linv (full symmetric)
void launch_lauum(hipStream_t s, const double* U, int Np, double* Kinv);                           // K^-1 = U U^T
// B (Np x Rp, ld = Np, Rp multiple of 128) <- (L L^T)^-1 B using the block inverses in Linv's diagonal
void launch_potrs(hipStream_t s, const double* L, const double* Linv, int Np, double* B, int Rp);
// y = A x; `part` is a caller-owned scratch of (Np/128) * Np doubles (per-chunk partial sums, reduced in fixed order)
void launch_gemv_n(hipStream_t s, const double* A, int Np, const double* x, double* y, double* part, bool lower = false);   // lower: A is lower triangular (zeros above the diagonal are not read)
void launch_gemv_t(hipStream_t s, const double* A, int Np, const double* x, double* y, bool lower = false);   // y = A^T x
void launch_zero_upper(hipStream_t s, double* A, int Np);
void launch_fill(hipStream_t s, double* p, long n, double v);
// mu_data[i] = y[i] - b*alpha[i] (i<N); out: first argmax + value; logdet = 2 sum log L_ii (i<N)
// mu_data = y - b alpha, scal[0] = its first maximum, d_idx[0] = where, scal[1] = 2 sum log L_ii; summary (mapped host memory or
// nullptr): [0] max, [1] log-det, [2] index, [3..4] info[0..1]
void launch_fit_summary(hipStream_t s, const double* y, const double* alpha, double b, int N, double* mu_data, const double* L, int Np,
                        const int* info, double* scal, long* d_idx, double* summary);
// bordered factorisation (value-only MAP objective): row N of each of the nprob matrices A + q strideA <- (y^T, c); after the
// factorisation out[2 q] = y^T K^-1 y (= |row N of L|^2) and out[2 q + 1] = log|K|
void launch_border_row(hipStream_t s, double* A, long strideA, int nprob, int Np, int N, const double* y, double c);
void launch_border_reduce(hipStream_t s, const double* L, long strideA, int nprob, int Np, int N, double* out);

// ---- rank-1 growth of the fitted state by one data point (kernels_chol.hip) ----
// scal_out[0] = k.u, scal_out[1] = l.l, scal_out[2] = u.y  (fixed-order block reductions)
void launch_append_dots(hipStream_t s, const double* k, const double* u, const double* l, const double* y, int N, double* scal_out);
// Kinv(0:N,0:N) += u u^T / s ; Kinv(N,0:N) = Kinv(0:N,N) = -u / s ; Kinv(N,N) = 1/s ;
// L(N,0:N) = l ; L(N,N) = lam ; Linv(N,0:N) = -u / lam ; Linv(N,N) = 1/lam ; alpha(0:N) += u (uy - eta)/s ; alpha(N) = (eta - uy)/s
void launch_append_update(hipStream_t s, double* Kinv, double* L, double* Linv, double* alpha, int Np, int N, const double* u,
                          const double* l, const double* scal /* k.u, l.l, u.y on device */, double kappa, double eta);

// generic C = alpha * opA opB^T + beta * C on full 128-tiles (mt x nt tiles, K multiple of 16)
void launch_gemm_plain(hipStream_t s, const double* A, long lda, bool a_kc, const double* B, long ldb, bool b_kc, double* C,
                       long ldc, int mt, int nt, int K, double alpha, double beta);

// C = A L^T, L lower triangular (k < 128 (tn + 1) per output tile column); C = alpha L B^T + beta C (k < 128 (tm + 1) per tile row).
// All operands M-contiguous, full 128-tiles (kernels_tri.hip).
void launch_gemm_rhs_lower(hipStream_t s, const double* A, long lda, const double* L, long ldl, double* C, long ldc, int mt, int nt);
void launch_gemm_lhs_lower(hipStream_t s, const double* L, long ldl, const double* B, long ldb, double* C, long ldc, int mt, int nt,
                           double alpha, double beta);

// ---- kernels_post.hip: joint posterior at M query points ---------------------------------------------------------
// C[i + j*Mp] = k(xs_i, xs_j) - sum_{k < Kv} V[i + k*ldv] V[j + k*ldv] for i, j < M, identity in the padding (i or j >= M), for
// the full Mp x Mp matrix: one workgroup per LOWER 128 x 128 tile, the tile and its mirror written from the same registers, so C
// is exactly symmetric.  XsT [n + d*ldx] / ns: the query points' scaled coordinates and norms (launch_prep_points); Dp, Kv
// multiples of 16.
// V2 != nullptr (same layout as V): the second factor of the product, C = k - V V2^T -- a Laplace handle passes V2 = V T, T symmetric;
// only the lower half of every tile is computed and the mirror is written from the same registers, so C stays exactly symmetric.
void launch_post_cov(hipStream_t s, const double* XsT, long ldx, int Dp, const double* ns, const double* V, long ldv, int Kv, int Mp,
                     int M, KernelSpec ks, double* C, const double* V2 = nullptr);
// the same with the prior term k(Xs, Xs) from the raw query points Xs[d + i*D] (gram_direct_form)
void launch_post_cov_direct(hipStream_t s, const double* Xs, int D, const double* inv_ell, const double* V, long ldv, int Kv, int Mp,
                            int M, KernelSpec ks, double* C, const double* V2 = nullptr);
// Standard normal number t of stream `seed`: Philox4x64-10 with key (seed, 0) on block counter (t / 4, 0, 0, 0); each 64-bit
// output x becomes u = ((x >> 11) + 0.5) 2^-53; Box-Muller on the output pairs (0, 1) and (2, 3) gives r01 cos, r01 sin, r23 cos,
// r23 sin for t mod 4 = 0 .. 3.
// Zt[sl + j*ldz] = normal number (s0 + sl) M + j for sl < sc, j < M; 0 for sl in [sc, Scp) or j in [M, Mp) (sample-major).
void launch_normal_fill(hipStream_t s, unsigned long long seed, long s0, int sc, int Scp, int M, int Mp, double* Zt, long ldz);
// out[i] = normal number offset + i of stream `seed`, i < n
void launch_random_normal(hipStream_t s, unsigned long long seed, long offset, long n, double* out);
// A[i + i*Mp] += v for i < M
void launch_add_diag(hipStream_t s, double* A, int Mp, int M, double v);
// flag[0] (device int) = 1 + the first i < M whose pivot L_ii^2 is <= thr (or not a number), 0 if none
void launch_pivot_check(hipStream_t s, const double* L, int Mp, int M, double thr, int* flag);
// zero the strictly upper triangle of every 128 x 128 diagonal block of A (Mp x Mp)
void launch_zero_diag_upper(hipStream_t s, double* A, int Mp);
// C[m + n*ldc] = mu[m] for m < Mp, n < ncols
void launch_bcast_cols(hipStream_t s, const double* mu, int Mp, double* C, long ldc, int ncols);

// ---- kernels_path.hip: pathwise posterior function draws (sls_path_*) ----------------------------------------------------
// Om[l + d*Fp] = frequency l (l < F, d < D; 0 in the padding up to Fp x Dc) from the B0 normals Z of the draw-independent block
void launch_path_omega(hipStream_t s, const double* Z, int F, int Fp, int D, int Dc, int matern, double* Om);
// W (2Fp x Rp, ld 2Fp): cos weights in rows [0, F), sin weights in rows [Fp, Fp + F), times `scale`, from the draw block E; 0 elsewhere
// (N enters through the draw stride 2F + N alone: a Laplace handle, whose draws take 2F + 2N numbers, passes 2N)
void launch_path_weights(hipStream_t s, const double* E, int F, int Fp, int N, int n_draws, int Rp, double scale, double* W);
// R[i + s*Np] <- y_i - sqrt_b eps_{s,i} - R[i + s*Np] (i < N, s < n_draws), 0 in the padding (Np x Rp)
// Q != nullptr (a Laplace handle; Np x Rp): draws take 2F + 2N numbers (w, w', eps, z) and
// R[i + s*Np] <- (y_i + Q[i + s*Np]) - sqrt_b eps_{s,i} - R[i + s*Np], Q = L L_B^-T z the sampled deviation of the goodness values
void launch_path_rhs(hipStream_t s, const double* y, const double* E, int F, int N, int Np, int n_draws, int Rp, double sqrt_b,
                     double* R, const double* Q = nullptr);
// Z[i + s*Np] = E[s (2F + 2N) + 2F + N + i] for i < N, s < n_draws; 0 elsewhere (Np x Rp): the z block of a Laplace handle's draws
void launch_path_laplace_z(hipStream_t s, const double* E, int F, int N, int Np, int n_draws, int Rp, double* Z);
// Random-feature contraction of Mp points (XsT [m + d*ldx], Dp columns) with the frequencies (Om [l + d*Fp], Fp a multiple of 128) on
// the matrix cores, sincos epilogue.  draw != nullptr (gathered form, rows m < nvalid under draw[m]): G[m + l*ldg] = W_s cos - W_c
// sin and the value partials vpart[chunk*ldv + m] of the 128-frequency chunks; draw == nullptr: G[m + l*ldg] = cos, G[m + (Fp+l)*ldg]
// = sin (the features Phi, Mp x 2Fp).
void launch_path_feat(hipStream_t s, const double* XsT, long ldx, int Dp, int Mp, const double* Om, int Fp, const double* W, long ldw,
                      const int* draw, int nvalid, double* G, long ldg, double* vpart, long ldv);
// val[n] = sum over the chunks (in order) of vpart[c*ldv + n]
void launch_path_vsum(hipStream_t s, const double* vpart, long ldv, int nchunk, int S, double* val);
// Data term of P (point, draw) pairs on K* / C* ([pt + i*ldk], cross_gram): val[o] += K*[pt, :] . V[:, dr].  Gathered form (draw !=
// nullptr): point p under draw[p], o = p; every-draw form: point p % npts under draw p / npts, o = pt + dr*ldo.  Pm != nullptr
// (gathered form only): Pm[pt + i*ldk] = C*[pt, i] V[i, dr] (0 for N <= i < Np) and csum[pt] = sum_i Pm[pt, i]
void launch_path_data(hipStream_t s, const double* Ks, const double* Cs, long ldk, int N, int Np, const double* V, long ldv, const int* draw,
                      int npts, long ldo, int P, double* val, double* Pm, double* csum);
// grad[n + d*ldo] = inv_ell_d (Gt[n + d*ldk] - XsT[n + d*ldk] csum[n])
void launch_path_grad(hipStream_t s, int S, int D, long ldk, const double* Gt, const double* XsT, const double* csum, const double* inv_ell,
                      double* grad, long ldo);
// grad[n + d*ldo] = inv_ell_d (Gt[n + d*ldk] + Gd[n + d*ldk]): Gt = G Om alone, Gd = launch_grad_direct's Gs with P = Pm (gram_direct_form)
void launch_path_grad_direct(hipStream_t s, int S, int D, long ldk, const double* Gt, const double* Gd, const double* inv_ell, double* grad,
                             long ldo);
// draw[j] = (live ? live[j] : j) / S, j < n
void launch_path_draw_of_live(hipStream_t s, const int* live, int n, int S, int* draw);
// per draw s (starts [s S, (s+1) S)): first maximum of -f; out[s (D + 2) + 0] = value, [+1] = index within the draw, [+2 ..] = x
void launch_path_argmax(hipStream_t s, const double* f, int S, int n_draws, const double* x, long ldx, int D, double* out);

// ---- kernels_qeubo.hip: expected utility of the best of q options on posterior draws (sls_qeubo_*) ------------------------
// Points of a pass are option-major: option i of set n is point i*Sp + n (Sp = the pass's sets rounded up to 128).
// V[i*Sp + n + s*ldv] = f_s(x_i) on entry (Rp rows s, the every-draw values).  One lane per set: sum[n] = sum over s < S (increasing) of
// max_i, the lowest i winning ties; wins[n + i*ldw] = draws option i wins (wins may be NULL); bad[n] = 1 if any value is not a number.
// V is overwritten in place by the 0/1 winner indicator, cleared for s >= S and for the padding sets n in [nsets, Sp).
// t != nullptr (qNEI: S device doubles, the per-draw baseline): the options compete against t[s] -- best = t[s] with no winner, every
// option strictly-greater in increasing i --, sum[n] adds best - t[s], and a draw without a winner leaves its mask column zero.
void launch_qeubo_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, const double* t, double* sum,
                         int* wins, long ldw, int* bad);
// val[n] = sum[n] / S, grad[n + (i*D + d)*ldo] = gpt[i*Sp + n + d*ldg] / S for n < nsets; bad[n] or a NaN among them: value
// `floor` (SLS_QEUBO_FLOOR; 0 for qNEI) and the zero gradient.  val / grad may be NULL.
// precomputed (qLogNEI): val[n] = sum[n] and the gradient as it stands, nothing divided.
void launch_qeubo_finish(hipStream_t s, int nsets, int Sp, int q, int D, int S, const double* sum, const int* bad, const double* gpt,
                         long ldg, double floor, double* val, double* grad, long ldo, bool precomputed = false);
// Per draw s < n_draws (one workgroup each): the maximum over pt < rows of V[pt + s*ldv] and the lowest pt that attains it, merged into
// the running record: base = 0 writes (t[s], arg[s]); base > 0 (a later pass, indices base + pt) replaces it only when strictly
// greater.  A NaN in the column gives (NaN, -1), which later passes leave.
void launch_path_colmax(hipStream_t s, const double* V, long ldv, int rows, int n_draws, int base, double* t, int* arg);

// ---- kernels_qlognei.hip: log-space noisy expected improvement on posterior draws (sls_qlognei_*) -------------------------
// L[i] = log softplus(a[i]), R[i] = L'(a[i]), i < n (the branches of include/sls_hip.h); either output may be NULL
void launch_qlognei_terms(hipStream_t s, const double* a, long n, double* L, double* R);
// The slices the S draws are cut into (a fixed slice length, whatever S and the pass are)
int qlognei_slices(int S);
// The selection of the qEUBO pass in log space, two launches.  V[i*Sp + n + s*ldv] = f_s(x_i) on entry, c_{i,s} = d value / d v_{i,s}
// on exit (rows S <= s < Rp, the lanes n >= nsets and sets with a NaN: exactly 0); t = S device doubles.  sum[n] = the value (nothing
// is left to divide), wins[n + i*ldw] = the hard wins of launch_qeubo_select with the same t, bad[n] = a NaN among the q S values.
// Scratch: mq, zq (Sp x Rp doubles), pmx, psm (Sp x qlognei_slices(S) doubles), pbad (as many ints), pwin (q times as many ints).
void launch_qlognei_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, const double* t, double tau0,
                           double taum, double* mq, double* zq, double* pmx, double* psm, int* pbad, int* pwin, double* sum, int* wins,
                           long ldw, int* bad);

// ---- kernels_qbald.hip: information gain of a choice query on posterior draws (sls_qbald_*) -------------------------------
// The slices the S draws are cut into (a fixed slice length, whatever S and the pass are)
int qbald_slices(int S);
// The selection of the qEUBO pass under the BTL likelihood of scale tau, two launches.  V[i*Sp + n + s*ldv] = f_s(x_i) on entry,
// c_{i,s} = d value / d v_{i,s} on exit (rows S <= s < Rp, the lanes n >= nsets and sets with a NaN: exactly 0).
// pkl[n + k*Sp] = the sum of KL_s over slice k (launch_qbald_finish adds the slices), pbar[n + i*Sp] = the predicted choice
// probability of option i, wins[n + i*ldw] = the hard wins of launch_qeubo_select without a baseline (wins may be NULL), bad[n] = a
// NaN among the q S values.
// Scratch: pp (Sp x q qbald_slices(S) doubles), pbad (Sp x qbald_slices(S) ints), pwin (q times as many ints).
void launch_qbald_select(hipStream_t s, int nsets, int Sp, int q, int S, int Rp, double* V, long ldv, double tau, double* pp, double* pkl,
                         int* pbad, int* pwin, double* pbar, int* wins, long ldw, int* bad);
// val[n] = (sum over the slices k, increasing, of pkl[n + k*Sp]) / S, grad[n + (i*D + d)*ldo] = gpt[i*Sp + n + d*ldg] as it stands,
// prob[n + i*ldp] = pbar[n + i*Sp] for n < nsets; bad[n] or a NaN among value and gradient: `floor`, the zero gradient and a zero
// prob column.  val / grad / prob may be NULL.
void launch_qbald_finish(hipStream_t s, int nsets, int Sp, int q, int D, int S, const double* pkl, const int* bad, const double* gpt,
                         long ldg, const double* pbar, double floor, double* val, double* grad, long ldo, double* prob, long ldp);

// ---- kernels_line.hip: expected utility of the best slider position (sls_line_*) ------------------------------------------
// A line is its ends (a, b); position i of q is x_i = u_i a + t_i b with u_i = (q-1-i)/(q-1), t_i = i/(q-1) computed on the device (one
// division each; two products and one sum per coordinate, never fused).  trial[n + r*ld] is the candidate-major line block: rows
// 0..D-1 = a and D..2D-1 = b (anchor == nullptr), or D rows = b with a = anchor[d] (device, D doubles).
// sets[n + (i*D + d)*lds] = x_i[d] for n < nlines: the block qeubo_eval_device reads.
void launch_line_expand(hipStream_t s, int nlines, int D, int q, const double* trial, long ld, const double* anchor, double* sets,
                        long lds);
// grad_a = sum_i u_i g_i (from zero, increasing i), grad_b = sum_i t_i g_i (from zero, DECREASING i: the mirror image of grad_a's order)
// of the set gradient sgrad[n + (i*D + d)*lds], product and sum never fused.  grad[n + d*ldo] = grad_a and grad[n + (D + d)*ldo] =
// grad_b; anchored: grad[n + d*ldo] = grad_b alone.
void launch_line_fold(hipStream_t s, int nlines, int D, int q, bool anchored, const double* sgrad, long lds, double* grad, long ldo);

// ---- kernels_patch.hip: expected utility of the best gallery cell (sls_patch_*) -------------------------------------------
// A patch is its corners (c00, c10, c01, c11); cell (i, j) of the qs x qt grid is option k = i + qs j of the expanded set:
// x_k = v_j (u_i c00 + s_i c10) + t_j (u_i c01 + s_i c11), the weights of launch_line_expand along each axis, three sums of two
// products, never fused.  trial[n + r*ld] is the candidate-major patch block: rows 0, D, 2D, 3D start c00, c10, c01, c11 (anchor ==
// nullptr), or rows 0, D, 2D start c10, c01, c11 with c00 = anchor[d] (device, D doubles).
// sets[n + (k*D + d)*lds] = x_k[d] for n < npatches: the block qeubo_eval_device reads.  qs, qt >= 2, qs qt <= 16.
void launch_patch_expand(hipStream_t s, int npatches, int D, int qs, int qt, const double* trial, long ld, const double* anchor,
                         double* sets, long lds);
// The fold of launch_line_fold along i within every grid row (A_j with u in increasing i, B_j with s in decreasing i), then along j
// over the row sums (v in increasing j for c00 / c10, t in decreasing j for c01 / c11), of the set gradient sgrad[n + (k*D + d)*lds].
// grad[n + r*ldo] in the rows of the patch block (3D rows, without c00, when anchored).
void launch_patch_fold(hipStream_t s, int npatches, int D, int qs, int qt, bool anchored, const double* sgrad, long lds, double* grad,
                       long ldo);

// ---- kernels_sub.hip: search over affine subspaces (the *_sub entry points) ------------------------------------------------
// The maps of one call as the kernels read them (device pointers into ONE block, uploaded once per call): n_maps blocks A_k of D x d,
// column-major A_k[r + j*D], n_maps blocks c_k of D, and the map of every column of the call (nullptr: every column uses map 0).
struct SubMaps {
    int D, d, n_maps;
    const double* A;
    const double* c;
    const int* map_of_column;
};
// X[n + r*ldx] = c_r + sum_j A_rj z[n + j*ld] for n < ncols, r < D, with the map of column (live ? live[n] : n): from c_r, one product
// and one sum per j in increasing j, never fused.  No clamp.  A column's bits depend on its own z and its own map alone.
// The columns ncols <= n < min(round_up(ncols, 128), ldx) are set to 0.5 (the padding of the last tile the evaluation reads).
void launch_sub_expand(hipStream_t s, const SubMaps& m, int ncols, const int* live, const double* z, long ld, double* X, long ldx);
// gz[n + j*ldo] = sum_r A_rj gx[n + r*ldx] for n < ncols, j < d: from zero, one product and one sum per r in increasing r, never fused.
void launch_sub_fold(hipStream_t s, const SubMaps& m, int ncols, const int* live, const double* gx, long ldx, double* gz, long ldo);

// ---- kernels_map.hip -----------------------------------------------------------
// MAP-gradient weights (replaces the (D+1) x N x N tensor of CalcLargeKYThetaDerivative, src/regressor.cpp:110-134):
// G[j + k*Np] = 1/2 (alpha_j alpha_k - Kinv_jk) c_jk  (0 in the padding);  wk_part[tile] = sum over the tile of
// 1/2 (alpha_j alpha_k - Kinv_jk) kf_jk  (kf = kernel value without noise).  ntiles = (Np/128)^2 partials.
void launch_nll_weight(hipStream_t s, const double* XT, long ld, int Dp, const double* nx, int Np, int N, KernelSpec ks,
                       const double* alpha, const double* Kinv, double* G, double* wk_part, double* row_part);
// row_part (nullptr: skip): [Np / 128][Np] partial row sums of G, one slice per tile column; launch_sum_chunks adds them in slice order
// out[0] = sum_t part[t] (fixed order);  out[1] = 1/2 (alpha.alpha - tr Kinv);  out[2] = y.alpha
void launch_nll_scalars(hipStream_t s, const double* part, int nparts, const double* alpha, const double* y,
                        const double* Kinv, int Np, int N, double* out, const double* Lfac = nullptr,
                        const int* info = nullptr);   // Lfac: out[4] = 2 sum log L_ii too;  info: out[5..6] = info[0..1]
// gl[p] = 2 * inv_ell[p] * sum_j XT[j,p] * (XT[j,p] * s_j - Y[j,p]),  p < D;  one more workgroup of the same launch does what
// launch_nll_scalars does (arguments from `part` on)
void launch_lengthscale_grad(hipStream_t s, const double* XT, const double* Y, const double* svec, const double* inv_ell,
                             long ld, int N, int D, double* gl, const double* part, int nparts, const double* alpha, const double* y,
                             const double* Kinv, int Np, double* out, const double* Lfac, const int* info);
// gram_direct_form: G and the per-tile sums wk_part from the raw coordinate differences (X[d + i*D]), and the length-scale gradient
// as the unexpanded contraction sum_ij G_ij (x~_ip - x~_jp)^2 / l_p (no Y, no row sums); the last block leaves the evaluation's sums.
void launch_nll_weight_direct(hipStream_t s, const double* X, int D, const double* inv_ell, int Np, int N, KernelSpec ks,
                              const double* alpha, const double* Kinv, double* G, double* wk_part);
void launch_lengthscale_grad_direct(hipStream_t s, const double* X, const double* G, const double* inv_ell, int Np, int N, int D,
                                    double* gl, const double* part, int nparts, const double* alpha, const double* y, const double* Kinv,
                                    double* out, const double* Lfac, const int* info);
// Y = sum of `chunks` partial products `stride` apart (in place in the first), and svec = sum of `row_chunks` slices of row_part
void launch_sum_chunks(hipStream_t s, double* Y, long n, int chunks, long stride, const double* row_part, int Np, int row_chunks,
                       double* svec);

// ---- kernels_loo.hip: leave-one-out cross-validation (sls_nll_loo, sls_gp_loo_grad, sls_gp_loo) ---------------------------------
// With d_i = (K_y^-1)_ii = dvec[i*dstride] (Kinv with stride Np + 1, or a vector), one workgroup writes, for i < N (exactly 0 for
// N <= i < Np): mu[i] = y_i - alpha_i / d_i, var[i] = 1 / d_i, logp[i] = 1/2 log d_i - alpha_i^2 / (2 d_i) - 1/2 log 2 pi,
// ad[i] = alpha_i / d_i, sc[i] = sqrt(c_i), c_i = 1/2 (1 + alpha_i^2 / d_i) / d_i; and Lsum[0] = sum_i logp[i]: 256 partial sums over
// i mod 256 in increasing i, then the binary tree.
void launch_loo_terms(hipStream_t s, const double* dvec, long dstride, const double* alpha, const double* y, int Np, int N, double* mu,
                      double* var, double* logp, double* ad, double* sc, double* Lsum);
// d[i] = sum_k (L^-1)_ki^2, i < N: diag(K_y^-1) from L^-1 alone (lower triangular, [k + i*Np])
void launch_loo_diag_linv(hipStream_t s, const double* Linv, int Np, int N, double* d);
// R = Kinv diag(sc) (one N^2 pass, Np x Np), then M = R R^T = Kinv diag(c) Kinv on the fp64 matrix cores: only the nt (nt + 1) / 2
// tiles with tm >= tn are computed and written (N^3 flop); the tiles of M above the diagonal keep whatever they held.
void launch_loo_syrk(hipStream_t s, const double* Kinv, const double* sc, int Np, double* R, double* M);
// launch_nll_weight / launch_nll_weight_direct with the LOO weights w_ij = 1/2 (u_i alpha_j + alpha_i u_j) - M_ij (0 for a padded
// index), M read from its lower triangle only (entry (i, j), i < j, reads M_ji): the same G, wk_part and row_part in the same orders.
void launch_loo_weight(hipStream_t s, const double* XT, long ld, int Dp, const double* nx, int Np, int N, KernelSpec ks,
                       const double* alpha, const double* u, const double* M, double* G, double* wk_part, double* row_part);
void launch_loo_weight_direct(hipStream_t s, const double* X, int D, const double* inv_ell, int Np, int N, KernelSpec ks,
                              const double* alpha, const double* u, const double* M, double* G, double* wk_part);
// out[0] = sum_t part[t], out[1] = dL/db = sum_{i < N} (u_i alpha_i - M_ii), both in launch_nll_scalars' orders
void launch_loo_scalars(hipStream_t s, const double* part, int nparts, const double* alpha, const double* u, const double* M, int Np,
                        int N, double* out);

// ---- kernels_laplace.hip: Laplace posterior of the goodness values (sls_gp_set_laplace) ----------------------------------------
// W (Np x Np, zero in the padding) = the Hessian of the Bradley-Terry-Luce terms at y: per tuple (diag(p) - p p^T) / s^2, p = softmax
// (y / s) with the maximum subtracted, scattered at the tuple's indices.  off / flat: the CSR of the tuples; csc_off / csc_ent: the
// flat positions that name point i, increasing; tuple_of[e]: the tuple of flat position e (all device ints).  P (flat length) and
// logp0 (n_prefs) receive the probabilities and log p of each tuple's first member.  No atomics: one lane owns one row, fixed order.
void launch_laplace_w(hipStream_t s, const int* off, const int* flat, const int* csc_off, const int* csc_ent, const int* tuple_of,
                      int n_prefs, const double* y, double btl_scale, int N, int Np, double* P, double* logp0, double* W);
// A[r + c*Np] <- A[c + r*Np] for r < c: exactly symmetric from the lower triangle
void launch_mirror_lower(hipStream_t s, double* A, int Np);
// out[0] = sum_t logp0[t], out[1] = 2 sum_{i<N} log LB_ii, out[2] = y . alpha: one workgroup, one fixed order
void launch_laplace_summary(hipStream_t s, const double* logp0, int n_prefs, const double* LB, int Np, int N, const double* y,
                            const double* alpha, double* out);
// launch_gemm_plain on the tiles with tm >= tn only (square nt x nt outputs): the lower tiles of a symmetric product; the tiles above
// the diagonal keep what they held (launch_mirror_lower fills them)
void launch_gemm_lower_tiles(hipStream_t s, const double* A, long lda, bool a_kc, const double* B, long ldb, bool b_kc, double* C,
                             long ldc, int nt, int K, double alpha, double beta);

}  // namespace slsk
