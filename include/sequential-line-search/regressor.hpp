// Abstract regressor + Gram-matrix builders (reference surface: include/sequential-line-search/regressor.hpp:10-72).
// Every builder below runs on the MI355X through the C ABI (include/sls_hip.h).
#ifndef SEQUENTIAL_LINE_SEARCH_REGRESSOR_HPP
#define SEQUENTIAL_LINE_SEARCH_REGRESSOR_HPP

#include <sequential-line-search/eigen-lite.hpp>
#include <sequential-line-search/kernel-type.hpp>
#include <utility>
#include <vector>

struct sls_gp;
struct sls_path;

namespace sequential_line_search
{
    struct SearchSubspace;   // acquisition-function.hpp

    class Regressor
    {
    public:
        Regressor(const KernelType kernel_type);
        virtual ~Regressor() {}

        unsigned GetNumDims() const { return GetLargeX().rows(); }

        virtual double PredictMu(const Eigen::VectorXd& x) const    = 0;
        virtual double PredictSigma(const Eigen::VectorXd& x) const = 0;

        virtual Eigen::VectorXd PredictMuDerivative(const Eigen::VectorXd& x) const    = 0;
        virtual Eigen::VectorXd PredictSigmaDerivative(const Eigen::VectorXd& x) const = 0;

        virtual const Eigen::VectorXd& GetKernelHyperparams() const = 0;
        virtual double                 GetNoiseHyperparam() const   = 0;

        virtual const Eigen::MatrixXd& GetLargeX() const = 0;
        virtual const Eigen::VectorXd& GetSmallY() const = 0;

        /// argmax_i PredictMu(x_i) over the data points.  For the built-in regressors this is hoisted to fit time
        /// (mu(x_i) = y_i - b alpha_i); a user subclass without a device handle gets the reference's N x PredictMu loop.
        Eigen::VectorXd PredictMaximumPointFromData() const;

        Kernel                   GetKernel() const { return m_kernel; }
        KernelThetaDerivative    GetKernelThetaDerivative() const { return m_kernel_theta_derivative; }
        KernelFirstArgDerivative GetKernelFirstArgDerivative() const { return m_kernel_first_arg_derivative; }
        KernelType               GetKernelType() const { return m_kernel_type; }

        /// Device-resident state (K_y^-1, alpha, ...) or nullptr; used by acquisition_func for batched evaluation.
        virtual sls_gp* GetDeviceHandle() const { return nullptr; }
        /// true when the device handle carries the Laplace posterior of a preference model (PreferenceRegressor::UseLaplacePosterior):
        /// every sigma above is then the Laplace variance, and the routes that cannot honour it refuse the regressor.
        virtual bool UsesLaplacePosterior() const { return false; }

        // Batched forms (not in the reference; D x M input, one query point per column).
        void PredictBatch(const Eigen::MatrixXd& Xs, Eigen::VectorXd& mu, Eigen::VectorXd& sigma) const;

        /// Joint posterior of the latent function at the M query points (D x M): the M x M covariance
        /// K(Xs, Xs) - K*^T K_y^-1 K*, exactly symmetric, diagonal not clamped (sls_gp_predict_cov).  M <= 8192.
        /// Both calls below need the device handle: a user subclass without one gets a 0 x 0 matrix.
        Eigen::MatrixXd PredictCovariance(const Eigen::MatrixXd& Xs) const;
        /// num_samples draws f ~ N(mu, cov + j I) at the M query points, one draw per column (M x num_samples); the same seed gives
        /// the same bits, and the first k columns do not depend on num_samples (sls_gp_sample_posterior).  jitter_used (may be
        /// nullptr) receives j.
        Eigen::MatrixXd SamplePosterior(const Eigen::MatrixXd& Xs, int num_samples, unsigned long long seed,
                                        double* jitter_used = nullptr) const;
        /// num_draws pathwise posterior function draws (sls_path_create): closed-form functions that can be evaluated -- and
        /// maximised -- anywhere in [0,1]^D, from num_frequencies random features shared by all draws.  Needs the device handle
        /// (std::invalid_argument otherwise).  The object holds a snapshot of this regressor's fit and must not outlive it.
        class PosteriorFunctionSamples SamplePosteriorFunctions(int num_draws, unsigned long long seed, int num_frequencies = 2048) const;

    protected:
        KernelType               m_kernel_type;
        Kernel                   m_kernel;
        KernelThetaDerivative    m_kernel_theta_derivative;
        KernelFirstArgDerivative m_kernel_first_arg_derivative;
    };

    /// Posterior function draws of a fitted regressor (Regressor::SamplePosteriorFunctions; include/sls_hip.h sls_path_*).  The
    /// draws share one set of random frequencies: each is an exact draw from the random-feature-approximate posterior, and the
    /// O(a / sqrt(F)) error of that prior is common to all of them.  Move-only.
    class PosteriorFunctionSamples
    {
    public:
        /// handle: a fitted device handle of num_dims dimensions (Regressor::GetDeviceHandle).
        PosteriorFunctionSamples(sls_gp* handle, int num_dims, int num_draws, unsigned long long seed, int num_frequencies);
        PosteriorFunctionSamples(PosteriorFunctionSamples&& other) noexcept;
        PosteriorFunctionSamples& operator=(PosteriorFunctionSamples&& other) noexcept;
        PosteriorFunctionSamples(const PosteriorFunctionSamples&) = delete;
        PosteriorFunctionSamples& operator=(const PosteriorFunctionSamples&) = delete;
        ~PosteriorFunctionSamples();

        int GetNumDraws() const { return m_num_draws; }
        /// Every draw at every column of Xs (D x M): M x num_draws.
        Eigen::MatrixXd Evaluate(const Eigen::MatrixXd& Xs) const;
        /// Gradient of draw `draw` at x (D).
        Eigen::VectorXd EvaluateDerivative(const Eigen::VectorXd& x, int draw) const;
        /// One maximiser per draw: starts is D x (num_draws S), columns [s S, (s + 1) S) start draw s; one lock-step bounded L-BFGS
        /// of num_local_search_iters evaluations per start (the acquisition maximiser's local search tolerances); per draw the
        /// best end point.  values (may be nullptr) receives the draws' maxima.
        std::vector<Eigen::VectorXd> Maximize(const Eigen::MatrixXd& starts, unsigned num_local_search_iters,
                                              Eigen::VectorXd* values = nullptr) const;
        /// Maximize with every draw searched over the affine subspace x = offset + basis z, z in [0,1]^d (SearchSubspace,
        /// acquisition-function.hpp; include/sls_hip.h sls_path_maximize_sub): starts_z is d x (num_draws S).  Returns the draws'
        /// best points x (D each); values (may be nullptr) receives their maxima over the subspace.
        std::vector<Eigen::VectorXd> MaximizeInSubspace(const SearchSubspace& subspace, const Eigen::MatrixXd& starts_z,
                                                        unsigned num_local_search_iters, Eigen::VectorXd* values = nullptr) const;
        /// Expected utility of the best of q = options.size() options on these draws (qEUBO, Astudillo et al. 2023; include/sls_hip.h
        /// sls_qeubo_*): set m is (options[0].col(m), .., options[q-1].col(m)), every options[i] D x M, 1 <= q <= 16.  Returns the M
        /// values; grads (may be nullptr) receives q matrices D x M, the gradient with respect to each option; win_counts (may be
        /// nullptr) q x M, the number of draws each option wins (win_counts / GetNumDraws() estimates the probability that it is
        /// chosen).  One device pass.
        Eigen::VectorXd CalcExpectedUtilitiesOfBestOption(const std::vector<Eigen::MatrixXd>& options,
                                                          std::vector<Eigen::MatrixXd>* grads = nullptr,
                                                          Eigen::MatrixXi* win_counts = nullptr) const;
        /// Maximiser of that utility over [0,1]^(qD): starts is (num_options D) x S, rows iD..iD+D-1 start option i; one lock-step
        /// bounded L-BFGS of num_local_search_iters evaluations per start (the acquisition maximiser's local search tolerances),
        /// the best end point split into its num_options options.  value (may be nullptr) receives the utility there.
        std::vector<Eigen::VectorXd> MaximizeExpectedUtilityOfBestOption(int num_options, const Eigen::MatrixXd& starts,
                                                                         unsigned num_local_search_iters, double* value = nullptr) const;
        /// Per draw, the maximum over the columns of Xb (D x Mb, Mb >= 1; include/sls_hip.h sls_path_max_over_points): the draws'
        /// incumbents when Xb is the data.  arg (may be nullptr) receives the lowest column that attains each maximum.
        Eigen::VectorXd MaxOverPoints(const Eigen::MatrixXd& Xb, Eigen::VectorXi* arg = nullptr) const;
        /// Noisy expected improvement of q = options.size() points on these draws over the per-draw baseline (qNEI, Letham et al.
        /// 2019; include/sls_hip.h sls_qnei_*): (1 / num_draws) sum_s max(0, max_i f_s(x_i) - baseline_s), baseline of num_draws
        /// finite values (MaxOverPoints at the data; a constant gives Monte-Carlo qEI).  Arguments and results as
        /// CalcExpectedUtilitiesOfBestOption; a draw that nobody improves has no winner, so a column of win_counts sums to at most
        /// num_draws.
        Eigen::VectorXd CalcNoisyExpectedImprovements(const std::vector<Eigen::MatrixXd>& options, const Eigen::VectorXd& baseline,
                                                      std::vector<Eigen::MatrixXd>* grads = nullptr,
                                                      Eigen::MatrixXi* win_counts = nullptr) const;
        /// Maximiser of that improvement over [0,1]^(num_points D): as MaximizeExpectedUtilityOfBestOption.  A start that no draw
        /// improves is stationary (value 0, zero gradient) and does not move.
        std::vector<Eigen::VectorXd> MaximizeNoisyExpectedImprovement(int num_points, const Eigen::VectorXd& baseline,
                                                                      const Eigen::MatrixXd& starts, unsigned num_local_search_iters,
                                                                      double* value = nullptr) const;
        /// Log-space noisy expected improvement (qLogNEI after Ament et al. 2023; include/sls_hip.h sls_qlognei_*): the smooth log
        /// form of CalcNoisyExpectedImprovements -- a softplus of temperature tau_relu for max(0, .), a log-sum-exp of temperature
        /// tau_max for the max over the points, a log-sum-exp over the draws.  Arguments and results as
        /// CalcNoisyExpectedImprovements (win_counts are its hard counts); a set that no draw improves has a finite value and a
        /// nonzero gradient.
        Eigen::VectorXd CalcLogNoisyExpectedImprovements(const std::vector<Eigen::MatrixXd>& options, const Eigen::VectorXd& baseline,
                                                         std::vector<Eigen::MatrixXd>* grads = nullptr,
                                                         Eigen::MatrixXi* win_counts = nullptr, double tau_relu = 1e-6,
                                                         double tau_max = 1e-2) const;
        /// Maximiser of that criterion over [0,1]^(num_points D): as MaximizeNoisyExpectedImprovement, but a start that no draw
        /// improves moves.
        std::vector<Eigen::VectorXd> MaximizeLogNoisyExpectedImprovement(int num_points, const Eigen::VectorXd& baseline,
                                                                         const Eigen::MatrixXd& starts, unsigned num_local_search_iters,
                                                                         double* value = nullptr, double tau_relu = 1e-6,
                                                                         double tau_max = 1e-2) const;
        /// Information gain of a choice query (qBALD; include/sls_hip.h sls_qbald_*): the mutual information between the user's pick
        /// among options[i].col(m), i = 0 .. q-1, and the latent function, under the BTL likelihood of the given scale
        /// (PreferenceRegressor's btl_scale), estimated on the draws.  options as for CalcExpectedUtilitiesOfBestOption.  Returns the M
        /// values, each in [0, ln q]; *grads (optional) the gradients, *probabilities (optional, q x M) the predicted probability that
        /// the user picks option i -- what a held-out preference log-loss is computed from --, *win_counts (optional, q x M) the hard
        /// win counts of CalcExpectedUtilitiesOfBestOption.
        Eigen::VectorXd CalcChoiceInformationGains(const std::vector<Eigen::MatrixXd>& options, double scale,
                                                   std::vector<Eigen::MatrixXd>* grads = nullptr, Eigen::MatrixXd* probabilities = nullptr,
                                                   Eigen::MatrixXi* win_counts = nullptr) const;
        /// Maximiser of that criterion over [0,1]^(num_options D): as MaximizeExpectedUtilityOfBestOption.
        std::vector<Eigen::VectorXd> MaximizeChoiceInformationGain(int num_options, double scale, const Eigen::MatrixXd& starts,
                                                                   unsigned num_local_search_iters, double* value = nullptr) const;
        /// Expected utility of the best of num_positions grid positions on the slider from ends_a.col(m) to ends_b.col(m) (line EUBO;
        /// include/sls_hip.h sls_line_*): CalcExpectedUtilitiesOfBestOption at the positions (1 - t_i) a + t_i b, t_i = i /
        /// (num_positions - 1), 2 <= num_positions <= 16 -- Slider::GetValue on the grid.  ends_a, ends_b D x M.  Returns the M values;
        /// grad_a, grad_b (may be nullptr) receive the gradients with respect to the two ends (D x M each, the chain rule on the
        /// positions' gradients), win_counts (may be nullptr) num_positions x M, the number of draws each position wins (win_counts
        /// / GetNumDraws() estimates the probability that the user stops there).  With baseline (num_draws finite values) the
        /// criterion is CalcNoisyExpectedImprovements at the same positions.
        Eigen::VectorXd CalcExpectedUtilitiesOfBestSliderPosition(const Eigen::MatrixXd& ends_a, const Eigen::MatrixXd& ends_b,
                                                                  int num_positions, Eigen::MatrixXd* grad_a = nullptr,
                                                                  Eigen::MatrixXd* grad_b = nullptr, Eigen::MatrixXi* win_counts = nullptr,
                                                                  const Eigen::VectorXd* baseline = nullptr) const;
        /// Maximiser of that utility over the ends: starts is 2D x S (rows 0..D-1 start the first end), or with `anchor` (D values;
        /// the first end of every slider, e.g. the current best point) D x S, the second end alone -- 2D or D variables whatever
        /// num_positions is.  One lock-step bounded L-BFGS of num_local_search_iters evaluations per start (the acquisition
        /// maximiser's local search tolerances); returns the best slider's two ends (the first is the anchor when there is one).
        /// value (may be nullptr) receives the utility there.
        std::pair<Eigen::VectorXd, Eigen::VectorXd> MaximizeExpectedUtilityOfBestSliderPosition(
            int num_positions, const Eigen::MatrixXd& starts, unsigned num_local_search_iters, const Eigen::VectorXd* anchor = nullptr,
            const Eigen::VectorXd* baseline = nullptr, double* value = nullptr) const;
        /// Expected utility of the best cell of a grid_s x grid_t grid on the bilinear patch spanned by the corners corners00.col(m),
        /// corners10.col(m), corners01.col(m), corners11.col(m) (gallery EUBO; include/sls_hip.h sls_patch_*):
        /// CalcExpectedUtilitiesOfBestOption at the cells (1 - t_j) ((1 - s_i) c00 + s_i c10) + t_j ((1 - s_i) c01 + s_i c11), s_i =
        /// i / (grid_s - 1), t_j = j / (grid_t - 1), grid_s, grid_t >= 2 and grid_s grid_t <= 16.  Every corner block D x M.  Returns
        /// the M values; grads (may be nullptr) receives four matrices D x M, the gradients with respect to c00, c10, c01, c11;
        /// win_counts (may be nullptr) (grid_s grid_t) x M, the number of draws cell i + grid_s j wins.  With baseline (num_draws
        /// finite values) the criterion is CalcNoisyExpectedImprovements at the same cells.
        Eigen::VectorXd CalcExpectedUtilitiesOfBestGalleryCell(const Eigen::MatrixXd& corners00, const Eigen::MatrixXd& corners10,
                                                               const Eigen::MatrixXd& corners01, const Eigen::MatrixXd& corners11,
                                                               int grid_s, int grid_t, std::vector<Eigen::MatrixXd>* grads = nullptr,
                                                               Eigen::MatrixXi* win_counts = nullptr,
                                                               const Eigen::VectorXd* baseline = nullptr) const;
        /// Maximiser of that utility over the corners: starts is 4D x S (rows in blocks of D start c00, c10, c01, c11), or with
        /// `anchor` (D values; the corner c00 of every patch, e.g. the current best point) 3D x S, the other three corners -- 4D or 3D
        /// variables whatever the grid.  One lock-step bounded L-BFGS of num_local_search_iters evaluations per start (the
        /// acquisition maximiser's local search tolerances); returns the best patch's four corners c00, c10, c01, c11 (the first is
        /// the anchor when there is one).  value (may be nullptr) receives the utility there.
        std::vector<Eigen::VectorXd> MaximizeExpectedUtilityOfBestGalleryCell(int grid_s, int grid_t, const Eigen::MatrixXd& starts,
                                                                              unsigned               num_local_search_iters,
                                                                              const Eigen::VectorXd* anchor   = nullptr,
                                                                              const Eigen::VectorXd* baseline = nullptr,
                                                                              double*                value    = nullptr) const;

    private:
        // the set criteria of every kind: baseline == nullptr is the expected utility of the best option, taus != nullptr
        // (tau_relu, tau_max) the log form of the noisy expected improvement, scale != nullptr (the BTL scale, without a baseline) the
        // information gain of the choice, with its optional probabilities
        Eigen::VectorXd              CalcSetCriterion(const char* who, const std::vector<Eigen::MatrixXd>& options,
                                                      const Eigen::VectorXd* baseline, std::vector<Eigen::MatrixXd>* grads,
                                                      Eigen::MatrixXi* win_counts, const double* taus = nullptr,
                                                      const double* scale = nullptr, Eigen::MatrixXd* probabilities = nullptr) const;
        std::vector<Eigen::VectorXd> MaximizeSetCriterion(const char* who, int num_options, const Eigen::VectorXd* baseline,
                                                          const Eigen::MatrixXd& starts, unsigned num_local_search_iters,
                                                          double* value, const double* taus = nullptr,
                                                          const double* scale = nullptr) const;

        sls_path* m_path      = nullptr;
        int       m_num_draws = 0;
        int       m_num_dims  = 0;
    };

    // k
    Eigen::VectorXd CalcSmallK(const Eigen::VectorXd& x, const Eigen::MatrixXd& X, const Eigen::VectorXd& kernel_hyperparameters,
                               const Kernel kernel);
    // K_y = K_f + sigma^2 I
    Eigen::MatrixXd CalcLargeKY(const Eigen::MatrixXd& X, const Eigen::VectorXd& kernel_hyperparameters, const double noise_level,
                                const Kernel kernel);
    // K_f
    Eigen::MatrixXd CalcLargeKF(const Eigen::MatrixXd& X, const Eigen::VectorXd& kernel_hyperparameters, const Kernel kernel);
    // partial k / partial x  (D x N).  Rarely needed: the predictors contract it on the device without forming it.
    Eigen::MatrixXd CalcSmallKSmallXDerivative(const Eigen::VectorXd& x, const Eigen::MatrixXd& X,
                                               const Eigen::VectorXd&         kernel_hyperparameters,
                                               const KernelFirstArgDerivative kernel_first_arg_derivative);
    // partial K_y / partial theta: (D+1) dense N x N matrices.  Kept for API compatibility only (O(D N^2) memory);
    // the MAP objectives use the fused contraction of sls_nll_eval instead.
    std::vector<Eigen::MatrixXd> CalcLargeKYThetaDerivative(const Eigen::MatrixXd& X, const Eigen::VectorXd& kernel_hyperparameters,
                                                            const KernelThetaDerivative kernel_theta_derivative);
    // partial K_y / partial sigma^2 = I
    Eigen::MatrixXd CalcLargeKYNoiseLevelDerivative(const Eigen::MatrixXd& X, const Eigen::VectorXd& kernel_hyperparameters,
                                                    const double noise_level);
} // namespace sequential_line_search

#endif
