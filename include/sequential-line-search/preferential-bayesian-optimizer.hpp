// Preferential Bayesian optimisation with discrete-choice queries
// (reference surface: include/sequential-line-search/preferential-bayesian-optimizer.hpp:16-160).  Search space [0,1]^D.
#ifndef SEQUENTIAL_LINE_SEARCH_PREFERENTIAL_BAYESIAN_OPTIMIZER_HPP
#define SEQUENTIAL_LINE_SEARCH_PREFERENTIAL_BAYESIAN_OPTIMIZER_HPP

#include <functional>
#include <memory>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/current-best-selection-strategy.hpp>
#include <sequential-line-search/eigen-lite.hpp>
#include <sequential-line-search/kernel-type.hpp>
#include <string>
#include <vector>

namespace sequential_line_search
{
    class PreferenceRegressor;
    class PreferenceDataManager;

    /// (number of dimensions, number of options per query) -> the first query.
    using InitialQueryGenerator = std::function<std::vector<Eigen::VectorXd>(const int, const int)>;

    std::vector<Eigen::VectorXd> GenerateRandomPoints(const int num_dims, const int num_options);

    class PreferentialBayesianOptimizer
    {
    public:
        PreferentialBayesianOptimizer(const int num_dims, const bool use_map_hyperparams = true,
                                      const KernelType             kernel_type             = KernelType::ArdMatern52Kernel,
                                      const AcquisitionFuncType    acquisition_func_type   = AcquisitionFuncType::ExpectedImprovement,
                                      const InitialQueryGenerator& initial_query_generator = GenerateRandomPoints,
                                      const CurrentBestSelectionStrategy current_best_selection_strategy =
                                          CurrentBestSelectionStrategy::LargestExpectValue,
                                      const int num_options = 2);

        void SetHyperparams(const double kernel_signal_var = 0.500, const double kernel_length_scale = 0.500,
                            const double noise_level = 0.005, const double kernel_hyperparams_prior_var = 0.250,
                            const double btl_scale = 0.010);

        /// option_index: zero-based index into GetCurrentOptions().  num_map_estimation_iters <= 0: heuristic
        /// 10 (D + number of data points).
        void SubmitFeedbackData(const int option_index, const int num_map_estimation_iters = 0);

        /// Same with arbitrary options instead of the ones proposed by the optimizer.
        void SubmitCustomFeedbackData(const Eigen::VectorXd& chosen_option, const std::vector<Eigen::VectorXd>& other_options,
                                      const int num_map_estimation_iters = 0);

        /// Builds the next query: option 0 = current best, the others from FindNextPoints.  Non-positive arguments select
        /// the reference's multi-start heuristic (500 D starts, 10 D local evaluations).
        void DetermineNextQuery(const int num_global_search_iters = 0, const int num_local_search_iters = 0);
        /// Opt-in alternative: option 0 as in DetermineNextQuery, the other options the maximisers of m_num_options - 1 pathwise
        /// posterior draws (acquisition_func::FindNextPointsByThompsonSampling with stream `seed`).  Non-positive arguments select
        /// the same heuristic as DetermineNextQuery.
        void DetermineNextQueryByThompsonSampling(const unsigned long long seed, const int num_global_search_iters = 0,
                                                  const int num_local_search_iters = 0);
        /// Opt-in alternative for two-option queries: BOTH options are the maximiser (x, x') of the expected utility of the best
        /// option E[max(f(x), f(x'))] (acquisition_func::FindNextQueryPairByExpectedUtility with start stream `seed`); the current
        /// best is not forced into the query.  The option with the larger posterior mean becomes option 0 (GetMaximizer()).
        /// num_options != 2 throws std::invalid_argument; before any feedback it throws as DetermineNextQuery does; non-positive
        /// arguments select the same heuristic as DetermineNextQuery.
        void DetermineNextQueryByExpectedUtility(const unsigned long long seed, const int num_global_search_iters = 0,
                                                 const int num_local_search_iters = 0);
        /// Opt-in alternative for ANY num_options >= 2: ALL options are the joint maximiser of the expected utility of the best
        /// option on num_draws posterior draws (acquisition_func::FindNextQueryByExpectedUtility with draw and start stream `seed`).
        /// The option with the largest posterior mean is moved to position 0 (GetMaximizer()); the others keep their order.  Before
        /// any feedback it throws as DetermineNextQuery does; non-positive iteration counts select the same heuristic.
        void DetermineNextQueryByExpectedUtilityOfDraws(const unsigned long long seed, const int num_draws = 256,
                                                        const int num_global_search_iters = 0, const int num_local_search_iters = 0);
        /// Opt-in alternative that explores: ALL options are the joint maximiser of the information the user's answer is expected to
        /// give about the latent function (acquisition_func::FindNextQueryByInformationGain with draw and start stream `seed`) under
        /// the BTL likelihood of scale btl_scale; btl_scale <= 0 means the optimiser's own (the constructor's btl_scale).  The
        /// option with the largest posterior mean is moved to position 0 (GetMaximizer()); the others keep their order.  Before any
        /// feedback it throws as DetermineNextQuery does; non-positive iteration counts select the same heuristic.
        void DetermineNextQueryByInformationGain(const unsigned long long seed, const int num_draws = 256,
                                                 const int num_global_search_iters = 0, const int num_local_search_iters = 0,
                                                 const double btl_scale = 0.0);
        /// Opt-in alternative: option 0 as in DetermineNextQuery, the other m_num_options - 1 options the JOINT maximiser of noisy
        /// expected improvement on num_draws posterior draws (acquisition_func::FindNextPointsByNoisyExpectedImprovement with draw
        /// and start stream `seed`): improvement over the per-draw incumbent rather than over a known best value, which a
        /// preference model does not have.  Before any feedback it throws as DetermineNextQuery does; non-positive iteration counts
        /// select the same heuristic.
        void DetermineNextQueryByNoisyExpectedImprovement(const unsigned long long seed, const int num_draws = 256,
                                                          const int num_global_search_iters = 0, const int num_local_search_iters = 0);
        /// The same with the log form of the criterion (acquisition_func::FindNextPointsByLogNoisyExpectedImprovement): starts that
        /// no draw improves still move.
        void DetermineNextQueryByLogNoisyExpectedImprovement(const unsigned long long seed, const int num_draws = 256,
                                                             const int num_global_search_iters = 0, const int num_local_search_iters = 0,
                                                             const double tau_relu = 1e-6, const double tau_max = 1e-2);

        const std::vector<Eigen::VectorXd>& GetCurrentOptions() const { return m_current_options; }
        Eigen::VectorXd                     GetMaximizer() const;

        double GetPreferenceValueMean(const Eigen::VectorXd& point) const;
        double GetPreferenceValueStdev(const Eigen::VectorXd& point) const;
        double GetAcquisitionFuncValue(const Eigen::VectorXd& point) const;

        /// Batched forms of the three accessors above (additions of this build: SURVEY.md 8(f3)): one query point per column of
        /// `points` (D x M), ONE device pass each -- what the reference's GUI demo does pixel by pixel
        /// (demos/bayesian_optimization_2d_gui/mainwidget.cpp:41-72).  Zeros while there is no data, like the scalar forms.
        Eigen::VectorXd GetPreferenceValueMeans(const Eigen::MatrixXd& points) const;
        Eigen::VectorXd GetPreferenceValueStdevs(const Eigen::MatrixXd& points) const;
        Eigen::VectorXd GetAcquisitionFuncValues(const Eigen::MatrixXd& points) const;

        /// Joint posterior of the preference values at the points (D x M): their M x M covariance (Regressor::PredictCovariance),
        /// and num_samples draws of them, one per column (M x num_samples, Regressor::SamplePosterior; same seed, same bits).
        /// Zeros while there is no data, like the accessors above.
        Eigen::MatrixXd GetPreferenceValueCovariance(const Eigen::MatrixXd& points) const;
        Eigen::MatrixXd SamplePreferenceValues(const Eigen::MatrixXd& points, const int num_samples, const unsigned long long seed) const;

        const Eigen::MatrixXd& GetRawDataPoints() const;
        void                   DampData(const std::string& directory_path) const;

        void SetGaussianProcessUpperConfidenceBoundHyperparam(const double hyperparam)
        {
            m_gaussian_process_upper_confidence_bound_hyperparam = hyperparam;
        }

        /// Laplace posterior of the goodness values (PreferenceRegressor::UseLaplacePosterior) for every regressor the
        /// SubmitFeedbackData* calls build from now on, and for the current one.  Off by default: today's behaviour, bit for bit.
        void SetUseLaplacePosterior(const bool use_laplace_posterior);
        bool GetUseLaplacePosterior() const { return m_use_laplace_posterior; }

    private:
        /// q options from (q, n_global, n_local): the part in which the two query builders differ
        using OptionGenerator = std::function<std::vector<Eigen::VectorXd>(int, int, int)>;
        void BuildNextQuery(const char* caller, int num_global_search_iters, int num_local_search_iters, const OptionGenerator& generate);

        const bool m_use_map_hyperparams;
        const int  m_num_options;

        const CurrentBestSelectionStrategy m_current_best_selection_strategy;

        std::shared_ptr<PreferenceRegressor>   m_regressor;
        bool                                   m_use_laplace_posterior = false;
        std::shared_ptr<PreferenceDataManager> m_data;
        std::vector<Eigen::VectorXd>           m_current_options;

        double m_kernel_signal_var;
        double m_kernel_length_scale;
        double m_noise_level;
        double m_kernel_hyperparams_prior_var;
        double m_btl_scale;

        const KernelType          m_kernel_type;
        const AcquisitionFuncType m_acquisition_func_type;

        double m_gaussian_process_upper_confidence_bound_hyperparam;

        void PerformMapEstimation(const int num_map_estimation_iters);
    };
} // namespace sequential_line_search

#endif
