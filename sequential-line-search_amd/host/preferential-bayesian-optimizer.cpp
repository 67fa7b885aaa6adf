// PreferentialBayesianOptimizer facade (reference: src/preferential-bayesian-optimizer.cpp) -- the second caller of the
// device path (PreferenceRegressor MAP + FindNextPoints).
#include <algorithm>
#include <string>
#include <sequential-line-search/preference-data-manager.hpp>
#include <sequential-line-search/preference-regressor.hpp>
#include <sequential-line-search/preferential-bayesian-optimizer.hpp>
#include <sequential-line-search/utils.hpp>
#include <stdexcept>

using Eigen::VectorXd;

namespace sequential_line_search
{
    // reference: src/preferential-bayesian-optimizer.cpp:11-20
    std::vector<VectorXd> GenerateRandomPoints(const int num_dims, const int num_options)
    {
        std::vector<VectorXd> options;
        for (int i = 0; i < num_options; ++i) options.push_back(utils::GenerateRandomVector(num_dims));
        return options;
    }

    // reference: :22-47
    PreferentialBayesianOptimizer::PreferentialBayesianOptimizer(const int num_dims, const bool use_map_hyperparams,
                                                                 const KernelType kernel_type, const AcquisitionFuncType acquisition_func_type,
                                                                 const InitialQueryGenerator&       initial_query_generator,
                                                                 const CurrentBestSelectionStrategy current_best_selection_strategy,
                                                                 const int                          num_options)
        : m_use_map_hyperparams(use_map_hyperparams),
          m_num_options(num_options),
          m_current_best_selection_strategy(current_best_selection_strategy),
          m_kernel_signal_var(0.500),
          m_kernel_length_scale(0.500),
          m_noise_level(0.005),
          m_kernel_hyperparams_prior_var(0.250),
          m_btl_scale(0.010),
          m_kernel_type(kernel_type),
          m_acquisition_func_type(acquisition_func_type),
          m_gaussian_process_upper_confidence_bound_hyperparam(1.0)
    {
        if (num_options < 2) throw std::invalid_argument("PreferentialBayesianOptimizer: num_options must be >= 2");
        m_data            = std::make_shared<PreferenceDataManager>();
        m_current_options = initial_query_generator(num_dims, num_options);
        if (static_cast<int>(m_current_options.size()) != num_options)
            throw std::invalid_argument("PreferentialBayesianOptimizer: the initial query generator returned a wrong number of options");
    }

    void PreferentialBayesianOptimizer::SetHyperparams(const double kernel_signal_var, const double kernel_length_scale,
                                                       const double noise_level, const double kernel_hyperparams_prior_var,
                                                       const double btl_scale)
    {
        m_kernel_signal_var            = kernel_signal_var;
        m_kernel_length_scale          = kernel_length_scale;
        m_noise_level                  = noise_level;
        m_kernel_hyperparams_prior_var = kernel_hyperparams_prior_var;
        m_btl_scale                    = btl_scale;
    }

    // reference: :64-81
    void PreferentialBayesianOptimizer::SubmitFeedbackData(const int option_index, const int num_map_estimation_iters)
    {
        if (option_index < 0 || option_index >= static_cast<int>(m_current_options.size()))
            throw std::out_of_range("PreferentialBayesianOptimizer::SubmitFeedbackData: option_index");
        std::vector<VectorXd> others;
        for (int i = 0; i < static_cast<int>(m_current_options.size()); ++i)
            if (i != option_index) others.push_back(m_current_options[i]);
        SubmitCustomFeedbackData(m_current_options[option_index], others, num_map_estimation_iters);
    }

    // reference: :83-93
    void PreferentialBayesianOptimizer::SubmitCustomFeedbackData(const VectorXd& chosen_option, const std::vector<VectorXd>& other_options,
                                                                 const int num_map_estimation_iters)
    {
        m_data->AddNewPoints(chosen_option, other_options, true);
        PerformMapEstimation(num_map_estimation_iters);
    }

    // Option 0 (current best) and options 1.. from `generate(num_options - 1, n_global, n_local)`; non-positive iteration counts take
    // the reference's multi-start heuristic (:95-141: 500 D starts, 10 D local evaluations).  Shared by both query builders.
    void PreferentialBayesianOptimizer::BuildNextQuery(const char* caller, const int num_global_search_iters, const int num_local_search_iters,
                                                       const OptionGenerator& generate)
    {
        if (!m_regressor) throw std::logic_error(std::string("PreferentialBayesianOptimizer::") + caller + " called before any feedback");
        const int num_dims = static_cast<int>(GetMaximizer().size());
        const int n_global = num_global_search_iters > 0 ? num_global_search_iters : 500 * num_dims;
        const int n_local  = num_local_search_iters > 0 ? num_local_search_iters : 10 * num_dims;

        const VectorXd x_plus = (m_current_best_selection_strategy == CurrentBestSelectionStrategy::LargestExpectValue)
                                    ? m_regressor->FindArgMax()
                                    : m_data->GetLastSelectedDataPoint();
        const std::vector<VectorXd> next = generate(m_num_options - 1, n_global, n_local);
        m_current_options[0] = x_plus;
        for (int i = 1; i < m_num_options; ++i) m_current_options[i] = next[i - 1];
    }

    void PreferentialBayesianOptimizer::DetermineNextQuery(const int num_global_search_iters, const int num_local_search_iters)
    {
        BuildNextQuery("DetermineNextQuery", num_global_search_iters, num_local_search_iters, [&](int q, int n_global, int n_local) {
            return acquisition_func::FindNextPoints(*m_regressor, q, n_global, n_local, m_acquisition_func_type,
                                                    m_gaussian_process_upper_confidence_bound_hyperparam);
        });
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByThompsonSampling(const unsigned long long seed,
                                                                             const int num_global_search_iters,
                                                                             const int num_local_search_iters)
    {
        BuildNextQuery("DetermineNextQueryByThompsonSampling", num_global_search_iters, num_local_search_iters,
                       [&](int q, int n_global, int n_local) {
                           return acquisition_func::FindNextPointsByThompsonSampling(*m_regressor, q, n_global, n_local, seed);
                       });
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtility(const unsigned long long seed,
                                                                            const int num_global_search_iters,
                                                                            const int num_local_search_iters)
    {
        if (m_num_options != 2)
            throw std::invalid_argument("PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtility: the pair criterion needs "
                                        "num_options == 2");
        if (!m_regressor)
            throw std::logic_error("PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtility called before any feedback");
        const int num_dims = static_cast<int>(GetMaximizer().size());
        const int n_global = num_global_search_iters > 0 ? num_global_search_iters : 500 * num_dims;
        const int n_local  = num_local_search_iters > 0 ? num_local_search_iters : 10 * num_dims;
        const std::pair<VectorXd, VectorXd> q = acquisition_func::FindNextQueryPairByExpectedUtility(*m_regressor, n_global, n_local, seed);
        const bool first_is_better = m_regressor->PredictMu(q.first) >= m_regressor->PredictMu(q.second);
        m_current_options[0] = first_is_better ? q.first : q.second;
        m_current_options[1] = first_is_better ? q.second : q.first;
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtilityOfDraws(const unsigned long long seed, const int num_draws,
                                                                                   const int num_global_search_iters,
                                                                                   const int num_local_search_iters)
    {
        if (!m_regressor)
            throw std::logic_error("PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtilityOfDraws called before any feedback");
        const int num_dims = static_cast<int>(GetMaximizer().size());
        const int n_global = num_global_search_iters > 0 ? num_global_search_iters : 500 * num_dims;
        const int n_local  = num_local_search_iters > 0 ? num_local_search_iters : 10 * num_dims;
        std::vector<VectorXd> q = acquisition_func::FindNextQueryByExpectedUtility(*m_regressor, m_num_options, std::max(1, num_draws),
                                                                                   n_global, n_local, seed);
        int    best    = 0;
        double mu_best = m_regressor->PredictMu(q[0]);
        for (int i = 1; i < m_num_options; ++i)
        {
            const double mu = m_regressor->PredictMu(q[i]);
            if (mu > mu_best)
            {
                mu_best = mu;
                best    = i;
            }
        }
        std::rotate(q.begin(), q.begin() + best, q.begin() + best + 1);   // the best one to the front, the others keep their order
        for (int i = 0; i < m_num_options; ++i) m_current_options[i] = q[i];
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByInformationGain(const unsigned long long seed, const int num_draws,
                                                                            const int num_global_search_iters,
                                                                            const int num_local_search_iters, const double btl_scale)
    {
        if (!m_regressor)
            throw std::logic_error("PreferentialBayesianOptimizer::DetermineNextQueryByInformationGain called before any feedback");
        const int num_dims = static_cast<int>(GetMaximizer().size());
        const int n_global = num_global_search_iters > 0 ? num_global_search_iters : 500 * num_dims;
        const int n_local  = num_local_search_iters > 0 ? num_local_search_iters : 10 * num_dims;
        std::vector<VectorXd> q = acquisition_func::FindNextQueryByInformationGain(
            *m_regressor, m_num_options, btl_scale > 0.0 ? btl_scale : m_btl_scale, std::max(1, num_draws), n_global, n_local, seed);
        int    best    = 0;
        double mu_best = m_regressor->PredictMu(q[0]);
        for (int i = 1; i < m_num_options; ++i)
        {
            const double mu = m_regressor->PredictMu(q[i]);
            if (mu > mu_best)
            {
                mu_best = mu;
                best    = i;
            }
        }
        std::rotate(q.begin(), q.begin() + best, q.begin() + best + 1);   // the best one to the front, the others keep their order
        for (int i = 0; i < m_num_options; ++i) m_current_options[i] = q[i];
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByNoisyExpectedImprovement(const unsigned long long seed, const int num_draws,
                                                                                     const int num_global_search_iters,
                                                                                     const int num_local_search_iters)
    {
        BuildNextQuery("DetermineNextQueryByNoisyExpectedImprovement", num_global_search_iters, num_local_search_iters,
                       [&](int q, int n_global, int n_local) {
                           return acquisition_func::FindNextPointsByNoisyExpectedImprovement(*m_regressor, q, std::max(1, num_draws),
                                                                                             n_global, n_local, seed);
                       });
    }

    void PreferentialBayesianOptimizer::DetermineNextQueryByLogNoisyExpectedImprovement(const unsigned long long seed, const int num_draws,
                                                                                        const int num_global_search_iters,
                                                                                        const int num_local_search_iters,
                                                                                        const double tau_relu, const double tau_max)
    {
        BuildNextQuery("DetermineNextQueryByLogNoisyExpectedImprovement", num_global_search_iters, num_local_search_iters,
                       [&](int q, int n_global, int n_local) {
                           return acquisition_func::FindNextPointsByLogNoisyExpectedImprovement(
                               *m_regressor, q, std::max(1, num_draws), n_global, n_local, seed, 2048, nullptr, tau_relu, tau_max);
                       });
    }

    VectorXd PreferentialBayesianOptimizer::GetMaximizer() const { return m_current_options[0]; }

    double PreferentialBayesianOptimizer::GetPreferenceValueMean(const VectorXd& point) const
    {
        return m_regressor ? m_regressor->PredictMu(point) : 0.0;
    }
    double PreferentialBayesianOptimizer::GetPreferenceValueStdev(const VectorXd& point) const
    {
        return m_regressor ? m_regressor->PredictSigma(point) : 0.0;
    }
    double PreferentialBayesianOptimizer::GetAcquisitionFuncValue(const VectorXd& point) const
    {
        return m_regressor ? acquisition_func::CalcAcquisitionValue(*m_regressor, point, m_acquisition_func_type,
                                                                    m_gaussian_process_upper_confidence_bound_hyperparam)
                           : 0.0;
    }

    Eigen::VectorXd PreferentialBayesianOptimizer::GetPreferenceValueMeans(const Eigen::MatrixXd& points) const
    {
        Eigen::VectorXd mu = Eigen::VectorXd::Zero(points.cols()), sigma;
        if (m_regressor) m_regressor->PredictBatch(points, mu, sigma);
        return mu;
    }
    Eigen::VectorXd PreferentialBayesianOptimizer::GetPreferenceValueStdevs(const Eigen::MatrixXd& points) const
    {
        Eigen::VectorXd mu, sigma = Eigen::VectorXd::Zero(points.cols());
        if (m_regressor) m_regressor->PredictBatch(points, mu, sigma);
        return sigma;
    }
    Eigen::MatrixXd PreferentialBayesianOptimizer::GetPreferenceValueCovariance(const Eigen::MatrixXd& points) const
    {
        if (!m_regressor) return Eigen::MatrixXd::Zero(points.cols(), points.cols());
        return m_regressor->PredictCovariance(points);
    }
    Eigen::MatrixXd PreferentialBayesianOptimizer::SamplePreferenceValues(const Eigen::MatrixXd& points, const int num_samples,
                                                  const unsigned long long seed) const
    {
        if (!m_regressor) return Eigen::MatrixXd::Zero(points.cols(), num_samples);
        return m_regressor->SamplePosterior(points, num_samples, seed);
    }
    Eigen::VectorXd PreferentialBayesianOptimizer::GetAcquisitionFuncValues(const Eigen::MatrixXd& points) const
    {
        if (!m_regressor) return Eigen::VectorXd::Zero(points.cols());
        return acquisition_func::CalcAcquisitionValues(*m_regressor, points, m_acquisition_func_type,
                                                       m_gaussian_process_upper_confidence_bound_hyperparam);
    }

    const Eigen::MatrixXd& PreferentialBayesianOptimizer::GetRawDataPoints() const { return m_data->GetX(); }

    void PreferentialBayesianOptimizer::DampData(const std::string& directory_path) const
    {
        if (m_regressor) m_regressor->DampData(directory_path);
    }

    // reference: :184-end (heuristic budget 10 (D + number of points))
    void PreferentialBayesianOptimizer::PerformMapEstimation(const int num_map_estimation_iters)
    {
        const int iters = num_map_estimation_iters > 0
                              ? num_map_estimation_iters
                              : 10 * (static_cast<int>(GetMaximizer().size()) + m_data->GetNumDataPoints());
        m_regressor = std::make_shared<PreferenceRegressor>(m_data->GetX(), m_data->GetD(), m_use_map_hyperparams, m_kernel_signal_var,
                                                            m_kernel_length_scale, m_noise_level, m_kernel_hyperparams_prior_var,
                                                            m_btl_scale, iters, m_kernel_type);
        if (m_use_laplace_posterior) m_regressor->UseLaplacePosterior();
    }
    void PreferentialBayesianOptimizer::SetUseLaplacePosterior(const bool use_laplace_posterior)
    {
        m_use_laplace_posterior = use_laplace_posterior;
        if (m_regressor) m_regressor->UseLaplacePosterior(use_laplace_posterior);
    }
} // namespace sequential_line_search
