// SequentialGallerySearchOptimizer facade: the gallery loop on the pieces of SequentialLineSearchOptimizer (sequential-line-search.cpp).
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/preference-data-manager.hpp>
#include <sequential-line-search/preference-regressor.hpp>
#include <algorithm>
#include <sequential-line-search/sequential-gallery-search.hpp>
#include <sequential-line-search/sequential-line-search.hpp>
#include <stdexcept>

using Eigen::MatrixXd;
using Eigen::VectorXd;

namespace sequential_line_search
{
    namespace
    {
        // w0 a + w1 b: two products and one sum, as every step of the expansion in include/sls_hip.h
        VectorXd Mix(const double w0, const VectorXd& a, const double w1, const VectorXd& b) { return w0 * a + w1 * b; }

        VectorXd Bilinear(const GalleryCorners& c, const double u, const double s, const double v, const double t)
        {
            return Mix(v, Mix(u, c[0], s, c[1]), t, Mix(u, c[2], s, c[3]));
        }
    } // namespace

    GalleryCorners GenerateRandomGalleryCorners(const int num_dims)
    {
        const auto lower = GenerateRandomSliderEnds(num_dims);
        const auto upper = GenerateRandomSliderEnds(num_dims);
        return {lower.first, lower.second, upper.first, upper.second};
    }

    SequentialGallerySearchOptimizer::SequentialGallerySearchOptimizer(
        const int num_dims, const bool use_map_hyperparams, const KernelType kernel_type, const AcquisitionFuncType acquisition_func_type,
        const std::function<GalleryCorners(const int)>& initial_query_generator,
        const CurrentBestSelectionStrategy              current_best_selection_strategy)
        : m_use_map_hyperparams(use_map_hyperparams),
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
        m_corners = initial_query_generator(num_dims);
        for (const VectorXd& c : m_corners)
            if (c.size() != num_dims)
                throw std::invalid_argument("SequentialGallerySearchOptimizer: the initial query must be four corners of num_dims values");
        m_data      = std::make_shared<PreferenceDataManager>();
        m_regressor = nullptr;
    }

    void SequentialGallerySearchOptimizer::SetHyperparams(const double kernel_signal_var, const double kernel_length_scale,
                                                          const double noise_level, const double kernel_hyperparams_prior_var,
                                                          const double btl_scale)
    {
        m_kernel_signal_var            = kernel_signal_var;
        m_kernel_length_scale          = kernel_length_scale;
        m_noise_level                  = noise_level;
        m_kernel_hyperparams_prior_var = kernel_hyperparams_prior_var;
        m_btl_scale                    = btl_scale;
    }

    void SequentialGallerySearchOptimizer::SubmitFeedbackData(const double position_s, const double position_t, const int grid_s,
                                                              const int grid_t, const int num_draws,
                                                              const int num_map_estimation_iters, const int num_global_search_iters,
                                                              const int num_local_search_iters, const unsigned long long seed,
                                                              const int num_frequencies)
    {
        const VectorXd x_chosen = CalcPointFromGalleryPosition(position_s, position_t);

        m_data->AddNewPoints(x_chosen, {m_corners[0], m_corners[1], m_corners[2], m_corners[3]}, true);

        m_regressor = std::make_shared<PreferenceRegressor>(m_data->GetX(), m_data->GetD(), m_use_map_hyperparams, m_kernel_signal_var,
                                                            m_kernel_length_scale, m_noise_level, m_kernel_hyperparams_prior_var,
                                                            m_btl_scale, num_map_estimation_iters, m_kernel_type);
        if (m_use_laplace_posterior) m_regressor->UseLaplacePosterior();

        const VectorXd x_plus = (m_current_best_selection_strategy == CurrentBestSelectionStrategy::LargestExpectValue)
                                    ? m_regressor->FindArgMax()
                                    : x_chosen;
        const std::vector<VectorXd> corners = acquisition_func::FindNextGalleryByExpectedUtility(
            *m_regressor, x_plus, grid_s, grid_t, static_cast<unsigned>(std::max(1, num_draws)),
            static_cast<unsigned>(std::max(1, num_global_search_iters)), static_cast<unsigned>(std::max(1, num_local_search_iters)), seed,
            num_frequencies);

        m_corners = {x_plus, corners[1], corners[2], corners[3]};
    }

    VectorXd SequentialGallerySearchOptimizer::CalcPointFromGalleryPosition(const double position_s, const double position_t) const
    {
        return Bilinear(m_corners, 1.0 - position_s, position_s, 1.0 - position_t, position_t);
    }

    MatrixXd SequentialGallerySearchOptimizer::GetGalleryPoints(const int grid_s, const int grid_t) const
    {
        if (grid_s < 2 || grid_t < 2) throw std::invalid_argument("SequentialGallerySearchOptimizer::GetGalleryPoints: 2 positions per axis at least");
        MatrixXd points(m_corners[0].size(), static_cast<long>(grid_s) * grid_t);
        for (int j = 0; j < grid_t; ++j)
            for (int i = 0; i < grid_s; ++i)
            {
                const double ds = grid_s - 1, dt = grid_t - 1;
                eig::SetCol(points, i + static_cast<long>(grid_s) * j,
                            Bilinear(m_corners, (grid_s - 1 - i) / ds, i / ds, (grid_t - 1 - j) / dt, j / dt));
            }
        return points;
    }

    double SequentialGallerySearchOptimizer::GetPreferenceValueMean(const VectorXd& point) const
    {
        return m_regressor ? m_regressor->PredictMu(point) : 0.0;
    }
    double SequentialGallerySearchOptimizer::GetPreferenceValueStdev(const VectorXd& point) const
    {
        return m_regressor ? m_regressor->PredictSigma(point) : 0.0;
    }
    double SequentialGallerySearchOptimizer::GetAcquisitionFuncValue(const VectorXd& point) const
    {
        return m_regressor ? acquisition_func::CalcAcquisitionValue(*m_regressor, point, m_acquisition_func_type,
                                                                    m_gaussian_process_upper_confidence_bound_hyperparam)
                           : 0.0;
    }

    VectorXd SequentialGallerySearchOptimizer::GetPreferenceValueMeans(const MatrixXd& points) const
    {
        VectorXd mu = VectorXd::Zero(points.cols()), sigma;
        if (m_regressor) m_regressor->PredictBatch(points, mu, sigma);
        return mu;
    }
    VectorXd SequentialGallerySearchOptimizer::GetPreferenceValueStdevs(const MatrixXd& points) const
    {
        VectorXd mu, sigma = VectorXd::Zero(points.cols());
        if (m_regressor) m_regressor->PredictBatch(points, mu, sigma);
        return sigma;
    }
    VectorXd SequentialGallerySearchOptimizer::GetAcquisitionFuncValues(const MatrixXd& points) const
    {
        if (!m_regressor) return VectorXd::Zero(points.cols());
        return acquisition_func::CalcAcquisitionValues(*m_regressor, points, m_acquisition_func_type,
                                                       m_gaussian_process_upper_confidence_bound_hyperparam);
    }

    const MatrixXd& SequentialGallerySearchOptimizer::GetRawDataPoints() const { return m_data->GetX(); }

    void SequentialGallerySearchOptimizer::DampData(const std::string& directory_path) const
    {
        if (m_regressor) m_regressor->DampData(directory_path);
    }
    void SequentialGallerySearchOptimizer::SetUseLaplacePosterior(const bool use_laplace_posterior)
    {
        m_use_laplace_posterior = use_laplace_posterior;
        if (m_regressor) m_regressor->UseLaplacePosterior(use_laplace_posterior);
    }
} // namespace sequential_line_search
