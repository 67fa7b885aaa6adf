// Optimizer facade of sequential gallery search: the two-dimensional successor of the slider query [Koyama+ 2020] on the
// machinery of SequentialLineSearchOptimizer (not in the reference).  The user is shown a bilinear patch of designs, spanned by four
// corners, as a grid and picks the best cell; the next patch has the current best point in its corner c00 and maximises the expected
// utility of its best cell (gallery EUBO; include/sls_hip.h sls_patch_*).  Search space: [0,1]^D.
#ifndef SEQUENTIAL_LINE_SEARCH_SEQUENTIAL_GALLERY_SEARCH_HPP
#define SEQUENTIAL_LINE_SEARCH_SEQUENTIAL_GALLERY_SEARCH_HPP

#include <array>
#include <functional>
#include <memory>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/current-best-selection-strategy.hpp>
#include <sequential-line-search/eigen-lite.hpp>
#include <sequential-line-search/kernel-type.hpp>
#include <string>
#include <utility>

namespace sequential_line_search
{
    class PreferenceRegressor;
    class PreferenceDataManager;

    /// The corners c00, c10, c01, c11 of a patch
    using GalleryCorners = std::array<Eigen::VectorXd, 4>;

    /// Four random corners, drawn two by two from the generator of the initial slider (GenerateRandomSliderEnds)
    GalleryCorners GenerateRandomGalleryCorners(const int num_dims);

    class SequentialGallerySearchOptimizer
    {
    public:
        /// The options of SequentialLineSearchOptimizer but its slider enlargement: a patch is shown as it was scored (an enlarged
        /// patch's corners could leave the cube).
        SequentialGallerySearchOptimizer(
            const int num_dims, const bool use_map_hyperparams = true,
            const KernelType          kernel_type           = KernelType::ArdMatern52Kernel,
            const AcquisitionFuncType acquisition_func_type = AcquisitionFuncType::ExpectedImprovement,
            const std::function<GalleryCorners(const int)>& initial_query_generator = GenerateRandomGalleryCorners,
            const CurrentBestSelectionStrategy current_best_selection_strategy = CurrentBestSelectionStrategy::LargestExpectValue);

        /// With MAP enabled the kernel values are prior medians and initial guesses; otherwise they are used directly.
        void SetHyperparams(const double kernel_signal_var = 0.500, const double kernel_length_scale = 0.500,
                            const double noise_level = 0.005, const double kernel_hyperparams_prior_var = 0.250,
                            const double btl_scale = 0.010);

        /// The user's pick at the continuous position (position_s, position_t) in [0,1]^2 of the current gallery ((0,0) = c00,
        /// (1,0) = c10, (0,1) = c01, (1,1) = c11): the chosen point is added as preferred over the four corners, the regressor is
        /// refitted (num_map_estimation_iters), the current best point x+ is taken by the strategy, and the next gallery is the
        /// maximiser of the expected utility of the best cell of a grid_s x grid_t grid anchored at c00 = x+
        /// (acquisition_func::FindNextGalleryByExpectedUtility: num_draws posterior draws of num_frequencies random features, draw
        /// and start stream `seed`).  The same seeds give the same run.
        void SubmitFeedbackData(const double position_s, const double position_t, const int grid_s = 4, const int grid_t = 4,
                                const int num_draws = 256, const int num_map_estimation_iters = 100,
                                const int num_global_search_iters = 100, const int num_local_search_iters = 50,
                                const unsigned long long seed = 0, const int num_frequencies = 2048);

        GalleryCorners  GetGalleryCorners() const { return m_corners; }
        /// (1 - t) ((1 - s) c00 + s c10) + t ((1 - s) c01 + s c11)
        Eigen::VectorXd CalcPointFromGalleryPosition(const double position_s, const double position_t) const;
        /// The cells of a grid_s x grid_t grid (each axis at least 2 positions): D x (grid_s grid_t), cell (i, j) in column i + grid_s j,
        /// by the expansion of include/sls_hip.h -- the points the criterion scores.
        Eigen::MatrixXd GetGalleryPoints(const int grid_s, const int grid_t) const;
        /// The current best point: the corner c00 (of the initial gallery too).
        Eigen::VectorXd GetMaximizer() const { return m_corners[0]; }

        double GetPreferenceValueMean(const Eigen::VectorXd& point) const;
        double GetPreferenceValueStdev(const Eigen::VectorXd& point) const;
        double GetAcquisitionFuncValue(const Eigen::VectorXd& point) const;

        /// Batched forms, one query point per column of `points` (D x M); zeros while there is no data.
        Eigen::VectorXd GetPreferenceValueMeans(const Eigen::MatrixXd& points) const;
        Eigen::VectorXd GetPreferenceValueStdevs(const Eigen::MatrixXd& points) const;
        Eigen::VectorXd GetAcquisitionFuncValues(const Eigen::MatrixXd& points) const;

        const Eigen::MatrixXd& GetRawDataPoints() const;

        void DampData(const std::string& directory_path) const;

        void SetGaussianProcessUpperConfidenceBoundHyperparam(const double hyperparam)
        {
            m_gaussian_process_upper_confidence_bound_hyperparam = hyperparam;
        }

        /// Laplace posterior of the goodness values (PreferenceRegressor::UseLaplacePosterior) for every regressor the
        /// SubmitFeedbackData* calls build from now on, and for the current one.  Off by default: today's behaviour, bit for bit.
        void SetUseLaplacePosterior(const bool use_laplace_posterior);
        bool GetUseLaplacePosterior() const { return m_use_laplace_posterior; }

    private:
        const bool m_use_map_hyperparams;

        const CurrentBestSelectionStrategy m_current_best_selection_strategy;

        std::shared_ptr<PreferenceRegressor>   m_regressor;
        bool                                   m_use_laplace_posterior = false;
        std::shared_ptr<PreferenceDataManager> m_data;
        GalleryCorners                         m_corners;

        double m_kernel_signal_var;
        double m_kernel_length_scale;
        double m_noise_level;
        double m_kernel_hyperparams_prior_var;
        double m_btl_scale;

        const KernelType          m_kernel_type;
        const AcquisitionFuncType m_acquisition_func_type;

        double m_gaussian_process_upper_confidence_bound_hyperparam;
    };
} // namespace sequential_line_search

#endif
