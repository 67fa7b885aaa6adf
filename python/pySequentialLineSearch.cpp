// pybind11 module `pySequentialLineSearch`: the two optimizer facades + the three enums, with the snake_case method names
// and keyword arguments of the reference's binding (python/pySequentialLineSearch.cpp:13-153), so the reference's
// python-examples recipes run unchanged on the MI355X path.  Vectors / matrices cross the boundary as numpy float64
// arrays (the reference relies on pybind11/eigen.h; Eigen is not available here, hence the small casters below).
// Additions: set_random_seed(), set/get_global_search_strategy(), set/get_devices(), and batched predict_mean_stdev /
// acquisition_values on (D, M) arrays; GaussianProcessRegressor (fixed hyper-parameters) with sample_max_values(),
// calc_max_value_entropies(), find_next_point_by_max_value_entropy_search() and find_next_point_direct().
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/device.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/preference-regressor.hpp>
#include <sequential-line-search/preferential-bayesian-optimizer.hpp>
#include <sequential-line-search/sequential-gallery-search.hpp>
#include <sequential-line-search/sequential-line-search.hpp>
#include <sequential-line-search/utils.hpp>

namespace py = pybind11;
using namespace py::literals;
using namespace sequential_line_search;
using Eigen::MatrixXd;
using Eigen::VectorXd;

#ifndef SLS_HAVE_REAL_EIGEN
namespace pybind11
{
    namespace detail
    {
        template <> struct type_caster<VectorXd>
        {
            PYBIND11_TYPE_CASTER(VectorXd, const_name("numpy.ndarray[float64[n]]"));
            bool load(handle src, bool)
            {
                auto a = array_t<double, array::c_style | array::forcecast>::ensure(src);
                if (!a || a.ndim() != 1) return false;
                value = VectorXd(a.shape(0));
                for (ssize_t i = 0; i < a.shape(0); ++i) value(i) = a.at(i);
                return true;
            }
            static handle cast(const VectorXd& v, return_value_policy, handle)
            {
                array_t<double> a(v.size());
                for (long i = 0; i < v.size(); ++i) a.mutable_at(i) = v(i);
                return a.release();
            }
        };
        template <> struct type_caster<MatrixXd>
        {
            PYBIND11_TYPE_CASTER(MatrixXd, const_name("numpy.ndarray[float64[m, n]]"));
            bool load(handle src, bool)
            {
                auto a = array_t<double, array::forcecast>::ensure(src);
                if (!a || a.ndim() != 2) return false;
                value = MatrixXd(a.shape(0), a.shape(1));
                for (ssize_t i = 0; i < a.shape(0); ++i)
                    for (ssize_t j = 0; j < a.shape(1); ++j) value(i, j) = a.at(i, j);
                return true;
            }
            static handle cast(const MatrixXd& m, return_value_policy, handle)
            {
                array_t<double> a({m.rows(), m.cols()});
                for (long i = 0; i < m.rows(); ++i)
                    for (long j = 0; j < m.cols(); ++j) a.mutable_at(i, j) = m(i, j);
                return a.release();
            }
        };
        template <> struct type_caster<Eigen::MatrixXi>
        {
            PYBIND11_TYPE_CASTER(Eigen::MatrixXi, const_name("numpy.ndarray[int32[m, n]]"));
            bool load(handle src, bool)
            {
                auto a = array_t<int, array::forcecast>::ensure(src);
                if (!a || a.ndim() != 2) return false;
                value = Eigen::MatrixXi(a.shape(0), a.shape(1));
                for (ssize_t i = 0; i < a.shape(0); ++i)
                    for (ssize_t j = 0; j < a.shape(1); ++j) value(i, j) = a.at(i, j);
                return true;
            }
            static handle cast(const Eigen::MatrixXi& m, return_value_policy, handle)
            {
                array_t<int> a({m.rows(), m.cols()});
                for (long i = 0; i < m.rows(); ++i)
                    for (long j = 0; j < m.cols(); ++j) a.mutable_at(i, j) = m(i, j);
                return a.release();
            }
        };
        template <> struct type_caster<Eigen::VectorXi>
        {
            PYBIND11_TYPE_CASTER(Eigen::VectorXi, const_name("numpy.ndarray[int32[n]]"));
            bool load(handle src, bool)
            {
                auto a = array_t<int, array::c_style | array::forcecast>::ensure(src);
                if (!a || a.ndim() != 1) return false;
                value = Eigen::VectorXi(a.shape(0));
                for (ssize_t i = 0; i < a.shape(0); ++i) value(i) = a.at(i);
                return true;
            }
            static handle cast(const Eigen::VectorXi& v, return_value_policy, handle)
            {
                array_t<int> a(v.size());
                for (long i = 0; i < v.size(); ++i) a.mutable_at(i) = v(i);
                return a.release();
            }
        };
    } // namespace detail
} // namespace pybind11
#else
#include <pybind11/eigen.h>
#endif

PYBIND11_MODULE(pySequentialLineSearch, m)
{
    m.doc() = "sequential-line-search on AMD MI355X (libsls_hip)";
    m.def("set_random_seed", &utils::SetRandomSeed, "seed"_a);
    // run-time switches of the MI355X build (the reference chooses the maximiser branch at compile time and has one device)
    py::enum_<GlobalSearchStrategy>(m, "GlobalSearchStrategy")
        .value("DirectThenLbfgs", GlobalSearchStrategy::DirectThenLbfgs)
        .value("ParallelMultiStart", GlobalSearchStrategy::ParallelMultiStart);
    m.def("set_global_search_strategy", &acquisition_func::SetGlobalSearchStrategy, "strategy"_a);
    m.def("get_global_search_strategy", &acquisition_func::GetGlobalSearchStrategy);
    m.def("set_local_search_tolerances", &acquisition_func::SetLocalSearchTolerances, "relative_func_tolerance"_a, "relative_param_tolerance"_a);
    m.def("get_local_search_tolerances", [] {
        double f = 0.0, x = 0.0;
        acquisition_func::GetLocalSearchTolerances(&f, &x);
        return std::make_pair(f, x);
    });
    m.def("set_map_fit_tolerances", &acquisition_func::SetMapFitTolerances, "relative_func_tolerance"_a, "relative_param_tolerance"_a);
    m.def("get_map_fit_tolerances", [] {
        double f = 0.0, x = 0.0;
        acquisition_func::GetMapFitTolerances(&f, &x);
        return std::make_pair(f, x);
    });
    m.def("set_devices", &device::SetDevices, "devices"_a);
    m.def("get_devices", [] { return device::Devices(); });

    py::enum_<CurrentBestSelectionStrategy>(m, "CurrentBestSelectionStrategy", py::arithmetic())
        .value("LargestExpectValue", CurrentBestSelectionStrategy::LargestExpectValue)
        .value("LastSelection", CurrentBestSelectionStrategy::LastSelection);
    py::enum_<AcquisitionFuncType>(m, "AcquisitionFuncType", py::arithmetic())
        .value("ExpectedImprovement", AcquisitionFuncType::ExpectedImprovement)
        .value("GaussianProcessUpperConfidenceBound", AcquisitionFuncType::GaussianProcessUpperConfidenceBound)
        .value("LogExpectedImprovement", AcquisitionFuncType::LogExpectedImprovement);
    py::enum_<KernelType>(m, "KernelType", py::arithmetic())
        .value("ArdSquaredExponentialKernel", KernelType::ArdSquaredExponentialKernel)
        .value("ArdMatern52Kernel", KernelType::ArdMatern52Kernel);

    // max-value entropy search on a regressor with fixed hyper-parameters (acquisition-function.hpp)
    py::enum_<HyperparamCriterion>(m, "HyperparamCriterion", py::arithmetic())
        .value("MarginalLikelihood", HyperparamCriterion::MarginalLikelihood)
        .value("LeaveOneOut", HyperparamCriterion::LeaveOneOut);
    py::class_<Regressor>(m, "Regressor");
    py::class_<GaussianProcessRegressor, Regressor>(m, "GaussianProcessRegressor")
        .def(py::init<const MatrixXd&, const VectorXd&, const VectorXd&, double, const KernelType, bool>(), "X"_a, "y"_a,
             "kernel_hyperparams"_a, "noise_hyperparam"_a, "kernel_type"_a = KernelType::ArdMatern52Kernel,
             "materialize_matrices"_a = false)
        // hyper-parameters estimated from the data: MAP of the log marginal likelihood, or of the leave-one-out pseudo-likelihood
        .def(py::init([](const MatrixXd& X, const VectorXd& y, const KernelType kernel_type, HyperparamCriterion criterion) {
                 const bool prev = GaussianProcessRegressor::s_materialize_matrices.exchange(false);
                 try
                 {
                     auto* gp = new GaussianProcessRegressor(X, y, kernel_type, criterion);
                     GaussianProcessRegressor::s_materialize_matrices.store(prev);
                     return gp;
                 }
                 catch (...)
                 {
                     GaussianProcessRegressor::s_materialize_matrices.store(prev);
                     throw;
                 }
             }),
             "X"_a, "y"_a, "kernel_type"_a = KernelType::ArdMatern52Kernel, "criterion"_a = HyperparamCriterion::MarginalLikelihood)
        .def("kernel_hyperparams", [](const GaussianProcessRegressor& r) { return r.GetKernelHyperparams(); })
        .def("noise_hyperparam", &GaussianProcessRegressor::GetNoiseHyperparam)
        // leave-one-out cross-validation at the object's hyper-parameters: (mean, variance, log density), N each
        .def("leave_one_out", [](const GaussianProcessRegressor& r) {
            VectorXd mu, var, logp;
            r.CalcLeaveOneOutPredictions(mu, var, logp);
            return std::make_tuple(mu, var, logp);
        });
    // preference regressor with fixed or MAP hyper-parameters: the model behind the three optimisers, reachable on its own for the
    // Laplace posterior of its goodness values (preference-regressor.hpp)
    py::class_<PreferenceRegressor, Regressor>(m, "PreferenceRegressor")
        .def(py::init([](const MatrixXd& X, const std::vector<std::vector<unsigned>>& preferences, bool use_map_hyperparams,
                         double default_kernel_signal_var, double default_kernel_length_scale, double default_noise_level,
                         double kernel_hyperparams_prior_var, double btl_scale, unsigned num_map_estimation_iters,
                         KernelType kernel_type) {
                 std::vector<Preference> D;
                 for (const auto& p : preferences) D.emplace_back(p);
                 return new PreferenceRegressor(X, D, use_map_hyperparams, default_kernel_signal_var, default_kernel_length_scale,
                                                default_noise_level, kernel_hyperparams_prior_var, btl_scale, num_map_estimation_iters,
                                                kernel_type);
             }),
             "X"_a, "preferences"_a, "use_map_hyperparams"_a = false, "default_kernel_signal_var"_a = 0.500,
             "default_kernel_length_scale"_a = 0.500, "default_noise_level"_a = 0.005, "kernel_hyperparams_prior_var"_a = 0.250,
             "btl_scale"_a = 0.010, "num_map_estimation_iters"_a = 100, "kernel_type"_a = KernelType::ArdMatern52Kernel)
        .def("goodness_values", [](const PreferenceRegressor& r) { return r.GetSmallY(); })
        .def("kernel_hyperparams", [](const PreferenceRegressor& r) { return r.GetKernelHyperparams(); })
        .def("noise_hyperparam", &PreferenceRegressor::GetNoiseHyperparam)
        // (mean, standard deviation) at the columns of points (D, M)
        .def("predict", [](const PreferenceRegressor& r, const MatrixXd& points) {
            VectorXd mu, sigma;
            r.PredictBatch(points, mu, sigma);
            return std::make_pair(mu, sigma);
        }, "points"_a)
        .def("use_laplace_posterior", &PreferenceRegressor::UseLaplacePosterior, "on"_a = true)
        .def("uses_laplace_posterior", &PreferenceRegressor::UsesLaplacePosterior)
        .def("laplace_log_evidence", &PreferenceRegressor::GetLaplaceLogEvidence)
        .def("goodness_covariance", &PreferenceRegressor::GetGoodnessCovariance);
    m.def("find_next_points", &acquisition_func::FindNextPoints, "regressor"_a, "num_points"_a, "num_global_search_iters"_a = 100,
          "num_local_search_iters"_a = 50, "func_type"_a = AcquisitionFuncType::ExpectedImprovement,
          "gaussian_process_upper_confidence_bound_hyperparam"_a = 1.0);
    m.def("sample_max_values", &acquisition_func::SampleMaxValues, "regressor"_a, "num_samples"_a = 64,
          "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("calc_max_value_entropies",
          [](const Regressor& r, const MatrixXd& Xs, const VectorXd& max_values) {
              return acquisition_func::CalcMaxValueEntropies(r, Xs, max_values);
          },
          "regressor"_a, "points"_a, "max_values"_a);
    m.def("find_next_point_by_max_value_entropy_search",
          [](const Regressor& r, unsigned num_max_value_samples, unsigned num_global_search_iters, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double         value = 0.0;
              const VectorXd x     = acquisition_func::FindNextPointByMaxValueEntropySearch(
                  r, num_max_value_samples, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "num_max_value_samples"_a = 64, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);

    // joint entropy search (acquisition-function.hpp): the sampled optima (locations D x K, values K), alpha on them at the columns
    // of points, and the maximiser with its value
    m.def("sample_optima", &acquisition_func::SampleOptima, "regressor"_a, "num_samples"_a = 64, "num_global_search_iters"_a = 100,
          "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("calc_joint_entropies",
          [](const Regressor& r, const MatrixXd& Xs, const MatrixXd& optima_x, const VectorXd& optima_f, double star_noise) {
              return acquisition_func::CalcJointEntropies(r, Xs, optima_x, optima_f, nullptr, star_noise);
          },
          "regressor"_a, "points"_a, "optima_x"_a, "optima_f"_a, "star_noise"_a = -1.0);
    m.def("find_next_point_by_joint_entropy_search",
          [](const Regressor& r, unsigned num_optima, unsigned num_global_search_iters, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double         value = 0.0;
              const VectorXd x     = acquisition_func::FindNextPointByJointEntropySearch(r, num_optima, num_global_search_iters,
                                                                                     num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "num_optima"_a = 64, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL,
          "num_frequencies"_a = 2048);

    // knowledge gradient on a discrete set (acquisition-function.hpp): values at the columns of points for the reference set
    // ref_points (D x K), the default reference set, and the maximiser on it with its value
    m.def("calc_knowledge_gradients",
          [](const Regressor& r, const MatrixXd& Xs, const MatrixXd& ref_points, bool include_candidate) {
              return acquisition_func::CalcKnowledgeGradients(r, Xs, ref_points, nullptr, include_candidate);
          },
          "regressor"_a, "points"_a, "ref_points"_a, "include_candidate"_a = true);
    m.def("knowledge_gradient_reference_points", &acquisition_func::KnowledgeGradientReferencePoints, "regressor"_a);
    m.def("find_next_point_by_knowledge_gradient",
          [](const Regressor& r, unsigned num_global_search_iters, unsigned num_local_search_iters, unsigned long long seed) {
              double         value = 0.0;
              const VectorXd x =
                  acquisition_func::FindNextPointByKnowledgeGradient(r, num_global_search_iters, num_local_search_iters, seed, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL);

    // expected utility of the best option of a query pair (acquisition-function.hpp): values for the pairs (points_a.col(m),
    // points_b.col(m)), and the maximising pair with its value: (x, x', value)
    m.def("calc_expected_utilities_of_best_option",
          [](const Regressor& r, const MatrixXd& Xa, const MatrixXd& Xb) {
              return acquisition_func::CalcExpectedUtilitiesOfBestOption(r, Xa, Xb);
          },
          "regressor"_a, "points_a"_a, "points_b"_a);
    m.def("find_next_query_pair_by_expected_utility",
          [](const Regressor& r, unsigned num_global_search_iters, unsigned num_local_search_iters, unsigned long long seed) {
              double     value = 0.0;
              const auto q =
                  acquisition_func::FindNextQueryPairByExpectedUtility(r, num_global_search_iters, num_local_search_iters, seed, &value);
              return std::make_tuple(q.first, q.second, value);
          },
          "regressor"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL);

    // expected utility of the best of q options on posterior draws (regressor.hpp, acquisition-function.hpp): the draws as an object
    // -- calc_... returns (values, [gradient per option], win counts q x M), maximize_... (options, value) -- and the whole query
    // with its value: (options, value)
    py::class_<PosteriorFunctionSamples>(m, "PosteriorFunctionSamples")
        .def("get_num_draws", &PosteriorFunctionSamples::GetNumDraws)
        .def("evaluate", &PosteriorFunctionSamples::Evaluate, "points"_a)
        .def("calc_expected_utilities_of_best_option",
             [](const PosteriorFunctionSamples& s, const std::vector<MatrixXd>& options) {
                 std::vector<MatrixXd> grads;
                 Eigen::MatrixXi       wins;
                 const VectorXd        v = s.CalcExpectedUtilitiesOfBestOption(options, &grads, &wins);
                 return std::make_tuple(v, grads, wins);
             },
             "options"_a)
        .def("maximize_expected_utility_of_best_option",
             [](const PosteriorFunctionSamples& s, int num_options, const MatrixXd& starts, unsigned num_local_search_iters) {
                 double     value = 0.0;
                 const auto q     = s.MaximizeExpectedUtilityOfBestOption(num_options, starts, num_local_search_iters, &value);
                 return std::make_pair(q, value);
             },
             "num_options"_a, "starts"_a, "num_local_search_iters"_a = 50)
        // noisy expected improvement on the draws: max_over_points returns (incumbents, argmax), calc_... (values, [gradient per
        // point], win counts q x M), maximize_... (points, value)
        .def("max_over_points",
             [](const PosteriorFunctionSamples& s, const MatrixXd& points) {
                 Eigen::VectorXi arg;
                 const VectorXd  t = s.MaxOverPoints(points, &arg);
                 return std::make_pair(t, arg);
             },
             "points"_a)
        .def("calc_noisy_expected_improvements",
             [](const PosteriorFunctionSamples& s, const std::vector<MatrixXd>& options, const VectorXd& baseline) {
                 std::vector<MatrixXd> grads;
                 Eigen::MatrixXi       wins;
                 const VectorXd        v = s.CalcNoisyExpectedImprovements(options, baseline, &grads, &wins);
                 return std::make_tuple(v, grads, wins);
             },
             "options"_a, "baseline"_a)
        .def("maximize_noisy_expected_improvement",
             [](const PosteriorFunctionSamples& s, int num_points, const VectorXd& baseline, const MatrixXd& starts,
                unsigned num_local_search_iters) {
                 double     value = 0.0;
                 const auto q     = s.MaximizeNoisyExpectedImprovement(num_points, baseline, starts, num_local_search_iters, &value);
                 return std::make_pair(q, value);
             },
             "num_points"_a, "baseline"_a, "starts"_a, "num_local_search_iters"_a = 50)
        // the log form of the two above (temperatures trailing)
        .def("calc_log_noisy_expected_improvements",
             [](const PosteriorFunctionSamples& s, const std::vector<MatrixXd>& options, const VectorXd& baseline, double tau_relu,
                double tau_max) {
                 std::vector<MatrixXd> grads;
                 Eigen::MatrixXi       wins;
                 const VectorXd        v = s.CalcLogNoisyExpectedImprovements(options, baseline, &grads, &wins, tau_relu, tau_max);
                 return std::make_tuple(v, grads, wins);
             },
             "options"_a, "baseline"_a, "tau_relu"_a = 1e-6, "tau_max"_a = 1e-2)
        .def("maximize_log_noisy_expected_improvement",
             [](const PosteriorFunctionSamples& s, int num_points, const VectorXd& baseline, const MatrixXd& starts,
                unsigned num_local_search_iters, double tau_relu, double tau_max) {
                 double     value = 0.0;
                 const auto q =
                     s.MaximizeLogNoisyExpectedImprovement(num_points, baseline, starts, num_local_search_iters, &value, tau_relu, tau_max);
                 return std::make_pair(q, value);
             },
             "num_points"_a, "baseline"_a, "starts"_a, "num_local_search_iters"_a = 50, "tau_relu"_a = 1e-6, "tau_max"_a = 1e-2)
        // the information gain of a choice query under the BTL likelihood: calc_... (values, [gradient per option], predicted choice
        // probabilities q x M, win counts q x M), maximize_... (options, value)
        .def("calc_choice_information_gains",
             [](const PosteriorFunctionSamples& s, const std::vector<MatrixXd>& options, double scale) {
                 std::vector<MatrixXd> grads;
                 MatrixXd              prob;
                 Eigen::MatrixXi       wins;
                 const VectorXd        v = s.CalcChoiceInformationGains(options, scale, &grads, &prob, &wins);
                 return std::make_tuple(v, grads, prob, wins);
             },
             "options"_a, "scale"_a = 0.010)
        .def("maximize_choice_information_gain",
             [](const PosteriorFunctionSamples& s, int num_options, const MatrixXd& starts, unsigned num_local_search_iters, double scale) {
                 double     value = 0.0;
                 const auto q     = s.MaximizeChoiceInformationGain(num_options, scale, starts, num_local_search_iters, &value);
                 return std::make_pair(q, value);
             },
             "num_options"_a, "starts"_a, "num_local_search_iters"_a = 50, "scale"_a = 0.010)
        // the expected utility of the best slider position on the draws: (values, gradient for the first end, for the second, win
        // counts num_positions x M); maximize_... ((end_0, end_1), value)
        .def("calc_expected_utilities_of_best_slider_position",
             [](const PosteriorFunctionSamples& s, const MatrixXd& ends_a, const MatrixXd& ends_b, int num_positions) {
                 MatrixXd        ga, gb;
                 Eigen::MatrixXi wins;
                 const VectorXd  v = s.CalcExpectedUtilitiesOfBestSliderPosition(ends_a, ends_b, num_positions, &ga, &gb, &wins);
                 return std::make_tuple(v, ga, gb, wins);
             },
             "ends_a"_a, "ends_b"_a, "num_positions"_a = 9)
        .def("maximize_expected_utility_of_best_slider_position",
             [](const PosteriorFunctionSamples& s, int num_positions, const MatrixXd& starts, unsigned num_local_search_iters,
                const VectorXd& anchor) {
                 double     value = 0.0;
                 const auto ends  = s.MaximizeExpectedUtilityOfBestSliderPosition(num_positions, starts, num_local_search_iters,
                                                                                 anchor.size() != 0 ? &anchor : nullptr, nullptr, &value);
                 return std::make_pair(ends, value);
             },
             "num_positions"_a, "starts"_a, "num_local_search_iters"_a = 50, "anchor"_a = VectorXd())
        // the expected utility of the best gallery cell on the draws: (values, gradients for c00, c10, c01, c11, win counts (grid_s
        // grid_t) x M); maximize_... ((c00, c10, c01, c11), value)
        .def("calc_expected_utilities_of_best_gallery_cell",
             [](const PosteriorFunctionSamples& s, const MatrixXd& c00, const MatrixXd& c10, const MatrixXd& c01, const MatrixXd& c11,
                int grid_s, int grid_t) {
                 std::vector<MatrixXd> grads;
                 Eigen::MatrixXi       wins;
                 const VectorXd        v = s.CalcExpectedUtilitiesOfBestGalleryCell(c00, c10, c01, c11, grid_s, grid_t, &grads, &wins);
                 return std::make_tuple(v, grads, wins);
             },
             "corners00"_a, "corners10"_a, "corners01"_a, "corners11"_a, "grid_s"_a = 4, "grid_t"_a = 4)
        .def("maximize_expected_utility_of_best_gallery_cell",
             [](const PosteriorFunctionSamples& s, int grid_s, int grid_t, const MatrixXd& starts, unsigned num_local_search_iters,
                const VectorXd& anchor) {
                 double     value   = 0.0;
                 const auto corners = s.MaximizeExpectedUtilityOfBestGalleryCell(grid_s, grid_t, starts, num_local_search_iters,
                                                                                 anchor.size() != 0 ? &anchor : nullptr, nullptr, &value);
                 return std::make_pair(corners, value);
             },
             "grid_s"_a, "grid_t"_a, "starts"_a, "num_local_search_iters"_a = 50, "anchor"_a = VectorXd());
    m.def("sample_posterior_functions",
          [](const Regressor& r, int num_draws, unsigned long long seed, int num_frequencies) {
              return r.SamplePosteriorFunctions(num_draws, seed, num_frequencies);
          },
          "regressor"_a, "num_draws"_a, "seed"_a = 0ULL, "num_frequencies"_a = 2048, py::keep_alive<0, 1>());
    m.def("find_next_query_by_expected_utility",
          [](const Regressor& r, int num_options, unsigned num_draws, unsigned num_global_search_iters, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextQueryByExpectedUtility(r, num_options, num_draws, num_global_search_iters,
                                                                              num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_options"_a, "num_draws"_a = 256, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_query_by_expected_utility_from_starts",
          [](const Regressor& r, int num_options, const MatrixXd& starts, unsigned num_draws, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextQueryByExpectedUtilityFromStarts(r, num_options, starts, num_draws,
                                                                                        num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_options"_a, "starts"_a, "num_draws"_a = 256, "num_local_search_iters"_a = 50, "seed"_a = 0ULL,
          "num_frequencies"_a = 2048);

    // a whole query by the information the answer is expected to give (acquisition-function.hpp): (options, value)
    m.def("find_next_query_by_information_gain",
          [](const Regressor& r, int num_options, double btl_scale, unsigned num_draws, unsigned num_global_search_iters,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextQueryByInformationGain(
                  r, num_options, btl_scale, num_draws, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_options"_a, "btl_scale"_a = 0.010, "num_draws"_a = 256, "num_global_search_iters"_a = 100,
          "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_query_by_information_gain_from_starts",
          [](const Regressor& r, int num_options, const MatrixXd& starts, double btl_scale, unsigned num_draws,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextQueryByInformationGainFromStarts(
                  r, num_options, btl_scale, starts, num_draws, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_options"_a, "starts"_a, "btl_scale"_a = 0.010, "num_draws"_a = 256,
          "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);

    // a batch of points chosen jointly by noisy expected improvement on posterior draws (acquisition-function.hpp): (points, value)
    m.def("find_next_points_by_noisy_expected_improvement",
          [](const Regressor& r, int num_points, unsigned num_draws, unsigned num_global_search_iters, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextPointsByNoisyExpectedImprovement(
                  r, num_points, num_draws, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_points"_a, "num_draws"_a = 256, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_points_by_noisy_expected_improvement_from_starts",
          [](const Regressor& r, int num_points, const MatrixXd& starts, unsigned num_draws, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextPointsByNoisyExpectedImprovementFromStarts(
                  r, num_points, starts, num_draws, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_points"_a, "starts"_a, "num_draws"_a = 256, "num_local_search_iters"_a = 50, "seed"_a = 0ULL,
          "num_frequencies"_a = 2048);
    m.def("find_next_points_by_log_noisy_expected_improvement",
          [](const Regressor& r, int num_points, unsigned num_draws, unsigned num_global_search_iters, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies, double tau_relu, double tau_max) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextPointsByLogNoisyExpectedImprovement(
                  r, num_points, num_draws, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value, tau_relu, tau_max);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_points"_a, "num_draws"_a = 256, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048, "tau_relu"_a = 1e-6, "tau_max"_a = 1e-2);
    m.def("find_next_points_by_log_noisy_expected_improvement_from_starts",
          [](const Regressor& r, int num_points, const MatrixXd& starts, unsigned num_draws, unsigned num_local_search_iters,
             unsigned long long seed, int num_frequencies, double tau_relu, double tau_max) {
              double     value = 0.0;
              const auto q     = acquisition_func::FindNextPointsByLogNoisyExpectedImprovementFromStarts(
                  r, num_points, starts, num_draws, num_local_search_iters, seed, num_frequencies, &value, tau_relu, tau_max);
              return std::make_pair(q, value);
          },
          "regressor"_a, "num_points"_a, "starts"_a, "num_draws"_a = 256, "num_local_search_iters"_a = 50, "seed"_a = 0ULL,
          "num_frequencies"_a = 2048, "tau_relu"_a = 1e-6, "tau_max"_a = 1e-2);

    // the starts of the seeded searches (acquisition-function.hpp): num_dims x count
    m.def("seeded_uniform_starts", &acquisition_func::SeededUniformStarts, "num_dims"_a, "count"_a, "seed"_a = 0ULL);
    // search restricted to a box / an affine subspace x = offset + basis z, z in [0,1]^d (acquisition-function.hpp): (x, value)
    m.def("find_next_point_in_box",
          [](const Regressor& r, const VectorXd& lower, const VectorXd& upper, unsigned num_global_search_iters,
             unsigned num_local_search_iters, AcquisitionFuncType func_type, double hyperparam, unsigned long long seed) {
              double         value = 0.0;
              const VectorXd x     = acquisition_func::FindNextPointInBox(r, lower, upper, num_global_search_iters, num_local_search_iters,
                                                                      func_type, hyperparam, seed, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "lower"_a, "upper"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "func_type"_a = AcquisitionFuncType::ExpectedImprovement, "gaussian_process_upper_confidence_bound_hyperparam"_a = 1.0,
          "seed"_a = 0ULL);
    m.def("find_next_point_in_subspace",
          [](const Regressor& r, const VectorXd& offset, const MatrixXd& basis, unsigned num_global_search_iters,
             unsigned num_local_search_iters, AcquisitionFuncType func_type, double hyperparam, unsigned long long seed) {
              SearchSubspace s;
              s.offset             = offset;
              s.basis              = basis;
              double         value = 0.0;
              const VectorXd x     = acquisition_func::FindNextPointInSubspace(r, s, num_global_search_iters, num_local_search_iters,
                                                                           func_type, hyperparam, seed, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "offset"_a, "basis"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "func_type"_a = AcquisitionFuncType::ExpectedImprovement, "gaussian_process_upper_confidence_bound_hyperparam"_a = 1.0,
          "seed"_a = 0ULL);
    m.def("find_next_points_by_thompson_sampling_in_box", &acquisition_func::FindNextPointsByThompsonSamplingInBox, "regressor"_a,
          "num_points"_a, "lower"_a, "upper"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL,
          "num_frequencies"_a = 2048);

    // the next slider by the expected utility of its best position (acquisition-function.hpp): ((end_0, end_1), value); an empty anchor
    // leaves both ends free
    m.def("find_next_slider_by_expected_utility",
          [](const Regressor& r, const VectorXd& anchor, int num_positions, unsigned num_draws, unsigned num_global_search_iters,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto ends  = acquisition_func::FindNextSliderByExpectedUtility(
                  r, anchor, num_positions, num_draws, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(ends, value);
          },
          "regressor"_a, "anchor"_a = VectorXd(), "num_positions"_a = 9, "num_draws"_a = 256, "num_global_search_iters"_a = 100,
          "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_slider_by_expected_utility_from_starts",
          [](const Regressor& r, const VectorXd& anchor, const MatrixXd& starts, int num_positions, unsigned num_draws,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value = 0.0;
              const auto ends  = acquisition_func::FindNextSliderByExpectedUtilityFromStarts(
                  r, anchor, starts, num_positions, num_draws, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(ends, value);
          },
          "regressor"_a, "anchor"_a, "starts"_a, "num_positions"_a = 9, "num_draws"_a = 256, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);

    // the gallery counterparts (acquisition-function.hpp).  calc_...: (values, gradients for c00, c10, c01, c11, win counts) on
    // num_draws draws of the regressor (stream `seed`); find_...: ((c00, c10, c01, c11), value), an empty anchor leaves all four free
    m.def("calc_expected_utilities_of_best_gallery_cell",
          [](const Regressor& r, const MatrixXd& c00, const MatrixXd& c10, const MatrixXd& c01, const MatrixXd& c11, int grid_s,
             int grid_t, int num_draws, unsigned long long seed, int num_frequencies) {
              const PosteriorFunctionSamples draws = r.SamplePosteriorFunctions(num_draws, seed, num_frequencies);
              std::vector<MatrixXd>          grads;
              Eigen::MatrixXi                wins;
              const VectorXd v = draws.CalcExpectedUtilitiesOfBestGalleryCell(c00, c10, c01, c11, grid_s, grid_t, &grads, &wins);
              return std::make_tuple(v, grads, wins);
          },
          "regressor"_a, "corners00"_a, "corners10"_a, "corners01"_a, "corners11"_a, "grid_s"_a = 4, "grid_t"_a = 4, "num_draws"_a = 256,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_gallery_by_expected_utility",
          [](const Regressor& r, const VectorXd& anchor, int grid_s, int grid_t, unsigned num_draws, unsigned num_global_search_iters,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value   = 0.0;
              const auto corners = acquisition_func::FindNextGalleryByExpectedUtility(
                  r, anchor, grid_s, grid_t, num_draws, num_global_search_iters, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(corners, value);
          },
          "regressor"_a, "anchor"_a = VectorXd(), "grid_s"_a = 4, "grid_t"_a = 4, "num_draws"_a = 256,
          "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048);
    m.def("find_next_gallery_by_expected_utility_from_starts",
          [](const Regressor& r, const VectorXd& anchor, const MatrixXd& starts, int grid_s, int grid_t, unsigned num_draws,
             unsigned num_local_search_iters, unsigned long long seed, int num_frequencies) {
              double     value   = 0.0;
              const auto corners = acquisition_func::FindNextGalleryByExpectedUtilityFromStarts(
                  r, anchor, starts, grid_s, grid_t, num_draws, num_local_search_iters, seed, num_frequencies, &value);
              return std::make_pair(corners, value);
          },
          "regressor"_a, "anchor"_a, "starts"_a, "grid_s"_a = 4, "grid_t"_a = 4, "num_draws"_a = 256, "num_local_search_iters"_a = 50,
          "seed"_a = 0ULL, "num_frequencies"_a = 2048);

    // DIRECT, then one L-BFGS from its result (acquisition_func::FindNextPointDirect) on such a regressor: (point, value)
    m.def("find_next_point_direct",
          [](const Regressor& r, unsigned num_global_search_iters, unsigned num_local_search_iters, AcquisitionFuncType func_type,
             double hyperparam) {
              double         value = 0.0;
              const VectorXd x =
                  acquisition_func::FindNextPointDirect(r, num_global_search_iters, num_local_search_iters, func_type, hyperparam, &value);
              return std::make_pair(x, value);
          },
          "regressor"_a, "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50,
          "acquisition_func_type"_a = AcquisitionFuncType::ExpectedImprovement,
          "gaussian_process_upper_confidence_bound_hyperparam"_a = 1.0);

    using SliderEndsGenerator = std::function<std::pair<VectorXd, VectorXd>(const int)>;
    m.def("generate_random_slider_ends", &GenerateRandomSliderEnds, "num_dims"_a);
    m.def("generate_centered_fixed_length_random_slider_ends", &GenerateCenteredFixedLengthRandomSliderEnds, "num_dims"_a);

    py::class_<SequentialLineSearchOptimizer>(m, "SequentialLineSearchOptimizer")
        .def(py::init<const int, const bool, const bool, const KernelType, const AcquisitionFuncType, const SliderEndsGenerator&,
                      const CurrentBestSelectionStrategy>(),
             "num_dims"_a, "use_slider_enlargement"_a = true, "use_map_hyperparams"_a = true,
             "kernel_type"_a = KernelType::ArdMatern52Kernel, "acquisition_func_type"_a = AcquisitionFuncType::ExpectedImprovement,
             "initial_query_generator"_a         = SliderEndsGenerator(GenerateRandomSliderEnds),
             "current_best_selection_strategy"_a = CurrentBestSelectionStrategy::LargestExpectValue)
        .def("set_hyperparams", &SequentialLineSearchOptimizer::SetHyperparams, "kernel_signal_var"_a = 0.500,
             "kernel_length_scale"_a = 0.500, "noise_level"_a = 0.005, "kernel_hyperparams_prior_var"_a = 0.250, "btl_scale"_a = 0.010)
        .def("submit_feedback_data", static_cast<void (SequentialLineSearchOptimizer::*)(const double)>(&SequentialLineSearchOptimizer::SubmitFeedbackData),
             "slider_position"_a)
        .def("submit_feedback_data",
             static_cast<void (SequentialLineSearchOptimizer::*)(const double, const int, const int, const int)>(
                 &SequentialLineSearchOptimizer::SubmitFeedbackData),
             "slider_position"_a, "num_map_estimation_iters"_a, "num_global_search_iters"_a, "num_local_search_iters"_a)
        .def("submit_feedback_data_by_expected_utility", &SequentialLineSearchOptimizer::SubmitFeedbackDataByExpectedUtility,
             "slider_position"_a, "num_positions"_a = 9, "num_draws"_a = 256, "num_map_estimation_iters"_a = 100,
             "num_global_search_iters"_a = 100, "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048)
        .def("get_slider_ends", &SequentialLineSearchOptimizer::GetSliderEnds)
        .def("calc_point_from_slider_position", &SequentialLineSearchOptimizer::CalcPointFromSliderPosition, "slider_position"_a)
        .def("get_maximizer", &SequentialLineSearchOptimizer::GetMaximizer)
        .def("get_preference_value_mean", &SequentialLineSearchOptimizer::GetPreferenceValueMean, "point"_a)
        .def("get_preference_value_stdev", &SequentialLineSearchOptimizer::GetPreferenceValueStdev, "point"_a)
        .def("get_acquisition_func_value", &SequentialLineSearchOptimizer::GetAcquisitionFuncValue, "point"_a)
        .def("get_preference_value_means", &SequentialLineSearchOptimizer::GetPreferenceValueMeans, "points"_a)
        .def("get_preference_value_stdevs", &SequentialLineSearchOptimizer::GetPreferenceValueStdevs, "points"_a)
        .def("get_preference_value_covariance", &SequentialLineSearchOptimizer::GetPreferenceValueCovariance, "points"_a)
        .def("sample_preference_values", &SequentialLineSearchOptimizer::SamplePreferenceValues, "points"_a, "num_samples"_a, "seed"_a)
        .def("get_acquisition_func_values", &SequentialLineSearchOptimizer::GetAcquisitionFuncValues, "points"_a)
        .def("get_raw_data_points", &SequentialLineSearchOptimizer::GetRawDataPoints)
        .def("damp_data", &SequentialLineSearchOptimizer::DampData, "directory_path"_a)
        .def("set_use_laplace_posterior", &SequentialLineSearchOptimizer::SetUseLaplacePosterior, "use_laplace_posterior"_a)
        .def("get_use_laplace_posterior", &SequentialLineSearchOptimizer::GetUseLaplacePosterior)
        .def("set_gaussian_process_upper_confidence_bound_hyperparam",
             &SequentialLineSearchOptimizer::SetGaussianProcessUpperConfidenceBoundHyperparam, "hyperparam"_a);

    using GalleryCornersGenerator = std::function<GalleryCorners(const int)>;
    m.def("generate_random_gallery_corners", &GenerateRandomGalleryCorners, "num_dims"_a);

    py::class_<SequentialGallerySearchOptimizer>(m, "SequentialGallerySearchOptimizer")
        .def(py::init<const int, const bool, const KernelType, const AcquisitionFuncType, const GalleryCornersGenerator&,
                      const CurrentBestSelectionStrategy>(),
             "num_dims"_a, "use_map_hyperparams"_a = true, "kernel_type"_a = KernelType::ArdMatern52Kernel,
             "acquisition_func_type"_a           = AcquisitionFuncType::ExpectedImprovement,
             "initial_query_generator"_a         = GalleryCornersGenerator(GenerateRandomGalleryCorners),
             "current_best_selection_strategy"_a = CurrentBestSelectionStrategy::LargestExpectValue)
        .def("set_hyperparams", &SequentialGallerySearchOptimizer::SetHyperparams, "kernel_signal_var"_a = 0.500,
             "kernel_length_scale"_a = 0.500, "noise_level"_a = 0.005, "kernel_hyperparams_prior_var"_a = 0.250, "btl_scale"_a = 0.010)
        .def("submit_feedback_data", &SequentialGallerySearchOptimizer::SubmitFeedbackData, "position_s"_a, "position_t"_a,
             "grid_s"_a = 4, "grid_t"_a = 4, "num_draws"_a = 256, "num_map_estimation_iters"_a = 100, "num_global_search_iters"_a = 100,
             "num_local_search_iters"_a = 50, "seed"_a = 0ULL, "num_frequencies"_a = 2048)
        .def("get_gallery_corners", &SequentialGallerySearchOptimizer::GetGalleryCorners)
        .def("calc_point_from_gallery_position", &SequentialGallerySearchOptimizer::CalcPointFromGalleryPosition, "position_s"_a,
             "position_t"_a)
        .def("get_gallery_points", &SequentialGallerySearchOptimizer::GetGalleryPoints, "grid_s"_a = 4, "grid_t"_a = 4)
        .def("get_maximizer", &SequentialGallerySearchOptimizer::GetMaximizer)
        .def("get_preference_value_mean", &SequentialGallerySearchOptimizer::GetPreferenceValueMean, "point"_a)
        .def("get_preference_value_stdev", &SequentialGallerySearchOptimizer::GetPreferenceValueStdev, "point"_a)
        .def("get_acquisition_func_value", &SequentialGallerySearchOptimizer::GetAcquisitionFuncValue, "point"_a)
        .def("get_preference_value_means", &SequentialGallerySearchOptimizer::GetPreferenceValueMeans, "points"_a)
        .def("get_preference_value_stdevs", &SequentialGallerySearchOptimizer::GetPreferenceValueStdevs, "points"_a)
        .def("get_acquisition_func_values", &SequentialGallerySearchOptimizer::GetAcquisitionFuncValues, "points"_a)
        .def("get_raw_data_points", &SequentialGallerySearchOptimizer::GetRawDataPoints)
        .def("damp_data", &SequentialGallerySearchOptimizer::DampData, "directory_path"_a)
        .def("set_use_laplace_posterior", &SequentialGallerySearchOptimizer::SetUseLaplacePosterior, "use_laplace_posterior"_a)
        .def("get_use_laplace_posterior", &SequentialGallerySearchOptimizer::GetUseLaplacePosterior)
        .def("set_gaussian_process_upper_confidence_bound_hyperparam",
             &SequentialGallerySearchOptimizer::SetGaussianProcessUpperConfidenceBoundHyperparam, "hyperparam"_a);

    py::class_<PreferentialBayesianOptimizer>(m, "PreferentialBayesianOptimizer")
        .def(py::init<const int, const bool, const KernelType, const AcquisitionFuncType, const InitialQueryGenerator&,
                      const CurrentBestSelectionStrategy, const int>(),
             "num_dims"_a, "use_map_hyperparams"_a = true, "kernel_type"_a = KernelType::ArdMatern52Kernel,
             "acquisition_func_type"_a = AcquisitionFuncType::ExpectedImprovement,
             "initial_query_generator"_a         = InitialQueryGenerator(GenerateRandomPoints),
             "current_best_selection_strategy"_a = CurrentBestSelectionStrategy::LargestExpectValue, "num_options"_a = 2)
        .def("set_hyperparams", &PreferentialBayesianOptimizer::SetHyperparams, "kernel_signal_var"_a = 0.500,
             "kernel_length_scale"_a = 0.500, "noise_level"_a = 0.005, "kernel_hyperparams_prior_var"_a = 0.250, "btl_scale"_a = 0.010)
        .def("submit_feedback_data", &PreferentialBayesianOptimizer::SubmitFeedbackData, "option_index"_a, "num_map_estimation_iters"_a = 0)
        .def("submit_custom_feedback_data", &PreferentialBayesianOptimizer::SubmitCustomFeedbackData, "chosen_option"_a,
             "other_options"_a, "num_map_estimation_iters"_a = 0)
        .def("determine_next_query", &PreferentialBayesianOptimizer::DetermineNextQuery, "num_global_search_iters"_a = 0,
             "num_local_search_iters"_a = 0)
        .def("determine_next_query_by_thompson_sampling", &PreferentialBayesianOptimizer::DetermineNextQueryByThompsonSampling,
             "seed"_a, "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0)
        .def("determine_next_query_by_expected_utility", &PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtility,
             "seed"_a, "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0)
        .def("determine_next_query_by_expected_utility_of_draws", &PreferentialBayesianOptimizer::DetermineNextQueryByExpectedUtilityOfDraws,
             "seed"_a, "num_draws"_a = 256, "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0)
        .def("determine_next_query_by_information_gain", &PreferentialBayesianOptimizer::DetermineNextQueryByInformationGain, "seed"_a,
             "num_draws"_a = 256, "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0, "btl_scale"_a = 0.0)
        .def("determine_next_query_by_noisy_expected_improvement",
             &PreferentialBayesianOptimizer::DetermineNextQueryByNoisyExpectedImprovement, "seed"_a, "num_draws"_a = 256,
             "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0)
        .def("determine_next_query_by_log_noisy_expected_improvement",
             &PreferentialBayesianOptimizer::DetermineNextQueryByLogNoisyExpectedImprovement, "seed"_a, "num_draws"_a = 256,
             "num_global_search_iters"_a = 0, "num_local_search_iters"_a = 0, "tau_relu"_a = 1e-6, "tau_max"_a = 1e-2)
        .def("get_current_options", &PreferentialBayesianOptimizer::GetCurrentOptions)
        .def("get_maximizer", &PreferentialBayesianOptimizer::GetMaximizer)
        .def("get_preference_value_mean", &PreferentialBayesianOptimizer::GetPreferenceValueMean, "point"_a)
        .def("get_preference_value_stdev", &PreferentialBayesianOptimizer::GetPreferenceValueStdev, "point"_a)
        .def("get_acquisition_func_value", &PreferentialBayesianOptimizer::GetAcquisitionFuncValue, "point"_a)
        .def("get_preference_value_means", &PreferentialBayesianOptimizer::GetPreferenceValueMeans, "points"_a)
        .def("get_preference_value_stdevs", &PreferentialBayesianOptimizer::GetPreferenceValueStdevs, "points"_a)
        .def("get_preference_value_covariance", &PreferentialBayesianOptimizer::GetPreferenceValueCovariance, "points"_a)
        .def("sample_preference_values", &PreferentialBayesianOptimizer::SamplePreferenceValues, "points"_a, "num_samples"_a, "seed"_a)
        .def("get_acquisition_func_values", &PreferentialBayesianOptimizer::GetAcquisitionFuncValues, "points"_a)
        .def("get_raw_data_points", &PreferentialBayesianOptimizer::GetRawDataPoints)
        .def("damp_data", &PreferentialBayesianOptimizer::DampData, "directory_path"_a)
        .def("set_use_laplace_posterior", &PreferentialBayesianOptimizer::SetUseLaplacePosterior, "use_laplace_posterior"_a)
        .def("get_use_laplace_posterior", &PreferentialBayesianOptimizer::GetUseLaplacePosterior)
        .def("set_gaussian_process_upper_confidence_bound_hyperparam",
             &PreferentialBayesianOptimizer::SetGaussianProcessUpperConfidenceBoundHyperparam, "hyperparam"_a);
}
