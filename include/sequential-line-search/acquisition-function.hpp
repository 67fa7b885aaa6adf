// Acquisition functions and their maximisation
// (reference surface: include/sequential-line-search/acquisition-function.hpp:11-79).
#ifndef SEQUENTIAL_LINE_SEARCH_ACQUISITION_FUNCTION_HPP
#define SEQUENTIAL_LINE_SEARCH_ACQUISITION_FUNCTION_HPP

#include <memory>
#include <sequential-line-search/eigen-lite.hpp>
#include <sequential-line-search/regressor.hpp>
#include <utility>
#include <vector>

namespace sequential_line_search
{
    enum class AcquisitionFuncType
    {
        ExpectedImprovement,
        GaussianProcessUpperConfidenceBound,
        /// log of ExpectedImprovement, formed in log space (not in the reference; include/sls_hip.h "log expected improvement"): it
        /// neither underflows nor loses its gradient far below the incumbent.  The hyperparameter is ignored.  Device-resident
        /// regressors only: for any other Regressor every function below throws std::invalid_argument.
        LogExpectedImprovement,
    };

    /// How FindNextPoint / FindNextPoints search [0,1]^D (reference: the two branches of FindGlobalSolution,
    /// src/acquisition-function.cpp:112-167, chosen there at COMPILE time by the CMake option
    /// SEQUENTIAL_LINE_SEARCH_USE_PARALLELIZED_MULTI_START_SEARCH, default OFF):
    ///   DirectThenLbfgs      DIRECT with num_global_search_iters evaluations, then one L-BFGS of num_local_search_iters
    ///                        evaluations from its result (:155-165, the reference's default build);
    ///   ParallelMultiStart   num_global_search_iters random starts, one L-BFGS each, best end point (:121-153).
    /// Here the choice is a run-time setting.  Its initial value is ParallelMultiStart if this library was compiled with
    /// -DSEQUENTIAL_LINE_SEARCH_USE_PARALLELIZED_MULTI_START_SEARCH, else DirectThenLbfgs; the environment variable
    /// SLS_GLOBAL_SEARCH=direct|multistart overrides that, SetGlobalSearchStrategy overrides both.
    enum class GlobalSearchStrategy
    {
        DirectThenLbfgs,
        ParallelMultiStart,
    };

    /// The affine image x = offset + basis z of the box z in [0,1]^d, 1 <= d <= D, that a search is restricted to (not in the
    /// reference; include/sls_hip.h "maximisation over affine subspaces"): a trust region, a line or plane, a random embedding.
    /// offset has D entries, basis is D x d.  The constructors only produce maps whose image lies inside [0,1]^D (a coordinate may
    /// touch a face to within rounding); a hand-made one may leave it: the evaluations are defined on all of R^D.
    struct SearchSubspace
    {
        Eigen::VectorXd offset;
        Eigen::MatrixXd basis;

        /// The box [lower, upper] (a trust region): offset = lower, basis = diag(upper - lower).  Throws std::invalid_argument
        /// unless 0 <= lower <= upper <= 1 in every coordinate.
        static SearchSubspace Box(const Eigen::VectorXd& lower, const Eigen::VectorXd& upper);
        /// The segment from a (z = 0) to b (z = 1), d = 1: a slider.  Throws unless both ends lie in [0,1]^D.
        static SearchSubspace Segment(const Eigen::VectorXd& a, const Eigen::VectorXd& b);
        /// The image of [0,1]^d under `directions` (D x d), centred at `center` (in [0,1]^D): every row of `directions` that would
        /// carry the image across a face is scaled down so that it just reaches it (0.5 sum_j |B_rj| <= min(center_r, 1 - center_r)).
        static SearchSubspace Centered(const Eigen::VectorXd& center, const Eigen::MatrixXd& directions);
        /// offset + basis z, in the device's arithmetic (from offset, one product and one sum per column of the basis).
        Eigen::VectorXd Point(const Eigen::VectorXd& z) const;
    };

    namespace acquisition_func
    {
        void                 SetGlobalSearchStrategy(GlobalSearchStrategy strategy);
        GlobalSearchStrategy GetGlobalSearchStrategy();

        /// Relative stopping tolerances of the local (L-BFGS) searches.  Every search of the reference goes through
        /// nloptutil::solve, whose defaults are relative_func_tolerance = relative_param_tolerance = 1e-6 (NLopt's ftol_rel /
        /// xtol_rel): a local search ends with the first accepted step that changes the value, or every
        /// coordinate, by less than that fraction -- long before the evaluation cap on most of C3's acquisition landscapes (the
        /// cap only polishes the 7th to 10th digit).  Initial values 1e-6 / 1e-6; SLS_LOCAL_SEARCH_TOL=<v> sets both (0 = off: run
        /// to the cap, the behaviour before round 5's last revision).  The MAP fits keep running to convergence or their caps
        /// (their optima are this layer's parity anchors; SLS_MAP_FIT_TOL opts in, see host/device.hpp).
        void SetLocalSearchTolerances(double relative_func_tolerance, double relative_param_tolerance);
        void GetLocalSearchTolerances(double* relative_func_tolerance, double* relative_param_tolerance);
        /// The same pair for the two MAP fits (GaussianProcessRegressor::PerformMapEstimation, PreferenceRegressor's).  Initial
        /// values 0 / 0 (off) -- a DEVIATION from the reference, whose fits run under nloptutil::solve's 1e-6 defaults like every
        /// other search: pass (1e-6, 1e-6) for the reference's evaluation counts (INTEGRATION.md 2 says why off is the default).
        void SetMapFitTolerances(double relative_func_tolerance, double relative_param_tolerance);
        void GetMapFitTolerances(double* relative_func_tolerance, double* relative_param_tolerance);

        /// Acquisition value at x (0 if the regressor holds no data).  `..._hyperparam` is the GP-UCB trade-off weight
        /// (ignored for EI).
        double CalcAcquisitionValue(const Regressor& regressor, const Eigen::VectorXd& x, const AcquisitionFuncType func_type,
                                    const double gaussian_process_upper_confidence_bound_hyperparam = 1.0);

        Eigen::VectorXd CalcAcquisitionValueDerivative(const Regressor& regressor, const Eigen::VectorXd& x,
                                                       const AcquisitionFuncType func_type,
                                                       const double gaussian_process_upper_confidence_bound_hyperparam = 1.0);

        /// Batched value (and gradient, D x M, if grad != nullptr) for the columns of Xs: one device pass.
        Eigen::VectorXd CalcAcquisitionValues(const Regressor& regressor, const Eigen::MatrixXd& Xs, const AcquisitionFuncType func_type,
                                              const double gaussian_process_upper_confidence_bound_hyperparam = 1.0,
                                              Eigen::MatrixXd* grad = nullptr);

        /// Maximiser of the acquisition function over [0,1]^D by the current GlobalSearchStrategy.  DirectThenLbfgs: every
        /// DIRECT iteration's sample points are one batched device evaluation.  ParallelMultiStart: all starts advance in
        /// lock step on the GPU (sharded over device::Devices() when several are configured).
        Eigen::VectorXd FindNextPoint(const Regressor& regressor, const unsigned num_global_search_iters = 100,
                                      const unsigned            num_local_search_iters = 50,
                                      const AcquisitionFuncType func_type              = AcquisitionFuncType::ExpectedImprovement,
                                      const double              gaussian_process_upper_confidence_bound_hyperparam = 1.0);

        /// The DirectThenLbfgs branch, whatever the current strategy (deterministic: DIRECT draws no random numbers).
        Eigen::VectorXd FindNextPointDirect(const Regressor& regressor, const unsigned num_global_search_iters,
                                            const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                            const double gaussian_process_upper_confidence_bound_hyperparam, double* value = nullptr);

        /// The ParallelMultiStart branch from an explicit start set (D x S), for reproducible runs and multi-GPU sharding;
        /// returns also the value.
        Eigen::VectorXd FindNextPointFromStarts(const Regressor& regressor, const Eigen::MatrixXd& starts,
                                                const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                const double gaussian_process_upper_confidence_bound_hyperparam, double* value = nullptr);

        /// Sequential batch of `num_points` maximisers [Schonlau+ 1998]: after each point the predictive variance is updated
        /// with the new point, the mean is kept.
        std::vector<Eigen::VectorXd> FindNextPoints(const Regressor& regressor, const unsigned num_points,
                                                    const unsigned            num_global_search_iters = 100,
                                                    const unsigned            num_local_search_iters  = 50,
                                                    const AcquisitionFuncType func_type = AcquisitionFuncType::ExpectedImprovement,
                                                    const double gaussian_process_upper_confidence_bound_hyperparam = 1.0);

        /// Batch by Thompson sampling (not in the reference): num_points pathwise posterior draws of the latent function
        /// (Regressor::SamplePosteriorFunctions, stream `seed`, num_frequencies random features), each maximised over [0,1]^D from
        /// num_global_search_iters uniform random starts with num_local_search_iters L-BFGS evaluations each, all draws in one
        /// lock-step run on the device.  One maximiser per draw; the starts come from a generator seeded with `seed`, so the same
        /// seed gives the same points.
        std::vector<Eigen::VectorXd> FindNextPointsByThompsonSampling(const Regressor& regressor, const unsigned num_points,
                                                                      const unsigned num_global_search_iters = 100,
                                                                      const unsigned num_local_search_iters  = 50,
                                                                      const unsigned long long seed = 0, const int num_frequencies = 2048);
        /// The same from an explicit start set: starts is D x (num_points S), columns [s S, (s + 1) S) start draw s.
        std::vector<Eigen::VectorXd> FindNextPointsByThompsonSamplingFromStarts(const Regressor& regressor, const unsigned num_points,
                                                                                const Eigen::MatrixXd& starts,
                                                                                const unsigned         num_local_search_iters,
                                                                                const unsigned long long seed = 0,
                                                                                const int num_frequencies = 2048);

        /// Max-value entropy search (not in the reference; Wang & Jegelka 2017, include/sls_hip.h sls_mes_*).
        /// A Monte-Carlo sample of the maximum VALUE of the latent function: the maxima of num_samples pathwise posterior draws
        /// (stream `seed`, num_frequencies random features), each maximised from num_global_search_iters uniform starts of the
        /// generator FindNextPointsByThompsonSampling uses, clamped from below at the mean at the best data point (the maximum of a
        /// function is at least its value there).  num_samples <= 4096.
        Eigen::VectorXd SampleMaxValues(const Regressor& regressor, const unsigned num_samples = 64,
                                        const unsigned num_global_search_iters = 100, const unsigned num_local_search_iters = 50,
                                        const unsigned long long seed = 0, const int num_frequencies = 2048);
        /// alpha(x) = mean_k g((y*_k - mu(x)) / sigma(x)) for the columns of Xs on the sample max_values of y* (and its gradient,
        /// D x M, if grad != nullptr): one device pass.
        Eigen::VectorXd CalcMaxValueEntropies(const Regressor& regressor, const Eigen::MatrixXd& Xs, const Eigen::VectorXd& max_values,
                                              Eigen::MatrixXd* grad = nullptr);
        /// Maximiser of alpha over [0,1]^D: SampleMaxValues, then one L-BFGS of num_local_search_iters evaluations (the tolerances
        /// of GetLocalSearchTolerances) from each of num_global_search_iters uniform starts of a generator seeded with `seed`, all
        /// in lock step on the device.  The same seed gives the same point.  value (may be nullptr) receives alpha there.
        Eigen::VectorXd FindNextPointByMaxValueEntropySearch(const Regressor& regressor, const unsigned num_max_value_samples = 64,
                                                             const unsigned num_global_search_iters = 100,
                                                             const unsigned num_local_search_iters  = 50,
                                                             const unsigned long long seed = 0, const int num_frequencies = 2048,
                                                             double* value = nullptr);
        /// The same from an explicit sample of y* and an explicit start set (D x S).
        Eigen::VectorXd FindNextPointByMaxValueEntropySearchFromStarts(const Regressor& regressor, const Eigen::VectorXd& max_values,
                                                                       const Eigen::MatrixXd& starts,
                                                                       const unsigned num_local_search_iters, double* value = nullptr);

        /// Joint entropy search (not in the reference; Hvarfner et al. 2022, Tu et al. 2022, include/sls_hip.h sls_jes_*).
        /// A Monte-Carlo sample of the OPTIMA of the latent function: locations (D x K) and values (K) of the maxima of num_samples
        /// pathwise posterior draws, found exactly as SampleMaxValues finds its values (same draws, same starts, same clamp: the
        /// values equal SampleMaxValues with the same arguments) with the locations kept.  num_samples <= 1024 for the calls below.
        /// A value that the clamp raised to the mean at the best data point keeps the location where the local search ended: such a
        /// pair (x*, f*) is not a point of its draw (the draw is lower there); JES conditions on it as on any other sampled pair.
        std::pair<Eigen::MatrixXd, Eigen::VectorXd> SampleOptima(const Regressor& regressor, const unsigned num_samples = 64,
                                                                 const unsigned num_global_search_iters = 100,
                                                                 const unsigned num_local_search_iters  = 50,
                                                                 const unsigned long long seed = 0, const int num_frequencies = 2048);
        /// alpha(x) of joint entropy search for the columns of Xs on the optima (optima_x D x K, optima_f K) (and its gradient, D x
        /// M, if grad != nullptr): one device pass.  The future observation's noise variance is max(b, 1e-12) of the regressor;
        /// star_noise is the variance with which an optimum value counts as observed (negative: the default 1e-8 a).
        Eigen::VectorXd CalcJointEntropies(const Regressor& regressor, const Eigen::MatrixXd& Xs, const Eigen::MatrixXd& optima_x,
                                           const Eigen::VectorXd& optima_f, Eigen::MatrixXd* grad = nullptr,
                                           const double star_noise = -1.0);
        /// Maximiser of alpha over [0,1]^D: SampleOptima, then one L-BFGS of num_local_search_iters evaluations (the tolerances of
        /// GetLocalSearchTolerances) from each of num_global_search_iters uniform starts, seeded exactly as
        /// FindNextPointByMaxValueEntropySearch is.  The same seed gives the same point.  value (may be nullptr) receives alpha there.
        Eigen::VectorXd FindNextPointByJointEntropySearch(const Regressor& regressor, const unsigned num_optima = 64,
                                                          const unsigned num_global_search_iters = 100,
                                                          const unsigned num_local_search_iters  = 50,
                                                          const unsigned long long seed = 0, const int num_frequencies = 2048,
                                                          double* value = nullptr);
        /// The same from an explicit sample of optima and an explicit start set (D x S).
        Eigen::VectorXd FindNextPointByJointEntropySearchFromStarts(const Regressor& regressor, const Eigen::MatrixXd& optima_x,
                                                                    const Eigen::VectorXd& optima_f, const Eigen::MatrixXd& starts,
                                                                    const unsigned num_local_search_iters, double* value = nullptr,
                                                                    const double star_noise = -1.0);

        /// Knowledge gradient on a discrete set (not in the reference; Frazier, Powell & Dayanik 2009; with the candidate itself in the
        /// set KGCP, Scott, Frazier & Powell 2011; include/sls_hip.h sls_kg_*): the expected gain of the highest posterior mean over
        /// ref_points (D x K, K <= 1024) -- plus the candidate when include_candidate -- from one noisy measurement at x, for the
        /// columns of Xs (and its gradient, D x M, if grad != nullptr): one device pass.  The baseline is the highest mean over
        /// ref_points alone, so the value is smooth in x.  The measurement's noise variance is max(b, 1e-12) of the regressor, as
        /// CalcJointEntropies passes it.
        Eigen::VectorXd CalcKnowledgeGradients(const Regressor& regressor, const Eigen::MatrixXd& Xs, const Eigen::MatrixXd& ref_points,
                                               Eigen::MatrixXd* grad = nullptr, const bool include_candidate = true);
        /// The default reference set: the regressor's data points; above 1024 of them the 1024 with the highest posterior mean
        /// (ties to the lower index), kept in increasing index order.
        Eigen::MatrixXd KnowledgeGradientReferencePoints(const Regressor& regressor);
        /// Maximiser of the knowledge gradient over [0,1]^D on the default reference set with the candidate included: one L-BFGS of
        /// num_local_search_iters evaluations (the tolerances of GetLocalSearchTolerances) from each of num_global_search_iters
        /// uniform starts, seeded exactly as FindNextPointByMaxValueEntropySearch seeds them.  The same seed gives the same point.
        /// value (may be nullptr) receives the knowledge gradient there.
        Eigen::VectorXd FindNextPointByKnowledgeGradient(const Regressor& regressor, const unsigned num_global_search_iters = 100,
                                                         const unsigned num_local_search_iters = 50, const unsigned long long seed = 0,
                                                         double* value = nullptr);
        /// The same from an explicit reference set and an explicit start set (D x S).
        Eigen::VectorXd FindNextPointByKnowledgeGradientFromStarts(const Regressor& regressor, const Eigen::MatrixXd& ref_points,
                                                                   const Eigen::MatrixXd& starts, const unsigned num_local_search_iters,
                                                                   double* value = nullptr, const bool include_candidate = true);

        /// Expected utility of the best option of a query pair (not in the reference; the q = 2 case of qEUBO, Astudillo et al.
        /// 2023, include/sls_hip.h sls_eubo_*): EUBO(x, x') = E[max(f(x), f(x'))] under the joint posterior of the two options,
        /// for the pairs (Xa.col(m), Xb.col(m)) (both D x M), and its gradients in x (grad_a, D x M) and x' (grad_b, D x M) where
        /// asked for: one device pass.  Device-resident regressors only (std::invalid_argument otherwise).
        Eigen::VectorXd CalcExpectedUtilitiesOfBestOption(const Regressor& regressor, const Eigen::MatrixXd& Xa, const Eigen::MatrixXd& Xb,
                                                          Eigen::MatrixXd* grad_a = nullptr, Eigen::MatrixXd* grad_b = nullptr);
        /// Maximiser (x, x') of EUBO over [0,1]^D x [0,1]^D: one L-BFGS of num_local_search_iters evaluations (the tolerances of
        /// GetLocalSearchTolerances) over the 2D coordinates from each of num_global_search_iters uniform starts of the generator
        /// FindNextPointByMaxValueEntropySearch uses, seeded with `seed`, all in lock step on the device.  The same seed gives the
        /// same pair.  value (may be nullptr) receives EUBO there.
        std::pair<Eigen::VectorXd, Eigen::VectorXd> FindNextQueryPairByExpectedUtility(const Regressor& regressor,
                                                                                       const unsigned   num_global_search_iters = 100,
                                                                                       const unsigned   num_local_search_iters  = 50,
                                                                                       const unsigned long long seed = 0,
                                                                                       double*                  value = nullptr);
        /// The same from an explicit start set (2D x S: rows 0..D-1 start x, rows D..2D-1 start x').
        std::pair<Eigen::VectorXd, Eigen::VectorXd> FindNextQueryPairByExpectedUtilityFromStarts(const Regressor&       regressor,
                                                                                                 const Eigen::MatrixXd& starts,
                                                                                                 const unsigned num_local_search_iters,
                                                                                                 double*        value = nullptr);

        /// A whole query of num_options >= 1 options by the expected utility of the best option on posterior draws (not in the
        /// reference; qEUBO, Astudillo et al. 2023, include/sls_hip.h sls_qeubo_*): num_draws pathwise posterior draws (stream
        /// `seed`, num_frequencies random features) fix the estimator (1 / num_draws) sum_s max_i f_s(x_i), which is maximised over
        /// [0,1]^(num_options D) jointly: one L-BFGS of num_local_search_iters evaluations (the tolerances of
        /// GetLocalSearchTolerances) from each of num_global_search_iters uniform starts of the generator
        /// FindNextQueryPairByExpectedUtility uses, seeded with `seed`, all in lock step on the device.  The same seed gives the same
        /// query.  value (may be nullptr) receives the utility there.  Device-resident regressors only (std::invalid_argument
        /// otherwise).
        std::vector<Eigen::VectorXd> FindNextQueryByExpectedUtility(const Regressor& regressor, const int num_options,
                                                                    const unsigned num_draws = 256,
                                                                    const unsigned num_global_search_iters = 100,
                                                                    const unsigned num_local_search_iters = 50,
                                                                    const unsigned long long seed = 0, const int num_frequencies = 2048,
                                                                    double* value = nullptr);
        /// The same from an explicit start set ((num_options D) x S: rows iD..iD+D-1 start option i).
        std::vector<Eigen::VectorXd> FindNextQueryByExpectedUtilityFromStarts(const Regressor& regressor, const int num_options,
                                                                              const Eigen::MatrixXd& starts,
                                                                              const unsigned num_draws = 256,
                                                                              const unsigned num_local_search_iters = 50,
                                                                              const unsigned long long seed = 0,
                                                                              const int num_frequencies = 2048, double* value = nullptr);

        /// A whole query of num_options options by the information it is expected to give (not in the reference; qBALD after
        /// Houlsby et al. 2011, include/sls_hip.h sls_qbald_*): the mutual information between the user's pick and the latent
        /// function under the BTL likelihood of scale btl_scale, estimated on num_draws pathwise posterior draws and maximised as
        /// FindNextQueryByExpectedUtility maximises its criterion (the same starts, tolerances and seed rule).  It asks which query
        /// teaches the model most, not where the best option is: the criterion for the first rounds of a session, or for learning
        /// the whole preference landscape.  With btl_scale far below the spread of the draws every query whose winner is uncertain
        /// is worth the same one answer and the search stalls; see the header.  value receives the information gain in nats.
        std::vector<Eigen::VectorXd> FindNextQueryByInformationGain(const Regressor& regressor, const int num_options,
                                                                    const double btl_scale, const unsigned num_draws = 256,
                                                                    const unsigned num_global_search_iters = 100,
                                                                    const unsigned num_local_search_iters = 50,
                                                                    const unsigned long long seed = 0, const int num_frequencies = 2048,
                                                                    double* value = nullptr);
        /// The same from an explicit start set ((num_options D) x S: rows iD..iD+D-1 start option i).
        std::vector<Eigen::VectorXd> FindNextQueryByInformationGainFromStarts(const Regressor& regressor, const int num_options,
                                                                              const double btl_scale, const Eigen::MatrixXd& starts,
                                                                              const unsigned num_draws = 256,
                                                                              const unsigned num_local_search_iters = 50,
                                                                              const unsigned long long seed = 0,
                                                                              const int num_frequencies = 2048, double* value = nullptr);

        /// A batch of num_points >= 1 points chosen jointly by noisy expected improvement on posterior draws (not in the reference;
        /// qNEI, Letham et al. 2019, include/sls_hip.h sls_qnei_*): num_draws pathwise posterior draws (SamplePosteriorFunctions with
        /// stream `seed` and num_frequencies random features) fix the estimator (1 / num_draws) sum_s max(0, max_i f_s(x_i) - t_s)
        /// with the incumbent t_s = max_j f_s(X_j) taken per draw over the regressor's data (MaxOverPoints(GetLargeX())) -- unlike
        /// FindNextPoints, which improves on a known number --, maximised over [0,1]^(num_points D) jointly: one L-BFGS of
        /// num_local_search_iters evaluations (the tolerances of GetLocalSearchTolerances) from each of num_global_search_iters
        /// uniform starts of the generator FindNextQueryByExpectedUtility uses, seeded with `seed`, all in lock step on the device.
        /// The same seed gives the same points.  value (may be nullptr) receives the improvement there.  Device-resident regressors
        /// only (std::invalid_argument otherwise).
        std::vector<Eigen::VectorXd> FindNextPointsByNoisyExpectedImprovement(const Regressor& regressor, const int num_points,
                                                                              const unsigned num_draws = 256,
                                                                              const unsigned num_global_search_iters = 100,
                                                                              const unsigned num_local_search_iters = 50,
                                                                              const unsigned long long seed = 0,
                                                                              const int num_frequencies = 2048, double* value = nullptr);
        /// The same from an explicit start set ((num_points D) x S: rows iD..iD+D-1 start point i).
        std::vector<Eigen::VectorXd> FindNextPointsByNoisyExpectedImprovementFromStarts(const Regressor& regressor, const int num_points,
                                                                                        const Eigen::MatrixXd& starts,
                                                                                        const unsigned num_draws = 256,
                                                                                        const unsigned num_local_search_iters = 50,
                                                                                        const unsigned long long seed = 0,
                                                                                        const int num_frequencies = 2048,
                                                                                        double* value = nullptr);

        /// The same batch by the log form of that criterion (not in the reference; qLogNEI after Ament et al. 2023, include/sls_hip.h
        /// sls_qlognei_*): a softplus of temperature tau_relu for max(0, .), a log-sum-exp of temperature tau_max for the max over
        /// the points and a log-sum-exp over the draws make the objective smooth, and a start that no draw improves -- stationary
        /// under FindNextPointsByNoisyExpectedImprovement -- has a gradient and moves.  value receives the LOG criterion.
        std::vector<Eigen::VectorXd> FindNextPointsByLogNoisyExpectedImprovement(const Regressor& regressor, const int num_points,
                                                                                 const unsigned num_draws = 256,
                                                                                 const unsigned num_global_search_iters = 100,
                                                                                 const unsigned num_local_search_iters = 50,
                                                                                 const unsigned long long seed = 0,
                                                                                 const int num_frequencies = 2048, double* value = nullptr,
                                                                                 const double tau_relu = 1e-6, const double tau_max = 1e-2);
        /// The same from an explicit start set ((num_points D) x S: rows iD..iD+D-1 start point i).
        std::vector<Eigen::VectorXd> FindNextPointsByLogNoisyExpectedImprovementFromStarts(
            const Regressor& regressor, const int num_points, const Eigen::MatrixXd& starts, const unsigned num_draws = 256,
            const unsigned num_local_search_iters = 50, const unsigned long long seed = 0, const int num_frequencies = 2048,
            double* value = nullptr, const double tau_relu = 1e-6, const double tau_max = 1e-2);

        /// The next slider by the expected utility of the best position on it (not in the reference; line EUBO, include/sls_hip.h
        /// sls_line_*): the query of SequentialLineSearchOptimizer is a line and the user picks the best point on it, so the
        /// criterion is E[max_t f((1 - t) a + t b)], estimated on num_positions grid positions (2 .. 16) over num_draws pathwise
        /// posterior draws (stream `seed`, num_frequencies random features) and maximised over the ends: with `anchor` (D values,
        /// e.g. the current best point) the first end is fixed there and the second is searched over [0,1]^D; with an empty anchor
        /// both ends are free ([0,1]^(2D)).  One L-BFGS of num_local_search_iters evaluations (the tolerances of
        /// GetLocalSearchTolerances) from each of num_global_search_iters uniform starts of the generator
        /// FindNextQueryByExpectedUtility uses, seeded with `seed`, all in lock step on the device.  The same seed gives the same
        /// slider.  value (may be nullptr) receives the utility there.  Device-resident regressors only (std::invalid_argument
        /// otherwise).
        std::pair<Eigen::VectorXd, Eigen::VectorXd> FindNextSliderByExpectedUtility(const Regressor& regressor, const Eigen::VectorXd& anchor,
                                                                                    const int      num_positions = 9,
                                                                                    const unsigned num_draws = 256,
                                                                                    const unsigned num_global_search_iters = 100,
                                                                                    const unsigned num_local_search_iters = 50,
                                                                                    const unsigned long long seed = 0,
                                                                                    const int num_frequencies = 2048, double* value = nullptr);
        /// The same from an explicit start set (2D x S: rows 0..D-1 start the first end; D x S with an anchor).
        std::pair<Eigen::VectorXd, Eigen::VectorXd> FindNextSliderByExpectedUtilityFromStarts(
            const Regressor& regressor, const Eigen::VectorXd& anchor, const Eigen::MatrixXd& starts, const int num_positions = 9,
            const unsigned num_draws = 256, const unsigned num_local_search_iters = 50, const unsigned long long seed = 0,
            const int num_frequencies = 2048, double* value = nullptr);

        /// The next gallery by the expected utility of the best cell of it (not in the reference; gallery EUBO, include/sls_hip.h
        /// sls_patch_*): the query of SequentialGallerySearchOptimizer is a two-dimensional patch of designs shown as a grid_s x
        /// grid_t grid (at least 2 per axis, at most 16 cells) and the user picks the best cell, so the criterion is
        /// E[max_{s,t} f(x(s,t))] on the grid of the bilinear patch spanned by four corners, over num_draws pathwise posterior draws
        /// (stream `seed`, num_frequencies random features), maximised over the corners: with `anchor` (D values, e.g. the current
        /// best point) the corner c00 is fixed there and the other three are searched over [0,1]^(3D); with an empty anchor all four
        /// are free ([0,1]^(4D)).  Starts, local search and tolerances as FindNextSliderByExpectedUtility; the same seed gives the
        /// same gallery.  Returns the corners c00, c10, c01, c11; value (may be nullptr) receives the utility there.  Device-resident
        /// regressors only (std::invalid_argument otherwise).
        std::vector<Eigen::VectorXd> FindNextGalleryByExpectedUtility(const Regressor& regressor, const Eigen::VectorXd& anchor,
                                                                      const int grid_s = 4, const int grid_t = 4,
                                                                      const unsigned num_draws = 256,
                                                                      const unsigned num_global_search_iters = 100,
                                                                      const unsigned num_local_search_iters = 50,
                                                                      const unsigned long long seed = 0,
                                                                      const int num_frequencies = 2048, double* value = nullptr);
        /// The same from an explicit start set (4D x S: rows in blocks of D start c00, c10, c01, c11; 3D x S with an anchor).
        std::vector<Eigen::VectorXd> FindNextGalleryByExpectedUtilityFromStarts(
            const Regressor& regressor, const Eigen::VectorXd& anchor, const Eigen::MatrixXd& starts, const int grid_s = 4,
            const int grid_t = 4, const unsigned num_draws = 256, const unsigned num_local_search_iters = 50,
            const unsigned long long seed = 0, const int num_frequencies = 2048, double* value = nullptr);

        /// The starts of every seeded search above and below (FindNextPointsByThompsonSampling, FindNextPointByMaxValueEntropySearch,
        /// FindNextPointInSubspace, ...): num_dims x count numbers uniform in [0,1), column after column from one std::mt19937_64
        /// seeded with `seed`.  With them and the tolerances of GetLocalSearchTolerances the ...FromStarts forms -- and the C ABI --
        /// reproduce a seeded call.
        Eigen::MatrixXd SeededUniformStarts(const unsigned num_dims, const long count, const unsigned long long seed);

        /// Search restricted to affine subspaces (not in the reference; include/sls_hip.h sls_acq_*_sub, sls_path_*_sub).  Device-
        /// resident regressors only (std::invalid_argument otherwise).
        /// Acquisition values at subspace.Point(Z.col(m)) (Z is d x M) and their gradient in z (d x M) if grad_z != nullptr.
        Eigen::VectorXd CalcAcquisitionValuesInSubspace(const Regressor& regressor, const SearchSubspace& subspace, const Eigen::MatrixXd& Z,
                                                        const AcquisitionFuncType func_type = AcquisitionFuncType::ExpectedImprovement,
                                                        const double gaussian_process_upper_confidence_bound_hyperparam = 1.0,
                                                        Eigen::MatrixXd* grad_z = nullptr);
        /// Maximiser of the acquisition function over the subspace: always the multi-start search, whatever the
        /// GlobalSearchStrategy -- one L-BFGS of num_local_search_iters evaluations (the tolerances of GetLocalSearchTolerances) in
        /// the d variables from each of num_global_search_iters uniform starts in [0,1]^d of the generator
        /// FindNextPointByMaxValueEntropySearch uses, seeded with `seed`.  The same seed gives the same point.  Returns the point
        /// x in R^D; value (may be nullptr) receives the acquisition value there.
        Eigen::VectorXd FindNextPointInSubspace(const Regressor& regressor, const SearchSubspace& subspace,
                                                const unsigned num_global_search_iters = 100, const unsigned num_local_search_iters = 50,
                                                const AcquisitionFuncType func_type = AcquisitionFuncType::ExpectedImprovement,
                                                const double gaussian_process_upper_confidence_bound_hyperparam = 1.0,
                                                const unsigned long long seed = 0, double* value = nullptr);
        /// Several subspaces of the same d in ONE lock-step search (several trust regions at once): start j (starts_z.col(j), d x S)
        /// searches subspaces[subspace_of_start[j]].  Returns the best end point over all of them; winner_subspace (may be nullptr)
        /// receives the subspace it lies in.
        Eigen::VectorXd FindNextPointInSubspacesFromStarts(const Regressor& regressor, const std::vector<SearchSubspace>& subspaces,
                                                           const std::vector<int>& subspace_of_start, const Eigen::MatrixXd& starts_z,
                                                           const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                           const double gaussian_process_upper_confidence_bound_hyperparam,
                                                           double* value = nullptr, int* winner_subspace = nullptr);
        /// FindNextPointInSubspace over SearchSubspace::Box(lower, upper).
        Eigen::VectorXd FindNextPointInBox(const Regressor& regressor, const Eigen::VectorXd& lower, const Eigen::VectorXd& upper,
                                           const unsigned num_global_search_iters = 100, const unsigned num_local_search_iters = 50,
                                           const AcquisitionFuncType func_type = AcquisitionFuncType::ExpectedImprovement,
                                           const double gaussian_process_upper_confidence_bound_hyperparam = 1.0,
                                           const unsigned long long seed = 0, double* value = nullptr);
        /// FindNextPointsByThompsonSampling with every draw maximised over the box [lower, upper] instead of the cube: the
        /// candidate step of a trust-region method (TuRBO).  The same seed gives the same points.
        std::vector<Eigen::VectorXd> FindNextPointsByThompsonSamplingInBox(const Regressor& regressor, const unsigned num_points,
                                                                           const Eigen::VectorXd& lower, const Eigen::VectorXd& upper,
                                                                           const unsigned num_global_search_iters = 100,
                                                                           const unsigned num_local_search_iters  = 50,
                                                                           const unsigned long long seed = 0,
                                                                           const int num_frequencies = 2048);
    } // namespace acquisition_func
} // namespace sequential_line_search

#endif
