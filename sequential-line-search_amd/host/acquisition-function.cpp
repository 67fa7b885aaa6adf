// acquisition_func over the C ABI (reference: src/acquisition-function.cpp).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <random>
#include <string>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/utils.hpp>
#include <stdexcept>

#include "device.hpp"

using Eigen::MatrixXd;
using Eigen::VectorXd;

namespace sequential_line_search
{
    namespace
    {
        int AcqId(AcquisitionFuncType t)
        {
            if (t == AcquisitionFuncType::LogExpectedImprovement) return SLS_ACQ_LOG_EXPECTED_IMPROVEMENT;
            return t == AcquisitionFuncType::ExpectedImprovement ? SLS_ACQ_EXPECTED_IMPROVEMENT : SLS_ACQ_GP_UCB;
        }
        // LogExpectedImprovement exists on the device only (there is no host erfcx): the stance of RequireHandle
        void RefuseLogEiOnHost(AcquisitionFuncType t)
        {
            if (t == AcquisitionFuncType::LogExpectedImprovement)
                throw std::invalid_argument("acquisition_func: LogExpectedImprovement needs a device-resident regressor "
                                            "(GaussianProcessRegressor / PreferenceRegressor); there is no host fallback");
        }

        // mathtoolbox::GetExpectedImprovement / ...Derivative for regressors WITHOUT a device
        // handle (user subclasses of Regressor): the reference's call structure on top of the virtual Predict* methods.
        double NormalCdf(double u) { return 0.5 * std::erfc(-u / std::sqrt(2.0)); }
        double NormalPdf(double u) { return std::exp(-0.5 * u * u) / std::sqrt(2.0 * M_PI); }

        double GenericValue(const Regressor& r, const VectorXd& x, AcquisitionFuncType type, double h)
        {
            RefuseLogEiOnHost(type);
            const double mu = r.PredictMu(x), sigma = r.PredictSigma(x);
            if (type == AcquisitionFuncType::GaussianProcessUpperConfidenceBound) return mu + h * sigma;
            const double diff = mu - r.PredictMu(r.PredictMaximumPointFromData());
            const double u    = diff / sigma;
            const double ei   = diff * NormalCdf(u) + sigma * NormalPdf(u);
            return (sigma < 1e-10 || std::isnan(ei)) ? 0.0 : ei;
        }
        VectorXd GenericDerivative(const Regressor& r, const VectorXd& x, AcquisitionFuncType type, double h)
        {
            RefuseLogEiOnHost(type);
            const VectorXd dm = r.PredictMuDerivative(x), ds = r.PredictSigmaDerivative(x);
            if (type == AcquisitionFuncType::GaussianProcessUpperConfidenceBound) return dm + h * ds;
            const double mu = r.PredictMu(x), sigma = r.PredictSigma(x);
            const double u  = (mu - r.PredictMu(r.PredictMaximumPointFromData())) / sigma;
            VectorXd     g  = NormalCdf(u) * dm + NormalPdf(u) * ds;
            bool         bad = sigma < 1e-10;
            for (long i = 0; i < g.size(); ++i) bad = bad || std::isnan(g(i));
            return bad ? VectorXd::Zero(x.size()) : g;
        }

        MatrixXd RandomStarts(unsigned num_dim, unsigned count)
        {
            // reference: x_ini = 0.5 (Random + 1) per start (src/acquisition-function.cpp:127), here drawn up front so that
            // the whole start set goes to the device in one transfer
            MatrixXd starts(num_dim, count);
            for (unsigned i = 0; i < count; ++i) eig::SetCol(starts, i, utils::GenerateRandomVector(num_dim));
            return starts;
        }

        // uniform starts in [0,1]^D as RandomStarts draws them, from a generator of their own so that `seed` fixes the whole batch
        MatrixXd SeededStarts(unsigned num_dim, long count, unsigned long long seed)
        {
            MatrixXd                               starts(num_dim, count);
            std::mt19937_64                        rng(seed);
            std::uniform_real_distribution<double> uni(0.0, 1.0);
            for (long j = 0; j < count; ++j)
                for (unsigned d = 0; d < num_dim; ++d) starts(d, j) = uni(rng);
            return starts;
        }

        GlobalSearchStrategy InitialStrategy()
        {
            if (const char* env = std::getenv("SLS_GLOBAL_SEARCH"))
            {
                const std::string v(env);
                if (v == "direct") return GlobalSearchStrategy::DirectThenLbfgs;
                if (v == "multistart") return GlobalSearchStrategy::ParallelMultiStart;
            }
#ifdef SEQUENTIAL_LINE_SEARCH_USE_PARALLELIZED_MULTI_START_SEARCH
            return GlobalSearchStrategy::ParallelMultiStart;
#else
            return GlobalSearchStrategy::DirectThenLbfgs;   // the reference's default build (CMakeLists.txt:33)
#endif
        }
        std::atomic<int> g_strategy{-1};

        sls_gp* RequireHandle(const Regressor& r)
        {
            sls_gp* h = r.GetDeviceHandle();
            if (!h)
                throw std::invalid_argument("acquisition_func: the multi-start maximiser needs a device-resident regressor "
                                            "(GaussianProcessRegressor / PreferenceRegressor); there is no host fallback");
            return h;
        }
    } // namespace

    namespace
    {
        sls_lbfgs_opts LocalSearchOpts()
        {
            sls_lbfgs_opts o;
            sls_lbfgs_default_opts(&o);
            optim::SearchTolerances(&o.ftol_rel, &o.xtol_rel);   // nloptutil::solve's defaults unless changed
            return o;
        }
    } // namespace
    void acquisition_func::SetLocalSearchTolerances(double f, double x) { optim::SetSearchTolerances(f, x); }
    void acquisition_func::GetLocalSearchTolerances(double* f, double* x) { optim::SearchTolerances(f, x); }
    void acquisition_func::SetMapFitTolerances(double f, double x) { optim::SetMapFitTolerances(f, x); }
    void acquisition_func::GetMapFitTolerances(double* f, double* x) { optim::MapFitTolerances(f, x); }

    void acquisition_func::SetGlobalSearchStrategy(GlobalSearchStrategy strategy) { g_strategy.store(static_cast<int>(strategy)); }
    GlobalSearchStrategy acquisition_func::GetGlobalSearchStrategy()
    {
        int v = g_strategy.load();
        if (v < 0)
        {
            v = static_cast<int>(InitialStrategy());
            g_strategy.store(v);
        }
        return static_cast<GlobalSearchStrategy>(v);
    }

    // reference: src/acquisition-function.cpp:170-198
    double acquisition_func::CalcAcquisitionValue(const Regressor& regressor, const VectorXd& x, const AcquisitionFuncType func_type,
                                                  const double hyperparam)
    {
        if (regressor.GetSmallY().rows() == 0) return 0.0;
        if (sls_gp* h = regressor.GetDeviceHandle())
        {
            double v = 0.0;
            device::Check(sls_acq_eval(h, AcqId(func_type), hyperparam, x.data(), 1, &v, nullptr), "sls_acq_eval");
            return v;
        }
        return GenericValue(regressor, x, func_type, hyperparam);
    }

    // reference: src/acquisition-function.cpp:200-230
    VectorXd acquisition_func::CalcAcquisitionValueDerivative(const Regressor& regressor, const VectorXd& x,
                                                              const AcquisitionFuncType func_type, const double hyperparam)
    {
        if (regressor.GetSmallY().rows() == 0) return VectorXd::Zero(x.size());
        if (sls_gp* h = regressor.GetDeviceHandle())
        {
            double   v = 0.0;
            VectorXd g(x.size());
            device::Check(sls_acq_eval(h, AcqId(func_type), hyperparam, x.data(), 1, &v, g.data()), "sls_acq_eval");
            return g;
        }
        return GenericDerivative(regressor, x, func_type, hyperparam);
    }

    VectorXd acquisition_func::CalcAcquisitionValues(const Regressor& regressor, const MatrixXd& Xs, const AcquisitionFuncType func_type,
                                                     const double hyperparam, MatrixXd* grad)
    {
        const long M = Xs.cols();
        VectorXd   v = VectorXd::Zero(M);
        if (grad) *grad = MatrixXd::Zero(Xs.rows(), M);
        if (regressor.GetSmallY().rows() == 0) return v;
        device::Check(sls_acq_eval(RequireHandle(regressor), AcqId(func_type), hyperparam, Xs.data(), static_cast<int>(M), v.data(),
                                   grad ? grad->data() : nullptr),
                      "sls_acq_eval");
        return v;
    }

    VectorXd acquisition_func::FindNextPointFromStarts(const Regressor& regressor, const MatrixXd& starts,
                                                       const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                       const double hyperparam, double* value)
    {
        VectorXd x(starts.rows());
        double   v   = 0.0;
        long     idx = 0;
        // several GPUs configured (device::SetDevices / $SLS_DEVICES): the iterations of the reference's parallel multi-start
        // loop (:125-141) share only the const regressor, so the start set is split over the devices, each holding a replica of
        // the fitted state, and the per-device winners meet in ONE ncclAllGather.  The replicas belong to the regressor's device
        // handle: they are built on the first call (the shard on the primary's device IS the primary: no second fit there) and
        // reused by every later one.
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // nloptutil::solve's relative tolerances
        // (a Laplace regressor runs on the primary device: replicas are plain fits of (X, y) and would carry the plain variance)
        if (std::shared_ptr<device::MultiGpHandle> replicas =
                regressor.UsesLaplacePosterior() ? nullptr : device::ReplicasFor(RequireHandle(regressor), regressor.GetLargeX().cols()))
        {
            device::Check(sls_multi_acq_maximize(replicas->h, AcqId(func_type), hyperparam, starts.data(),
                                                 static_cast<int>(starts.cols()), static_cast<int>(num_local_search_iters), &lopts,
                                                 x.data(), &v, &idx, nullptr),
                          "sls_multi_acq_maximize");
            if (value) *value = v;
            return x;
        }
        device::Check(sls_acq_maximize(RequireHandle(regressor), AcqId(func_type), hyperparam, starts.data(),
                                       static_cast<int>(starts.cols()), static_cast<int>(num_local_search_iters), &lopts, 0, x.data(),
                                       &v, &idx, nullptr, nullptr),
                      "sls_acq_maximize");
        if (value) *value = v;
        return x;
    }

    // reference: src/acquisition-function.cpp:155-165 -- DIRECT (num_global_search_iters evaluations), then L-BFGS
    // (num_local_search_iters evaluations) from its result.  Every DIRECT iteration is ONE batched device evaluation.
    VectorXd acquisition_func::FindNextPointDirect(const Regressor& regressor, const unsigned num_global_search_iters,
                                                   const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                   const double hyperparam, double* value)
    {
        const unsigned num_dim = regressor.GetNumDims();
        sls_gp*        h       = RequireHandle(regressor);
        // SLS_HOST_TIMING: where the time of one call goes (stderr) -- DIRECT's own bookkeeping on the host, its batched device
        // evaluations, the local phase
        static const bool timing = std::getenv("SLS_HOST_TIMING") != nullptr;   // read once per process
        using clk         = std::chrono::steady_clock;
        double ms_dev = 0.0;
        int    batches = 0;
        const optim::BatchObjective objective = [&](const std::vector<std::vector<double>>& xs, std::vector<double>& values) {
            const auto t0 = clk::now();
            MatrixXd Xs(num_dim, static_cast<long>(xs.size()));
            for (size_t m = 0; m < xs.size(); ++m)
                for (unsigned d = 0; d < num_dim; ++d) Xs(d, static_cast<long>(m)) = xs[m][d];
            values.resize(xs.size());
            device::Check(sls_acq_eval(h, AcqId(func_type), hyperparam, Xs.data(), static_cast<int>(xs.size()), values.data(), nullptr),
                          "sls_acq_eval");
            ms_dev += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
            ++batches;
        };
        const std::vector<double> lower(num_dim, 0.0), upper(num_dim, 1.0);
        const auto                t_direct0 = clk::now();
        const std::vector<double> xg = optim::DirectMaximize(objective, lower, upper, static_cast<int>(num_global_search_iters));
        const double ms_direct = std::chrono::duration<double, std::milli>(clk::now() - t_direct0).count();
        const auto   t_local0  = clk::now();
        struct Report {
            bool on; double direct, dev; int batches; clk::time_point t0;
            ~Report() {
                if (on)
                    std::fprintf(stderr, "  FindNextPointDirect: DIRECT %.2f ms (%d batched evaluations: %.2f ms on the device side, %.2f ms host bookkeeping), local phase %.2f ms\n",
                                 direct, batches, dev, direct - dev, std::chrono::duration<double, std::milli>(clk::now() - t0).count());
            }
        } report{timing, ms_direct, ms_dev, batches, t_local0};
        MatrixXd start(num_dim, 1);
        for (unsigned d = 0; d < num_dim; ++d) start(d, 0) = xg[d];
        if (num_local_search_iters == 0)
        {
            VectorXd x(num_dim);
            for (unsigned d = 0; d < num_dim; ++d) x(d) = xg[d];
            if (value) *value = CalcAcquisitionValue(regressor, x, func_type, hyperparam);
            return x;
        }
        VectorXd x(num_dim);
        double   v   = 0.0;
        long     idx = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // nloptutil::solve's relative tolerances
        device::Check(sls_acq_maximize(h, AcqId(func_type), hyperparam, start.data(), 1, static_cast<int>(num_local_search_iters), &lopts,
                                       0, x.data(), &v, &idx, nullptr, nullptr),
                      "sls_acq_maximize");
        if (value) *value = v;
        return x;
    }

    // reference: src/acquisition-function.cpp:232-244 + FindGlobalSolution :112-167 (both branches, chosen at run time)
    VectorXd acquisition_func::FindNextPoint(const Regressor& regressor, const unsigned num_global_search_iters,
                                             const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                             const double hyperparam)
    {
        const unsigned num_dim = regressor.GetNumDims();
        if (GetGlobalSearchStrategy() == GlobalSearchStrategy::DirectThenLbfgs)
            return FindNextPointDirect(regressor, num_global_search_iters, num_local_search_iters, func_type, hyperparam);
        return FindNextPointFromStarts(regressor, RandomStarts(num_dim, num_global_search_iters), num_local_search_iters, func_type,
                                       hyperparam);
    }

    // reference: src/acquisition-function.cpp:246-298
    std::vector<VectorXd> acquisition_func::FindNextPoints(const Regressor& regressor, const unsigned num_points,
                                                           const unsigned num_global_search_iters,
                                                           const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                           const double hyperparam)
    {
        const unsigned        num_dim = regressor.GetNumDims();
        std::vector<VectorXd> points;
        if (regressor.UsesLaplacePosterior())
        {
            // Schonlau's trick conditions the variance on pseudo-observations: on a plain GP that is one appended point, on the Laplace
            // posterior it is not defined here.  One point needs no pseudo-observation: the single-point search, on the Laplace variance.
            if (num_points > 1)
                throw std::runtime_error("acquisition_func::FindNextPoints: more than one point appends pseudo-observations (Schonlau's trick), "
                                         "which a regressor with the Laplace posterior does not support; use a draw-based batch criterion: "
                                         "FindNextQueryByExpectedUtility, FindNextQueryByInformationGain, "
                                         "FindNextPointsByNoisyExpectedImprovement or FindNextPointsByThompsonSampling");
            if (num_points == 1)
                points.push_back(FindNextPoint(regressor, num_global_search_iters, num_local_search_iters, func_type, hyperparam));
            return points;
        }
        sls_gp*               mean_handle = RequireHandle(regressor);
        const VectorXd        theta       = regressor.GetKernelHyperparams();

        // Dummy regressor that only tracks the variance.  Like the reference (:261-262, :293) it is built with the
        // DEFAULT kernel type (Matern-5/2), not the regressor's own -- reproduced on purpose.
        // It never exposes m_K_y / m_K_y_inv, so it is built without the host copies (per-object flag: no global state).
        std::shared_ptr<GaussianProcessRegressor> temp = std::make_shared<GaussianProcessRegressor>(
            regressor.GetLargeX(), regressor.GetSmallY(), theta, regressor.GetNoiseHyperparam(), KernelType::ArdMatern52Kernel,
            /*materialize_matrices=*/false);

        for (unsigned i = 0; i < num_points; ++i)
        {
            // FindGlobalSolution on objective_for_multiple_points (:265-278): both branches, as in FindNextPoint
            MatrixXd starts;
            if (GetGlobalSearchStrategy() == GlobalSearchStrategy::DirectThenLbfgs)
            {
                const optim::BatchObjective objective = [&](const std::vector<std::vector<double>>& xs, std::vector<double>& values) {
                    MatrixXd Xs(num_dim, static_cast<long>(xs.size()));
                    for (size_t m = 0; m < xs.size(); ++m)
                        for (unsigned d = 0; d < num_dim; ++d) Xs(d, static_cast<long>(m)) = xs[m][d];
                    values.resize(xs.size());
                    device::Check(sls_acq_eval_pair(mean_handle, temp->GetDeviceHandle(), AcqId(func_type), hyperparam, Xs.data(),
                                                    static_cast<int>(xs.size()), values.data(), nullptr),
                                  "sls_acq_eval_pair");
                };
                const std::vector<double> lower(num_dim, 0.0), upper(num_dim, 1.0);
                const std::vector<double> xg = optim::DirectMaximize(objective, lower, upper, static_cast<int>(num_global_search_iters));
                starts = MatrixXd(num_dim, 1);
                for (unsigned d = 0; d < num_dim; ++d) starts(d, 0) = xg[d];
            }
            else
            {
                starts = RandomStarts(num_dim, num_global_search_iters);
            }
            VectorXd x_star(num_dim);
            double   v   = 0.0;
            long     idx = 0;
            const sls_lbfgs_opts lopts = LocalSearchOpts();   // nloptutil::solve's relative tolerances
            device::Check(sls_acq_maximize_pair(mean_handle, temp->GetDeviceHandle(), AcqId(func_type), hyperparam, starts.data(),
                                                static_cast<int>(starts.cols()),
                                                std::max(1, static_cast<int>(num_local_search_iters)), &lopts, x_star.data(), &v, &idx),
                          "sls_acq_maximize_pair");
            points.push_back(x_star);
            if (points.size() != num_points)
            {
                // append the new point to the dummy regressor; its value is irrelevant for the variance (the reference
                // uses PredictMu, :286-289).  The reference rebuilds the regressor (:293); here the fitted state grows by a
                // rank-1 update on the device.
                temp->AppendPoint(x_star, temp->PredictMu(x_star));
            }
        }
        return points;
    }

    std::vector<VectorXd> acquisition_func::FindNextPointsByThompsonSampling(const Regressor& regressor, const unsigned num_points,
                                                                             const unsigned num_global_search_iters,
                                                                             const unsigned num_local_search_iters,
                                                                             const unsigned long long seed, const int num_frequencies)
    {
        const unsigned S = std::max(1u, num_global_search_iters);
        return FindNextPointsByThompsonSamplingFromStarts(regressor, num_points,
                                                          SeededStarts(regressor.GetNumDims(), static_cast<long>(num_points) * S, seed),
                                                          num_local_search_iters, seed, num_frequencies);
    }

    std::vector<VectorXd> acquisition_func::FindNextPointsByThompsonSamplingFromStarts(const Regressor& regressor, const unsigned num_points,
                                                                                       const MatrixXd& starts,
                                                                                       const unsigned num_local_search_iters,
                                                                                       const unsigned long long seed,
                                                                                       const int num_frequencies)
    {
        if (num_points == 0) return {};
        RequireHandle(regressor);
        const PosteriorFunctionSamples draws = regressor.SamplePosteriorFunctions(static_cast<int>(num_points), seed, num_frequencies);
        return draws.Maximize(starts, num_local_search_iters);
    }

    // ---- max-value entropy search (include/sls_hip.h sls_mes_*; Wang & Jegelka 2017) ----
    VectorXd acquisition_func::SampleMaxValues(const Regressor& regressor, const unsigned num_samples,
                                               const unsigned num_global_search_iters, const unsigned num_local_search_iters,
                                               const unsigned long long seed, const int num_frequencies)
    {
        // the values of the sampled optima (draws, starts and the clamp at the mean at the best data point are SampleOptima's)
        return SampleOptima(regressor, num_samples, num_global_search_iters, num_local_search_iters, seed, num_frequencies).second;
    }

    VectorXd acquisition_func::CalcMaxValueEntropies(const Regressor& regressor, const MatrixXd& Xs, const VectorXd& max_values,
                                                     MatrixXd* grad)
    {
        const long M = Xs.cols();
        VectorXd   v = VectorXd::Zero(M);
        if (grad) *grad = MatrixXd::Zero(Xs.rows(), M);
        if (regressor.GetSmallY().rows() == 0) return v;
        device::Check(sls_mes_eval(RequireHandle(regressor), max_values.data(), static_cast<int>(max_values.size()), Xs.data(),
                                   static_cast<int>(M), v.data(), grad ? grad->data() : nullptr),
                      "sls_mes_eval");
        return v;
    }

    VectorXd acquisition_func::FindNextPointByMaxValueEntropySearchFromStarts(const Regressor& regressor, const VectorXd& max_values,
                                                                              const MatrixXd& starts,
                                                                              const unsigned  num_local_search_iters, double* value)
    {
        VectorXd             x(starts.rows());
        double               v     = 0.0;
        long                 idx   = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // GetLocalSearchTolerances
        device::Check(sls_mes_maximize(RequireHandle(regressor), max_values.data(), static_cast<int>(max_values.size()), starts.data(),
                                       static_cast<int>(starts.cols()), std::max(1, static_cast<int>(num_local_search_iters)), &lopts, 0,
                                       x.data(), &v, &idx, nullptr, nullptr),
                      "sls_mes_maximize");
        if (value) *value = v;
        return x;
    }

    VectorXd acquisition_func::FindNextPointByMaxValueEntropySearch(const Regressor& regressor, const unsigned num_max_value_samples,
                                                                    const unsigned num_global_search_iters,
                                                                    const unsigned num_local_search_iters, const unsigned long long seed,
                                                                    const int num_frequencies, double* value)
    {
        const VectorXd max_values =
            SampleMaxValues(regressor, num_max_value_samples, num_global_search_iters, num_local_search_iters, seed, num_frequencies);
        return FindNextPointByMaxValueEntropySearchFromStarts(
            regressor, max_values, SeededStarts(regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed),
            num_local_search_iters, value);
    }

    // ---- joint entropy search (include/sls_hip.h sls_jes_*; Hvarfner et al. 2022, Tu et al. 2022) ----
    namespace
    {
        // the snapshot of the conditioned optima for the length of one call
        struct JesObject
        {
            sls_jes* h = nullptr;
            JesObject(const Regressor& r, const MatrixXd& optima_x, const VectorXd& optima_f, double star_noise)
            {
                if (optima_x.rows() != static_cast<long>(r.GetNumDims()) || optima_x.cols() != optima_f.size())
                    throw std::invalid_argument("acquisition_func: optima_x must be D x K and optima_f K long");
                device::Check(sls_jes_create(RequireHandle(r), optima_x.data(), optima_f.data(), static_cast<int>(optima_f.size()),
                                             star_noise, &h),
                              "sls_jes_create");
            }
            ~JesObject() { sls_jes_destroy(h); }
            JesObject(const JesObject&)            = delete;
            JesObject& operator=(const JesObject&) = delete;
        };
        // a < 0 as the argument: the default 1e-8 a
        double StarNoise(const Regressor& r, double star_noise) { return star_noise < 0.0 ? 1e-8 * r.GetKernelHyperparams()(0) : star_noise; }
        double FutureNoise(const Regressor& r) { return std::max(r.GetNoiseHyperparam(), 1e-12); }
    }   // namespace

    std::pair<MatrixXd, VectorXd> acquisition_func::SampleOptima(const Regressor& regressor, const unsigned num_samples,
                                                                 const unsigned num_global_search_iters,
                                                                 const unsigned num_local_search_iters, const unsigned long long seed,
                                                                 const int num_frequencies)
    {
        const unsigned D = regressor.GetNumDims();
        if (num_samples == 0) return {MatrixXd(D, 0), VectorXd()};
        sls_gp*        h = RequireHandle(regressor);
        const unsigned S = std::max(1u, num_global_search_iters);
        const PosteriorFunctionSamples draws = regressor.SamplePosteriorFunctions(static_cast<int>(num_samples), seed, num_frequencies);
        VectorXd                       values;
        const std::vector<VectorXd>    xs =
            draws.Maximize(SeededStarts(D, static_cast<long>(num_samples) * S, seed), num_local_search_iters, &values);
        // the maximum of a function is at least its value at the best data point (a local search may have ended below it)
        double mu_best = 0.0;
        device::Check(sls_gp_get_summary(h, nullptr, &mu_best, nullptr), "sls_gp_get_summary");
        MatrixXd X(D, static_cast<long>(xs.size()));
        for (long k = 0; k < values.size(); ++k)
        {
            X.col(k)  = xs[static_cast<size_t>(k)];
            values(k) = std::max(values(k), mu_best);
        }
        return {X, values};
    }

    VectorXd acquisition_func::CalcJointEntropies(const Regressor& regressor, const MatrixXd& Xs, const MatrixXd& optima_x,
                                                  const VectorXd& optima_f, MatrixXd* grad, const double star_noise)
    {
        const long M = Xs.cols();
        VectorXd   v = VectorXd::Zero(M);
        if (grad) *grad = MatrixXd::Zero(Xs.rows(), M);
        if (regressor.GetSmallY().rows() == 0 || M == 0) return v;
        const JesObject j(regressor, optima_x, optima_f, StarNoise(regressor, star_noise));
        device::Check(sls_jes_eval(j.h, FutureNoise(regressor), Xs.data(), static_cast<int>(M), v.data(), grad ? grad->data() : nullptr,
                                   nullptr),
                      "sls_jes_eval");
        return v;
    }

    VectorXd acquisition_func::FindNextPointByJointEntropySearchFromStarts(const Regressor& regressor, const MatrixXd& optima_x,
                                                                           const VectorXd& optima_f, const MatrixXd& starts,
                                                                           const unsigned num_local_search_iters, double* value,
                                                                           const double star_noise)
    {
        VectorXd             x(starts.rows());
        double               v     = 0.0;
        long                 idx   = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // GetLocalSearchTolerances
        const JesObject      j(regressor, optima_x, optima_f, StarNoise(regressor, star_noise));
        device::Check(sls_jes_maximize(j.h, FutureNoise(regressor), starts.data(), static_cast<int>(starts.cols()),
                                       std::max(1, static_cast<int>(num_local_search_iters)), &lopts, 0, x.data(), &v, &idx, nullptr,
                                       nullptr),
                      "sls_jes_maximize");
        if (value) *value = v;
        return x;
    }

    VectorXd acquisition_func::FindNextPointByJointEntropySearch(const Regressor& regressor, const unsigned num_optima,
                                                                 const unsigned num_global_search_iters,
                                                                 const unsigned num_local_search_iters, const unsigned long long seed,
                                                                 const int num_frequencies, double* value)
    {
        const std::pair<MatrixXd, VectorXd> optima =
            SampleOptima(regressor, num_optima, num_global_search_iters, num_local_search_iters, seed, num_frequencies);
        return FindNextPointByJointEntropySearchFromStarts(
            regressor, optima.first, optima.second, SeededStarts(regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed),
            num_local_search_iters, value);
    }

    // ---- knowledge gradient on a discrete set (include/sls_hip.h sls_kg_*; Frazier et al. 2009, Scott et al. 2011) ----
    namespace
    {
        // the snapshot of the fixed points for the length of one call
        struct KgObject
        {
            sls_kg* h = nullptr;
            KgObject(const Regressor& r, const MatrixXd& ref_points)
            {
                if (ref_points.rows() != static_cast<long>(r.GetNumDims()) || ref_points.cols() < 1)
                    throw std::invalid_argument("acquisition_func: ref_points must be D x K, K >= 1");
                device::Check(sls_kg_create(RequireHandle(r), ref_points.data(), static_cast<int>(ref_points.cols()), &h), "sls_kg_create");
            }
            ~KgObject() { sls_kg_destroy(h); }
            KgObject(const KgObject&)            = delete;
            KgObject& operator=(const KgObject&) = delete;
        };
    }   // namespace

    MatrixXd acquisition_func::KnowledgeGradientReferencePoints(const Regressor& regressor)
    {
        const MatrixXd& X = regressor.GetLargeX();
        const long      N = X.cols();
        if (N <= SLS_KG_MAX_POINTS) return X;
        VectorXd mu(N);
        device::Check(sls_gp_predict(RequireHandle(regressor), X.data(), static_cast<int>(N), mu.data(), nullptr), "sls_gp_predict");
        std::vector<long> order(static_cast<size_t>(N));
        for (long i = 0; i < N; ++i) order[static_cast<size_t>(i)] = i;
        // the SLS_KG_MAX_POINTS highest means, ties to the lower index, kept in increasing index order
        std::stable_sort(order.begin(), order.end(), [&](long p, long q) { return mu(p) > mu(q); });
        order.resize(SLS_KG_MAX_POINTS);
        std::sort(order.begin(), order.end());
        MatrixXd R(X.rows(), SLS_KG_MAX_POINTS);
        for (long k = 0; k < SLS_KG_MAX_POINTS; ++k)
            for (long d = 0; d < X.rows(); ++d) R(d, k) = X(d, order[static_cast<size_t>(k)]);
        return R;
    }

    VectorXd acquisition_func::CalcKnowledgeGradients(const Regressor& regressor, const MatrixXd& Xs, const MatrixXd& ref_points,
                                                      MatrixXd* grad, const bool include_candidate)
    {
        const long M = Xs.cols();
        VectorXd   v = VectorXd::Zero(M);
        if (grad) *grad = MatrixXd::Zero(Xs.rows(), M);
        if (regressor.GetSmallY().rows() == 0 || M == 0) return v;
        const KgObject k(regressor, ref_points);
        device::Check(sls_kg_eval(k.h, FutureNoise(regressor), include_candidate ? 1 : 0, Xs.data(), static_cast<int>(M), v.data(),
                                  grad ? grad->data() : nullptr, nullptr),
                      "sls_kg_eval");
        return v;
    }

    VectorXd acquisition_func::FindNextPointByKnowledgeGradientFromStarts(const Regressor& regressor, const MatrixXd& ref_points,
                                                                          const MatrixXd& starts, const unsigned num_local_search_iters,
                                                                          double* value, const bool include_candidate)
    {
        VectorXd             x(starts.rows());
        double               v     = 0.0;
        long                 idx   = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // GetLocalSearchTolerances
        const KgObject       k(regressor, ref_points);
        device::Check(sls_kg_maximize(k.h, FutureNoise(regressor), include_candidate ? 1 : 0, starts.data(), static_cast<int>(starts.cols()),
                                      std::max(1, static_cast<int>(num_local_search_iters)), &lopts, 0, x.data(), &v, &idx, nullptr,
                                      nullptr),
                      "sls_kg_maximize");
        if (value) *value = v;
        return x;
    }

    VectorXd acquisition_func::FindNextPointByKnowledgeGradient(const Regressor& regressor, const unsigned num_global_search_iters,
                                                                const unsigned num_local_search_iters, const unsigned long long seed,
                                                                double* value)
    {
        return FindNextPointByKnowledgeGradientFromStarts(
            regressor, KnowledgeGradientReferencePoints(regressor),
            SeededStarts(regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed), num_local_search_iters, value);
    }

    // ---- expected utility of the best option of a query pair (include/sls_hip.h sls_eubo_*; Astudillo et al. 2023) ----
    namespace
    {
        sls_gp* RequireDeviceHandleForExpectedUtility(const Regressor& r)
        {
            sls_gp* h = r.GetDeviceHandle();
            if (!h)
                throw std::invalid_argument("acquisition_func: the expected utility of the best option needs a device-resident regressor "
                                            "(GaussianProcessRegressor / PreferenceRegressor); there is no host fallback");
            return h;
        }
    } // namespace

    VectorXd acquisition_func::CalcExpectedUtilitiesOfBestOption(const Regressor& regressor, const MatrixXd& Xa, const MatrixXd& Xb,
                                                                 MatrixXd* grad_a, MatrixXd* grad_b)
    {
        sls_gp* h = RequireDeviceHandleForExpectedUtility(regressor);
        if (Xa.rows() != Xb.rows() || Xa.cols() != Xb.cols())
            throw std::invalid_argument("CalcExpectedUtilitiesOfBestOption: Xa and Xb must have the same shape");
        const long D = Xa.rows(), M = Xa.cols();
        MatrixXd   pairs(2 * D, M);
        for (long m = 0; m < M; ++m)
            for (long d = 0; d < D; ++d)
            {
                pairs(d, m)     = Xa(d, m);
                pairs(D + d, m) = Xb(d, m);
            }
        VectorXd       v = VectorXd::Zero(M);
        const bool     want_grad = grad_a || grad_b;
        MatrixXd       g(want_grad ? 2 * D : 0, want_grad ? M : 0);
        device::Check(sls_eubo_eval(h, pairs.data(), static_cast<int>(M), v.data(), want_grad ? g.data() : nullptr), "sls_eubo_eval");
        for (int o = 0; o < 2; ++o)
        {
            MatrixXd* out = o == 0 ? grad_a : grad_b;
            if (!out) continue;
            *out = MatrixXd(D, M);
            for (long m = 0; m < M; ++m)
                for (long d = 0; d < D; ++d) (*out)(d, m) = g(o * D + d, m);
        }
        return v;
    }

    std::pair<VectorXd, VectorXd> acquisition_func::FindNextQueryPairByExpectedUtilityFromStarts(const Regressor& regressor,
                                                                                                const MatrixXd&  starts,
                                                                                                const unsigned   num_local_search_iters,
                                                                                                double*          value)
    {
        sls_gp*    h = RequireDeviceHandleForExpectedUtility(regressor);
        const long D = regressor.GetNumDims();
        if (starts.rows() != 2 * D || starts.cols() < 1)
            throw std::invalid_argument("FindNextQueryPairByExpectedUtilityFromStarts: starts must be 2D x S with S >= 1");
        VectorXd             x(2 * D);
        double               v     = 0.0;
        long                 idx   = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // GetLocalSearchTolerances
        device::Check(sls_eubo_maximize(h, starts.data(), static_cast<int>(starts.cols()),
                                        std::max(1, static_cast<int>(num_local_search_iters)), &lopts, 0, x.data(), &v, &idx, nullptr,
                                        nullptr),
                      "sls_eubo_maximize");
        if (value) *value = v;
        return std::make_pair(x.segment(0, D), x.segment(D, D));
    }

    std::pair<VectorXd, VectorXd> acquisition_func::FindNextQueryPairByExpectedUtility(const Regressor& regressor,
                                                                                      const unsigned   num_global_search_iters,
                                                                                      const unsigned   num_local_search_iters,
                                                                                      const unsigned long long seed, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        return FindNextQueryPairByExpectedUtilityFromStarts(
            regressor, SeededStarts(2 * regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed), num_local_search_iters,
            value);
    }

    // ---- expected utility of the best of q options on posterior draws (include/sls_hip.h sls_qeubo_*) ----
    std::vector<VectorXd> acquisition_func::FindNextQueryByExpectedUtilityFromStarts(const Regressor& regressor, const int num_options,
                                                                                     const MatrixXd& starts, const unsigned num_draws,
                                                                                     const unsigned           num_local_search_iters,
                                                                                     const unsigned long long seed,
                                                                                     const int num_frequencies, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        return draws.MaximizeExpectedUtilityOfBestOption(num_options, starts, num_local_search_iters, value);
    }

    std::vector<VectorXd> acquisition_func::FindNextQueryByExpectedUtility(const Regressor& regressor, const int num_options,
                                                                           const unsigned num_draws,
                                                                           const unsigned num_global_search_iters,
                                                                           const unsigned num_local_search_iters,
                                                                           const unsigned long long seed, const int num_frequencies,
                                                                           double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (num_options < 1 || num_options > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextQueryByExpectedUtility: 1 .. 16 options");
        return FindNextQueryByExpectedUtilityFromStarts(
            regressor, num_options, SeededStarts(num_options * regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed),
            num_draws, num_local_search_iters, seed, num_frequencies, value);
    }

    // ---- information gain of a choice query on posterior draws (include/sls_hip.h sls_qbald_*; Houlsby et al. 2011) ----
    std::vector<VectorXd> acquisition_func::FindNextQueryByInformationGainFromStarts(const Regressor& regressor, const int num_options,
                                                                                     const double btl_scale, const MatrixXd& starts,
                                                                                     const unsigned           num_draws,
                                                                                     const unsigned           num_local_search_iters,
                                                                                     const unsigned long long seed,
                                                                                     const int num_frequencies, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        return draws.MaximizeChoiceInformationGain(num_options, btl_scale, starts, num_local_search_iters, value);
    }

    std::vector<VectorXd> acquisition_func::FindNextQueryByInformationGain(const Regressor& regressor, const int num_options,
                                                                           const double btl_scale, const unsigned num_draws,
                                                                           const unsigned num_global_search_iters,
                                                                           const unsigned num_local_search_iters,
                                                                           const unsigned long long seed, const int num_frequencies,
                                                                           double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (num_options < 1 || num_options > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextQueryByInformationGain: 1 .. 16 options");
        return FindNextQueryByInformationGainFromStarts(
            regressor, num_options, btl_scale,
            SeededStarts(num_options * regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed), num_draws,
            num_local_search_iters, seed, num_frequencies, value);
    }

    // ---- noisy expected improvement of a batch on posterior draws (include/sls_hip.h sls_qnei_*; Letham et al. 2019) ----
    std::vector<VectorXd> acquisition_func::FindNextPointsByNoisyExpectedImprovementFromStarts(
        const Regressor& regressor, const int num_points, const MatrixXd& starts, const unsigned num_draws,
        const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies, double* value)
    {
        if (!regressor.GetDeviceHandle())
            throw std::invalid_argument("acquisition_func: noisy expected improvement needs a device-resident regressor "
                                        "(GaussianProcessRegressor / PreferenceRegressor); there is no host fallback");
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        const VectorXd incumbents = draws.MaxOverPoints(regressor.GetLargeX());   // per draw, from the draw that evaluates the candidates
        return draws.MaximizeNoisyExpectedImprovement(num_points, incumbents, starts, num_local_search_iters, value);
    }

    std::vector<VectorXd> acquisition_func::FindNextPointsByNoisyExpectedImprovement(
        const Regressor& regressor, const int num_points, const unsigned num_draws, const unsigned num_global_search_iters,
        const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies, double* value)
    {
        if (num_points < 1 || num_points > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextPointsByNoisyExpectedImprovement: 1 .. 16 points");
        return FindNextPointsByNoisyExpectedImprovementFromStarts(
            regressor, num_points, SeededStarts(num_points * regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed),
            num_draws, num_local_search_iters, seed, num_frequencies, value);
    }

    // ---- its log form (include/sls_hip.h sls_qlognei_*; Ament et al. 2023) ----
    std::vector<VectorXd> acquisition_func::FindNextPointsByLogNoisyExpectedImprovementFromStarts(
        const Regressor& regressor, const int num_points, const MatrixXd& starts, const unsigned num_draws,
        const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies, double* value,
        const double tau_relu, const double tau_max)
    {
        if (!regressor.GetDeviceHandle())
            throw std::invalid_argument("acquisition_func: log noisy expected improvement needs a device-resident regressor "
                                        "(GaussianProcessRegressor / PreferenceRegressor); there is no host fallback");
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        const VectorXd incumbents = draws.MaxOverPoints(regressor.GetLargeX());
        return draws.MaximizeLogNoisyExpectedImprovement(num_points, incumbents, starts, num_local_search_iters, value, tau_relu, tau_max);
    }

    std::vector<VectorXd> acquisition_func::FindNextPointsByLogNoisyExpectedImprovement(
        const Regressor& regressor, const int num_points, const unsigned num_draws, const unsigned num_global_search_iters,
        const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies, double* value,
        const double tau_relu, const double tau_max)
    {
        if (num_points < 1 || num_points > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextPointsByLogNoisyExpectedImprovement: 1 .. 16 points");
        return FindNextPointsByLogNoisyExpectedImprovementFromStarts(
            regressor, num_points, SeededStarts(num_points * regressor.GetNumDims(), std::max(1u, num_global_search_iters), seed),
            num_draws, num_local_search_iters, seed, num_frequencies, value, tau_relu, tau_max);
    }
    // ---- the next slider by the expected utility of its best position (include/sls_hip.h sls_line_*) ----
    std::pair<VectorXd, VectorXd> acquisition_func::FindNextSliderByExpectedUtilityFromStarts(
        const Regressor& regressor, const VectorXd& anchor, const MatrixXd& starts, const int num_positions, const unsigned num_draws,
        const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (anchor.size() != 0 && anchor.size() != static_cast<long>(regressor.GetNumDims()))
            throw std::invalid_argument("FindNextSliderByExpectedUtilityFromStarts: the anchor must be empty or hold D values");
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        return draws.MaximizeExpectedUtilityOfBestSliderPosition(num_positions, starts, num_local_search_iters,
                                                                 anchor.size() != 0 ? &anchor : nullptr, nullptr, value);
    }

    std::pair<VectorXd, VectorXd> acquisition_func::FindNextSliderByExpectedUtility(
        const Regressor& regressor, const VectorXd& anchor, const int num_positions, const unsigned num_draws,
        const unsigned num_global_search_iters, const unsigned num_local_search_iters, const unsigned long long seed,
        const int num_frequencies, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (num_positions < SLS_LINE_MIN_POSITIONS || num_positions > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextSliderByExpectedUtility: 2 .. 16 positions");
        const unsigned nvar = (anchor.size() != 0 ? 1u : 2u) * regressor.GetNumDims();
        return FindNextSliderByExpectedUtilityFromStarts(regressor, anchor, SeededStarts(nvar, std::max(1u, num_global_search_iters), seed),
                                                         num_positions, num_draws, num_local_search_iters, seed, num_frequencies, value);
    }

    // ---- the next gallery by the expected utility of its best cell (include/sls_hip.h sls_patch_*) ----
    std::vector<VectorXd> acquisition_func::FindNextGalleryByExpectedUtilityFromStarts(
        const Regressor& regressor, const VectorXd& anchor, const MatrixXd& starts, const int grid_s, const int grid_t,
        const unsigned num_draws, const unsigned num_local_search_iters, const unsigned long long seed, const int num_frequencies,
        double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (anchor.size() != 0 && anchor.size() != static_cast<long>(regressor.GetNumDims()))
            throw std::invalid_argument("FindNextGalleryByExpectedUtilityFromStarts: the anchor must be empty or hold D values");
        const PosteriorFunctionSamples draws =
            regressor.SamplePosteriorFunctions(static_cast<int>(std::max(1u, num_draws)), seed, num_frequencies);
        return draws.MaximizeExpectedUtilityOfBestGalleryCell(grid_s, grid_t, starts, num_local_search_iters,
                                                              anchor.size() != 0 ? &anchor : nullptr, nullptr, value);
    }

    std::vector<VectorXd> acquisition_func::FindNextGalleryByExpectedUtility(
        const Regressor& regressor, const VectorXd& anchor, const int grid_s, const int grid_t, const unsigned num_draws,
        const unsigned num_global_search_iters, const unsigned num_local_search_iters, const unsigned long long seed,
        const int num_frequencies, double* value)
    {
        RequireDeviceHandleForExpectedUtility(regressor);
        if (grid_s < SLS_PATCH_MIN_POSITIONS || grid_t < SLS_PATCH_MIN_POSITIONS || grid_s > SLS_QEUBO_MAX_OPTIONS ||
            grid_t > SLS_QEUBO_MAX_OPTIONS || grid_s * grid_t > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument("FindNextGalleryByExpectedUtility: a grid of at least 2 positions per axis and at most 16 cells");
        const unsigned nvar = (anchor.size() != 0 ? 3u : 4u) * regressor.GetNumDims();
        return FindNextGalleryByExpectedUtilityFromStarts(regressor, anchor, SeededStarts(nvar, std::max(1u, num_global_search_iters), seed),
                                                          grid_s, grid_t, num_draws, num_local_search_iters, seed, num_frequencies, value);
    }

    MatrixXd acquisition_func::SeededUniformStarts(const unsigned num_dims, const long count, const unsigned long long seed)
    {
        return SeededStarts(num_dims, count, seed);
    }

    // ---- search restricted to affine subspaces (include/sls_hip.h sls_acq_*_sub, sls_path_*_sub) ----
    namespace
    {
        void RequireInCube(const char* who, const VectorXd& v)
        {
            for (long i = 0; i < v.size(); ++i)
                if (!(v(i) >= 0.0 && v(i) <= 1.0)) throw std::invalid_argument(std::string(who) + ": a coordinate lies outside [0,1]");
        }

        // sls_submaps over subspaces of one shape: the blocks A_k (D x d, column-major: MatrixXd's own layout) and c_k one behind the other
        struct PackedSubspaces
        {
            std::vector<double> A, c;
            sls_submaps         maps;
        };
        void Pack(const char* who, const std::vector<SearchSubspace>& subspaces, long num_dims, const int* subspace_of_start,
                  PackedSubspaces& p)
        {
            if (subspaces.empty()) throw std::invalid_argument(std::string(who) + ": no subspace");
            const long D = subspaces[0].basis.rows(), d = subspaces[0].basis.cols();
            if (D != num_dims || d < 1 || d > D)
                throw std::invalid_argument(std::string(who) + ": the basis must be D x d with 1 <= d <= D, D the regressor's dimensionality");
            for (const SearchSubspace& s : subspaces)
            {
                if (s.basis.rows() != D || s.basis.cols() != d || s.offset.size() != D)
                    throw std::invalid_argument(std::string(who) + ": every subspace needs a D x d basis and an offset of D values");
                p.A.insert(p.A.end(), s.basis.data(), s.basis.data() + D * d);
                p.c.insert(p.c.end(), s.offset.data(), s.offset.data() + D);
            }
            p.maps.struct_size   = static_cast<int>(sizeof(sls_submaps));
            p.maps.d             = static_cast<int>(d);
            p.maps.n_maps        = static_cast<int>(subspaces.size());
            p.maps.A             = p.A.data();
            p.maps.c             = p.c.data();
            p.maps.map_of_column = subspace_of_start;
        }
    } // namespace

    SearchSubspace SearchSubspace::Box(const VectorXd& lower, const VectorXd& upper)
    {
        const long D = lower.size();
        if (D < 1 || upper.size() != D) throw std::invalid_argument("SearchSubspace::Box: lower and upper must hold D >= 1 values each");
        for (long r = 0; r < D; ++r)
            if (!(0.0 <= lower(r) && lower(r) <= upper(r) && upper(r) <= 1.0))
                throw std::invalid_argument("SearchSubspace::Box: need 0 <= lower <= upper <= 1 in every coordinate");
        SearchSubspace s;
        s.offset = lower;
        s.basis  = MatrixXd::Zero(D, D);
        for (long r = 0; r < D; ++r) s.basis(r, r) = upper(r) - lower(r);
        return s;
    }

    SearchSubspace SearchSubspace::Segment(const VectorXd& a, const VectorXd& b)
    {
        const long D = a.size();
        if (D < 1 || b.size() != D) throw std::invalid_argument("SearchSubspace::Segment: the ends must hold D >= 1 values each");
        RequireInCube("SearchSubspace::Segment", a);
        RequireInCube("SearchSubspace::Segment", b);
        SearchSubspace s;
        s.offset = a;
        s.basis  = MatrixXd(D, 1);
        for (long r = 0; r < D; ++r) s.basis(r, 0) = b(r) - a(r);
        return s;
    }

    SearchSubspace SearchSubspace::Centered(const VectorXd& center, const MatrixXd& directions)
    {
        const long D = center.size(), d = directions.cols();
        if (D < 1 || directions.rows() != D || d < 1 || d > D)
            throw std::invalid_argument("SearchSubspace::Centered: directions must be D x d with 1 <= d <= D");
        RequireInCube("SearchSubspace::Centered", center);
        SearchSubspace s;
        s.offset = VectorXd(D);
        s.basis  = directions;
        for (long r = 0; r < D; ++r)
        {
            double half = 0.0;
            for (long j = 0; j < d; ++j)
            {
                if (!std::isfinite(directions(r, j))) throw std::invalid_argument("SearchSubspace::Centered: a direction is not finite");
                half += 0.5 * std::fabs(directions(r, j));
            }
            const double room = std::min(center(r), 1.0 - center(r));
            if (half > room)
                for (long j = 0; j < d; ++j) s.basis(r, j) *= room / half;
            double sum = 0.0;
            for (long j = 0; j < d; ++j) sum += s.basis(r, j);
            s.offset(r) = center(r) - 0.5 * sum;
        }
        return s;
    }

    VectorXd SearchSubspace::Point(const VectorXd& z) const
    {
        if (z.size() != basis.cols() || offset.size() != basis.rows())
            throw std::invalid_argument("SearchSubspace::Point: z must hold d values (basis D x d, offset D)");
        VectorXd x = offset;
        for (long j = 0; j < basis.cols(); ++j)
            for (long r = 0; r < basis.rows(); ++r)
            {
                const volatile double product = basis(r, j) * z(j);   // rounded before it is added, as on the device
                x(r) = x(r) + product;
            }
        return x;
    }

    VectorXd acquisition_func::CalcAcquisitionValuesInSubspace(const Regressor& regressor, const SearchSubspace& subspace, const MatrixXd& Z,
                                                               const AcquisitionFuncType func_type, const double hyperparam,
                                                               MatrixXd* grad_z)
    {
        sls_gp*         h = RequireHandle(regressor);
        PackedSubspaces p;
        Pack("CalcAcquisitionValuesInSubspace", {subspace}, regressor.GetNumDims(), nullptr, p);
        if (Z.rows() != p.maps.d) throw std::invalid_argument("CalcAcquisitionValuesInSubspace: Z must be d x M");
        const long M = Z.cols();
        VectorXd   v = VectorXd::Zero(M);
        if (grad_z) *grad_z = MatrixXd::Zero(Z.rows(), M);
        device::Check(sls_acq_eval_sub(h, AcqId(func_type), hyperparam, &p.maps, Z.data(), static_cast<int>(M), v.data(),
                                       grad_z ? grad_z->data() : nullptr, nullptr),
                      "sls_acq_eval_sub");
        return v;
    }

    VectorXd acquisition_func::FindNextPointInSubspacesFromStarts(const Regressor& regressor, const std::vector<SearchSubspace>& subspaces,
                                                                  const std::vector<int>& subspace_of_start, const MatrixXd& starts_z,
                                                                  const unsigned num_local_search_iters, const AcquisitionFuncType func_type,
                                                                  const double hyperparam, double* value, int* winner_subspace)
    {
        sls_gp*         h = RequireHandle(regressor);
        PackedSubspaces p;
        const long      S = starts_z.cols();
        if (!subspace_of_start.empty() && static_cast<long>(subspace_of_start.size()) != S)
            throw std::invalid_argument("FindNextPointInSubspacesFromStarts: subspace_of_start must be empty or hold one entry per start");
        Pack("FindNextPointInSubspacesFromStarts", subspaces, regressor.GetNumDims(), subspace_of_start.empty() ? nullptr : subspace_of_start.data(), p);
        if (starts_z.rows() != p.maps.d || S < 1) throw std::invalid_argument("FindNextPointInSubspacesFromStarts: starts_z must be d x S, S >= 1");
        VectorXd             x(regressor.GetNumDims());
        double               v     = 0.0;
        long                 idx   = 0;
        const sls_lbfgs_opts lopts = LocalSearchOpts();   // GetLocalSearchTolerances
        device::Check(sls_acq_maximize_sub(h, AcqId(func_type), hyperparam, &p.maps, starts_z.data(), static_cast<int>(S),
                                           std::max(1, static_cast<int>(num_local_search_iters)), &lopts, 0, nullptr, x.data(), &v, &idx,
                                           nullptr, nullptr, nullptr),
                      "sls_acq_maximize_sub");
        if (value) *value = v;
        if (winner_subspace) *winner_subspace = subspace_of_start.empty() ? 0 : subspace_of_start[static_cast<size_t>(idx)];
        return x;
    }

    VectorXd acquisition_func::FindNextPointInSubspace(const Regressor& regressor, const SearchSubspace& subspace,
                                                       const unsigned num_global_search_iters, const unsigned num_local_search_iters,
                                                       const AcquisitionFuncType func_type, const double hyperparam,
                                                       const unsigned long long seed, double* value)
    {
        RequireHandle(regressor);
        const MatrixXd starts = SeededStarts(static_cast<unsigned>(std::max<long>(1, subspace.basis.cols())), std::max(1u, num_global_search_iters), seed);
        return FindNextPointInSubspacesFromStarts(regressor, {subspace}, {}, starts, num_local_search_iters, func_type, hyperparam, value);
    }

    VectorXd acquisition_func::FindNextPointInBox(const Regressor& regressor, const VectorXd& lower, const VectorXd& upper,
                                                  const unsigned num_global_search_iters, const unsigned num_local_search_iters,
                                                  const AcquisitionFuncType func_type, const double hyperparam, const unsigned long long seed,
                                                  double* value)
    {
        return FindNextPointInSubspace(regressor, SearchSubspace::Box(lower, upper), num_global_search_iters, num_local_search_iters,
                                       func_type, hyperparam, seed, value);
    }

    std::vector<VectorXd> acquisition_func::FindNextPointsByThompsonSamplingInBox(const Regressor& regressor, const unsigned num_points,
                                                                                  const VectorXd& lower, const VectorXd& upper,
                                                                                  const unsigned num_global_search_iters,
                                                                                  const unsigned num_local_search_iters,
                                                                                  const unsigned long long seed, const int num_frequencies)
    {
        if (num_points == 0) return {};
        RequireHandle(regressor);
        const SearchSubspace box = SearchSubspace::Box(lower, upper);
        const unsigned       S   = std::max(1u, num_global_search_iters);
        const PosteriorFunctionSamples draws = regressor.SamplePosteriorFunctions(static_cast<int>(num_points), seed, num_frequencies);
        return draws.MaximizeInSubspace(box, SeededStarts(regressor.GetNumDims(), static_cast<long>(num_points) * S, seed),
                                        num_local_search_iters);
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeInSubspace(const SearchSubspace& subspace, const MatrixXd& starts_z,
                                                                       unsigned num_local_search_iters, VectorXd* values) const
    {
        const long T = starts_z.cols();
        if (T < m_num_draws || T % m_num_draws != 0)
            throw std::invalid_argument("PosteriorFunctionSamples::MaximizeInSubspace: the start count must be a positive multiple of the draw count");
        PackedSubspaces p;
        Pack("PosteriorFunctionSamples::MaximizeInSubspace", {subspace}, m_num_dims, nullptr, p);
        if (starts_z.rows() != p.maps.d) throw std::invalid_argument("PosteriorFunctionSamples::MaximizeInSubspace: starts_z must be d x (num_draws S)");
        const sls_lbfgs_opts o = LocalSearchOpts();   // the acquisition maximiser's local search tolerances
        MatrixXd             X(m_num_dims, m_num_draws);
        VectorXd             v(m_num_draws);
        device::Check(sls_path_maximize_sub(m_path, &p.maps, starts_z.data(), static_cast<int>(T / m_num_draws),
                                            std::max(1, static_cast<int>(num_local_search_iters)), &o, nullptr, X.data(), v.data(), nullptr),
                      "sls_path_maximize_sub");
        if (values) *values = v;
        std::vector<VectorXd> out;
        for (int s = 0; s < m_num_draws; ++s) out.push_back(X.col(s));
        return out;
    }
} // namespace sequential_line_search
