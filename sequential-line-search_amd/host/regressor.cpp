// Regressor base + Gram builders over the C ABI (reference: src/regressor.cpp).
#include <algorithm>
#include <cmath>
#include <sequential-line-search/regressor.hpp>
#include <stdexcept>
#include <string>

#include "device.hpp"

using Eigen::MatrixXd;
using Eigen::VectorXd;

namespace sequential_line_search
{
    namespace
    {
        double ScaledSquaredDistance(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            double q = 0.0;
            for (long i = 0; i < xa.size(); ++i)
            {
                const double d = (xa(i) - xb(i)) / theta(1 + i);
                q += d * d;
            }
            return q;
        }
        int KernelId(KernelType t) { return t == KernelType::ArdSquaredExponentialKernel ? SLS_KERNEL_ARD_SQUARED_EXPONENTIAL : SLS_KERNEL_ARD_MATERN52; }
    } // namespace

    // mathtoolbox kernel functions; scalar host forms for API compatibility only
    namespace kernels
    {
        double ArdSquaredExp(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            return theta(0) * std::exp(-0.5 * ScaledSquaredDistance(xa, xb, theta));
        }
        VectorXd ArdSquaredExpThetaDerivative(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            const double e = std::exp(-0.5 * ScaledSquaredDistance(xa, xb, theta));
            VectorXd     g(theta.size());
            g(0) = e;
            for (long i = 0; i < xa.size(); ++i)
            {
                const double d = xa(i) - xb(i), l = theta(1 + i);
                g(1 + i)       = theta(0) * e * d * d / (l * l * l);
            }
            return g;
        }
        VectorXd ArdSquaredExpFirstArgDerivative(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            const double k = ArdSquaredExp(xa, xb, theta);
            VectorXd     g(xa.size());
            for (long i = 0; i < xa.size(); ++i) g(i) = -k * (xa(i) - xb(i)) / (theta(1 + i) * theta(1 + i));
            return g;
        }
        double ArdMatern52(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            const double q = ScaledSquaredDistance(xa, xb, theta), s = std::sqrt(5.0 * q);
            return theta(0) * (1.0 + s + (5.0 / 3.0) * q) * std::exp(-s);
        }
        VectorXd ArdMatern52ThetaDerivative(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            const double q = ScaledSquaredDistance(xa, xb, theta), s = std::sqrt(5.0 * q), e = std::exp(-s);
            const double c = theta(0) * (5.0 / 3.0) * (1.0 + s) * e;
            VectorXd     g(theta.size());
            g(0) = (1.0 + s + (5.0 / 3.0) * q) * e;
            for (long i = 0; i < xa.size(); ++i)
            {
                const double d = xa(i) - xb(i), l = theta(1 + i);
                g(1 + i)       = c * d * d / (l * l * l);
            }
            return g;
        }
        VectorXd ArdMatern52FirstArgDerivative(const VectorXd& xa, const VectorXd& xb, const VectorXd& theta)
        {
            const double q = ScaledSquaredDistance(xa, xb, theta), s = std::sqrt(5.0 * q);
            const double c = theta(0) * (5.0 / 3.0) * (1.0 + s) * std::exp(-s);
            VectorXd     g(xa.size());
            for (long i = 0; i < xa.size(); ++i) g(i) = -c * (xa(i) - xb(i)) / (theta(1 + i) * theta(1 + i));
            return g;
        }
        KernelType TypeOf(Kernel k)
        {
            if (k == ArdSquaredExp) return KernelType::ArdSquaredExponentialKernel;
            if (k == ArdMatern52) return KernelType::ArdMatern52Kernel;
            throw std::invalid_argument("sequential_line_search: unknown kernel function pointer (only the built-in ARD "
                                        "squared-exponential / Matern-5/2 kernels run on the device; no host fallback)");
        }
        KernelType TypeOf(KernelThetaDerivative k, int)
        {
            if (k == ArdSquaredExpThetaDerivative || k == ArdSquaredExpFirstArgDerivative) return KernelType::ArdSquaredExponentialKernel;
            if (k == ArdMatern52ThetaDerivative || k == ArdMatern52FirstArgDerivative) return KernelType::ArdMatern52Kernel;
            throw std::invalid_argument("sequential_line_search: unknown kernel derivative function pointer");
        }
    } // namespace kernels

    // reference: src/regressor.cpp:8-27
    Regressor::Regressor(const KernelType kernel_type) : m_kernel_type(kernel_type)
    {
        if (kernel_type == KernelType::ArdSquaredExponentialKernel)
        {
            m_kernel                      = kernels::ArdSquaredExp;
            m_kernel_theta_derivative     = kernels::ArdSquaredExpThetaDerivative;
            m_kernel_first_arg_derivative = kernels::ArdSquaredExpFirstArgDerivative;
        }
        else
        {
            m_kernel                      = kernels::ArdMatern52;
            m_kernel_theta_derivative     = kernels::ArdMatern52ThetaDerivative;
            m_kernel_first_arg_derivative = kernels::ArdMatern52FirstArgDerivative;
        }
    }

    // reference: src/regressor.cpp:29-43
    VectorXd Regressor::PredictMaximumPointFromData() const
    {
        const MatrixXd& X = GetLargeX();
        if (sls_gp* h = GetDeviceHandle())
        {
            int best = 0;
            device::Check(sls_gp_get_summary(h, &best, nullptr, nullptr), "sls_gp_get_summary");
            return eig::Col(X, best);
        }
        int    best = 0;
        double bv   = -INFINITY;
        for (long i = 0; i < X.cols(); ++i)
        {
            const double f = PredictMu(eig::Col(X, i));
            if (f > bv) { bv = f; best = static_cast<int>(i); }
        }
        return eig::Col(X, best);
    }

    void Regressor::PredictBatch(const MatrixXd& Xs, VectorXd& mu, VectorXd& sigma) const
    {
        const long M = Xs.cols();
        mu           = VectorXd(M);
        sigma        = VectorXd(M);
        if (sls_gp* h = GetDeviceHandle())
        {
            device::Check(sls_gp_predict(h, Xs.data(), static_cast<int>(M), mu.data(), sigma.data()), "sls_gp_predict");
            return;
        }
        for (long m = 0; m < M; ++m)
        {
            mu(m)    = PredictMu(eig::Col(Xs, m));
            sigma(m) = PredictSigma(eig::Col(Xs, m));
        }
    }

    MatrixXd Regressor::PredictCovariance(const MatrixXd& Xs) const
    {
        sls_gp* h = GetDeviceHandle();
        if (!h) return MatrixXd();
        const long M   = Xs.cols();
        MatrixXd   cov(M, M);
        device::Check(sls_gp_predict_cov(h, Xs.data(), static_cast<int>(M), nullptr, cov.data()), "sls_gp_predict_cov");
        return cov;
    }

    PosteriorFunctionSamples Regressor::SamplePosteriorFunctions(int num_draws, unsigned long long seed, int num_frequencies) const
    {
        sls_gp* h = GetDeviceHandle();
        if (!h)
            throw std::invalid_argument("Regressor::SamplePosteriorFunctions needs a device-resident regressor "
                                        "(GaussianProcessRegressor / PreferenceRegressor)");
        return PosteriorFunctionSamples(h, static_cast<int>(GetNumDims()), num_draws, seed, num_frequencies);
    }

    PosteriorFunctionSamples::PosteriorFunctionSamples(sls_gp* handle, int num_dims, int num_draws, unsigned long long seed,
                                                       int num_frequencies)
        : m_num_draws(num_draws), m_num_dims(num_dims)
    {
        device::Check(sls_path_create(handle, num_draws, num_frequencies, seed, &m_path), "sls_path_create");
    }
    PosteriorFunctionSamples::PosteriorFunctionSamples(PosteriorFunctionSamples&& o) noexcept
        : m_path(o.m_path), m_num_draws(o.m_num_draws), m_num_dims(o.m_num_dims)
    {
        o.m_path = nullptr;
    }
    PosteriorFunctionSamples& PosteriorFunctionSamples::operator=(PosteriorFunctionSamples&& o) noexcept
    {
        if (this != &o)
        {
            if (m_path) sls_path_destroy(m_path);
            m_path      = o.m_path;
            m_num_draws = o.m_num_draws;
            m_num_dims  = o.m_num_dims;
            o.m_path    = nullptr;
        }
        return *this;
    }
    PosteriorFunctionSamples::~PosteriorFunctionSamples()
    {
        if (m_path) sls_path_destroy(m_path);
    }

    MatrixXd PosteriorFunctionSamples::Evaluate(const MatrixXd& Xs) const
    {
        const long M = Xs.cols();
        MatrixXd   F(M, m_num_draws);
        device::Check(sls_path_eval(m_path, Xs.data(), static_cast<int>(M), nullptr, F.data(), nullptr), "sls_path_eval");
        return F;
    }

    VectorXd PosteriorFunctionSamples::EvaluateDerivative(const VectorXd& x, int draw) const
    {
        VectorXd g(x.size());
        double   v = 0.0;
        device::Check(sls_path_eval(m_path, x.data(), 1, &draw, &v, g.data()), "sls_path_eval");
        return g;
    }

    std::vector<VectorXd> PosteriorFunctionSamples::Maximize(const MatrixXd& starts, unsigned num_local_search_iters,
                                                             VectorXd* values) const
    {
        const long T = starts.cols();
        if (T < m_num_draws || T % m_num_draws != 0)
            throw std::invalid_argument("PosteriorFunctionSamples::Maximize: the start count must be a positive multiple of the draw count");
        sls_lbfgs_opts o;
        sls_lbfgs_default_opts(&o);
        optim::SearchTolerances(&o.ftol_rel, &o.xtol_rel);   // the acquisition maximiser's local search tolerances
        MatrixXd X(m_num_dims, m_num_draws);
        VectorXd v(m_num_draws);
        device::Check(sls_path_maximize(m_path, starts.data(), static_cast<int>(T / m_num_draws),
                                        std::max(1, static_cast<int>(num_local_search_iters)), &o, X.data(), v.data(), nullptr),
                      "sls_path_maximize");
        if (values) *values = v;
        std::vector<VectorXd> out;
        for (int s = 0; s < m_num_draws; ++s) out.push_back(X.col(s));
        return out;
    }

    VectorXd PosteriorFunctionSamples::CalcSetCriterion(const char* who, const std::vector<MatrixXd>& options, const VectorXd* baseline,
                                                        std::vector<MatrixXd>* grads, Eigen::MatrixXi* win_counts,
                                                        const double* taus, const double* scale, MatrixXd* probabilities) const
    {
        const std::string name = std::string("PosteriorFunctionSamples::") + who;
        const long        q    = static_cast<long>(options.size());
        if (q < 1 || q > SLS_QEUBO_MAX_OPTIONS) throw std::invalid_argument(name + ": 1 .. 16 options");
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long D = m_num_dims, M = options[0].cols();
        for (const MatrixXd& X : options)
            if (X.rows() != D || X.cols() != M) throw std::invalid_argument(name + ": every option block must be D x M");
        MatrixXd sets(q * D, M);
        for (long i = 0; i < q; ++i)
            for (long m = 0; m < M; ++m)
                for (long d = 0; d < D; ++d) sets(i * D + d, m) = options[i](d, m);
        VectorXd v = VectorXd::Zero(M);
        MatrixXd g(grads ? q * D : 0, grads ? M : 0);
        if (win_counts) *win_counts = Eigen::MatrixXi::Zero(q, M);
        double* gp = grads ? g.data() : nullptr;
        int*    wp = win_counts ? win_counts->data() : nullptr;
        if (probabilities) *probabilities = MatrixXd::Zero(q, M);
        if (scale)
            device::Check(sls_qbald_eval(m_path, static_cast<int>(q), *scale, sets.data(), static_cast<int>(M), v.data(), gp,
                                         probabilities ? probabilities->data() : nullptr, wp),
                          "sls_qbald_eval");
        else if (baseline && taus)
            device::Check(sls_qlognei_eval(m_path, static_cast<int>(q), baseline->data(), taus[0], taus[1], sets.data(),
                                           static_cast<int>(M), v.data(), gp, wp),
                          "sls_qlognei_eval");
        else if (baseline)
            device::Check(sls_qnei_eval(m_path, static_cast<int>(q), baseline->data(), sets.data(), static_cast<int>(M), v.data(), gp, wp),
                          "sls_qnei_eval");
        else
            device::Check(sls_qeubo_eval(m_path, static_cast<int>(q), sets.data(), static_cast<int>(M), v.data(), gp, wp), "sls_qeubo_eval");
        if (grads)
        {
            grads->assign(q, MatrixXd(D, M));
            for (long i = 0; i < q; ++i)
                for (long m = 0; m < M; ++m)
                    for (long d = 0; d < D; ++d) (*grads)[i](d, m) = g(i * D + d, m);
        }
        return v;
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeSetCriterion(const char* who, int num_options, const VectorXd* baseline,
                                                                         const MatrixXd& starts, unsigned num_local_search_iters,
                                                                         double* value, const double* taus,
                                                                         const double* scale) const
    {
        const std::string name = std::string("PosteriorFunctionSamples::") + who;
        if (num_options < 1 || num_options > SLS_QEUBO_MAX_OPTIONS) throw std::invalid_argument(name + ": 1 .. 16 options");
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long D = m_num_dims;
        if (starts.rows() != num_options * D || starts.cols() < 1)
            throw std::invalid_argument(name + ": starts must be (num_options D) x S with S >= 1");
        sls_lbfgs_opts o;
        sls_lbfgs_default_opts(&o);
        optim::SearchTolerances(&o.ftol_rel, &o.xtol_rel);   // the acquisition maximiser's local search tolerances
        VectorXd  x(num_options * D);
        double    v   = 0.0;
        long      idx = 0;
        const int S = static_cast<int>(starts.cols()), n_local = std::max(1, static_cast<int>(num_local_search_iters));
        if (scale)
            device::Check(sls_qbald_maximize(m_path, num_options, *scale, starts.data(), S, n_local, &o, 0, x.data(), &v, &idx, nullptr,
                                             nullptr),
                          "sls_qbald_maximize");
        else if (baseline && taus)
            device::Check(sls_qlognei_maximize(m_path, num_options, baseline->data(), taus[0], taus[1], starts.data(), S, n_local, &o, 0,
                                               x.data(), &v, &idx, nullptr, nullptr),
                          "sls_qlognei_maximize");
        else if (baseline)
            device::Check(sls_qnei_maximize(m_path, num_options, baseline->data(), starts.data(), S, n_local, &o, 0, x.data(), &v, &idx,
                                            nullptr, nullptr),
                          "sls_qnei_maximize");
        else
            device::Check(sls_qeubo_maximize(m_path, num_options, starts.data(), S, n_local, &o, 0, x.data(), &v, &idx, nullptr, nullptr),
                          "sls_qeubo_maximize");
        if (value) *value = v;
        std::vector<VectorXd> out;
        for (int i = 0; i < num_options; ++i) out.push_back(x.segment(i * D, D));
        return out;
    }

    VectorXd PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestOption(const std::vector<MatrixXd>& options, std::vector<MatrixXd>* grads,
                                                                         Eigen::MatrixXi* win_counts) const
    {
        return CalcSetCriterion("CalcExpectedUtilitiesOfBestOption", options, nullptr, grads, win_counts);
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeExpectedUtilityOfBestOption(int num_options, const MatrixXd& starts,
                                                                                        unsigned num_local_search_iters, double* value) const
    {
        return MaximizeSetCriterion("MaximizeExpectedUtilityOfBestOption", num_options, nullptr, starts, num_local_search_iters, value);
    }

    VectorXd PosteriorFunctionSamples::MaxOverPoints(const MatrixXd& Xb, Eigen::VectorXi* arg) const
    {
        if (Xb.rows() != m_num_dims || Xb.cols() < 1)
            throw std::invalid_argument("PosteriorFunctionSamples::MaxOverPoints: Xb must be D x Mb with Mb >= 1");
        VectorXd t = VectorXd::Zero(m_num_draws);
        if (arg) *arg = Eigen::VectorXi(m_num_draws);
        device::Check(sls_path_max_over_points(m_path, Xb.data(), static_cast<int>(Xb.cols()), t.data(), arg ? arg->data() : nullptr),
                      "sls_path_max_over_points");
        return t;
    }

    VectorXd PosteriorFunctionSamples::CalcNoisyExpectedImprovements(const std::vector<MatrixXd>& options, const VectorXd& baseline,
                                                                     std::vector<MatrixXd>* grads, Eigen::MatrixXi* win_counts) const
    {
        return CalcSetCriterion("CalcNoisyExpectedImprovements", options, &baseline, grads, win_counts);
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeNoisyExpectedImprovement(int num_points, const VectorXd& baseline,
                                                                                     const MatrixXd& starts,
                                                                                     unsigned num_local_search_iters, double* value) const
    {
        return MaximizeSetCriterion("MaximizeNoisyExpectedImprovement", num_points, &baseline, starts, num_local_search_iters, value);
    }

    VectorXd PosteriorFunctionSamples::CalcLogNoisyExpectedImprovements(const std::vector<MatrixXd>& options, const VectorXd& baseline,
                                                                        std::vector<MatrixXd>* grads, Eigen::MatrixXi* win_counts,
                                                                        double tau_relu, double tau_max) const
    {
        const double taus[2] = {tau_relu, tau_max};
        return CalcSetCriterion("CalcLogNoisyExpectedImprovements", options, &baseline, grads, win_counts, taus);
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeLogNoisyExpectedImprovement(int num_points, const VectorXd& baseline,
                                                                                        const MatrixXd& starts,
                                                                                        unsigned num_local_search_iters, double* value,
                                                                                        double tau_relu, double tau_max) const
    {
        const double taus[2] = {tau_relu, tau_max};
        return MaximizeSetCriterion("MaximizeLogNoisyExpectedImprovement", num_points, &baseline, starts, num_local_search_iters, value,
                                    taus);
    }

    VectorXd PosteriorFunctionSamples::CalcChoiceInformationGains(const std::vector<MatrixXd>& options, double scale,
                                                                  std::vector<MatrixXd>* grads, MatrixXd* probabilities,
                                                                  Eigen::MatrixXi* win_counts) const
    {
        return CalcSetCriterion("CalcChoiceInformationGains", options, nullptr, grads, win_counts, nullptr, &scale, probabilities);
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeChoiceInformationGain(int num_options, double scale, const MatrixXd& starts,
                                                                                  unsigned num_local_search_iters, double* value) const
    {
        return MaximizeSetCriterion("MaximizeChoiceInformationGain", num_options, nullptr, starts, num_local_search_iters, value, nullptr,
                                    &scale);
    }

    VectorXd PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestSliderPosition(const MatrixXd& ends_a, const MatrixXd& ends_b,
                                                                                 int num_positions, MatrixXd* grad_a, MatrixXd* grad_b,
                                                                                 Eigen::MatrixXi* win_counts, const VectorXd* baseline) const
    {
        const std::string name = "PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestSliderPosition";
        if (num_positions < SLS_LINE_MIN_POSITIONS || num_positions > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument(name + ": 2 .. 16 positions");
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long D = m_num_dims, M = ends_a.cols();
        if (ends_a.rows() != D || ends_b.rows() != D || ends_b.cols() != M)
            throw std::invalid_argument(name + ": ends_a and ends_b must both be D x M");
        MatrixXd lines(2 * D, M);
        for (long m = 0; m < M; ++m)
            for (long d = 0; d < D; ++d)
            {
                lines(d, m)     = ends_a(d, m);
                lines(D + d, m) = ends_b(d, m);
            }
        VectorXd   v         = VectorXd::Zero(M);
        const bool want_grad = grad_a || grad_b;
        MatrixXd   g(want_grad ? 2 * D : 0, want_grad ? M : 0);
        if (win_counts) *win_counts = Eigen::MatrixXi::Zero(num_positions, M);
        device::Check(sls_line_eval(m_path, num_positions, baseline ? baseline->data() : nullptr, nullptr, lines.data(),
                                    static_cast<int>(M), v.data(), want_grad ? g.data() : nullptr,
                                    win_counts ? win_counts->data() : nullptr),
                      "sls_line_eval");
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

    std::pair<VectorXd, VectorXd> PosteriorFunctionSamples::MaximizeExpectedUtilityOfBestSliderPosition(
        int num_positions, const MatrixXd& starts, unsigned num_local_search_iters, const VectorXd* anchor, const VectorXd* baseline,
        double* value) const
    {
        const std::string name = "PosteriorFunctionSamples::MaximizeExpectedUtilityOfBestSliderPosition";
        if (num_positions < SLS_LINE_MIN_POSITIONS || num_positions > SLS_QEUBO_MAX_OPTIONS)
            throw std::invalid_argument(name + ": 2 .. 16 positions");
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long D = m_num_dims, nvar = anchor ? D : 2 * D;
        if (anchor && anchor->size() != D) throw std::invalid_argument(name + ": the anchor must hold D values");
        if (starts.rows() != nvar || starts.cols() < 1)
            throw std::invalid_argument(name + ": starts must be 2D x S (D x S with an anchor) with S >= 1");
        sls_lbfgs_opts o;
        sls_lbfgs_default_opts(&o);
        optim::SearchTolerances(&o.ftol_rel, &o.xtol_rel);   // the acquisition maximiser's local search tolerances
        VectorXd x(nvar);
        double   v   = 0.0;
        long     idx = 0;
        device::Check(sls_line_maximize(m_path, num_positions, baseline ? baseline->data() : nullptr, anchor ? anchor->data() : nullptr,
                                        starts.data(), static_cast<int>(starts.cols()),
                                        std::max(1, static_cast<int>(num_local_search_iters)), &o, 0, x.data(), &v, &idx, nullptr, nullptr),
                      "sls_line_maximize");
        if (value) *value = v;
        if (anchor) return std::make_pair(*anchor, x);
        return std::make_pair(VectorXd(x.segment(0, D)), VectorXd(x.segment(D, D)));
    }

    namespace
    {
        void RequireGalleryGrid(const std::string& name, int grid_s, int grid_t)
        {
            if (grid_s < SLS_PATCH_MIN_POSITIONS || grid_t < SLS_PATCH_MIN_POSITIONS || grid_s > SLS_QEUBO_MAX_OPTIONS ||
                grid_t > SLS_QEUBO_MAX_OPTIONS || grid_s * grid_t > SLS_QEUBO_MAX_OPTIONS)
                throw std::invalid_argument(name + ": a grid of at least 2 positions per axis and at most 16 cells");
        }
    } // namespace

    VectorXd PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestGalleryCell(const MatrixXd& corners00, const MatrixXd& corners10,
                                                                              const MatrixXd& corners01, const MatrixXd& corners11,
                                                                              int grid_s, int grid_t, std::vector<MatrixXd>* grads,
                                                                              Eigen::MatrixXi* win_counts, const VectorXd* baseline) const
    {
        const std::string name = "PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestGalleryCell";
        RequireGalleryGrid(name, grid_s, grid_t);
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long      D = m_num_dims, M = corners00.cols();
        const MatrixXd* corners[4] = {&corners00, &corners10, &corners01, &corners11};
        for (const MatrixXd* c : corners)
            if (c->rows() != D || c->cols() != M) throw std::invalid_argument(name + ": every corner block must be D x M");
        MatrixXd patches(4 * D, M);
        for (long c = 0; c < 4; ++c)
            for (long m = 0; m < M; ++m)
                for (long d = 0; d < D; ++d) patches(c * D + d, m) = (*corners[c])(d, m);
        VectorXd v = VectorXd::Zero(M);
        MatrixXd g(grads ? 4 * D : 0, grads ? M : 0);
        if (win_counts) *win_counts = Eigen::MatrixXi::Zero(grid_s * grid_t, M);
        device::Check(sls_patch_eval(m_path, grid_s, grid_t, baseline ? baseline->data() : nullptr, nullptr, patches.data(),
                                     static_cast<int>(M), v.data(), grads ? g.data() : nullptr,
                                     win_counts ? win_counts->data() : nullptr),
                      "sls_patch_eval");
        if (grads)
        {
            grads->assign(4, MatrixXd(D, M));
            for (long c = 0; c < 4; ++c)
                for (long m = 0; m < M; ++m)
                    for (long d = 0; d < D; ++d) (*grads)[c](d, m) = g(c * D + d, m);
        }
        return v;
    }

    std::vector<VectorXd> PosteriorFunctionSamples::MaximizeExpectedUtilityOfBestGalleryCell(int grid_s, int grid_t, const MatrixXd& starts,
                                                                                             unsigned        num_local_search_iters,
                                                                                             const VectorXd* anchor,
                                                                                             const VectorXd* baseline, double* value) const
    {
        const std::string name = "PosteriorFunctionSamples::MaximizeExpectedUtilityOfBestGalleryCell";
        RequireGalleryGrid(name, grid_s, grid_t);
        if (baseline && baseline->size() != m_num_draws) throw std::invalid_argument(name + ": the baseline must hold one value per draw");
        const long D = m_num_dims, nvar = (anchor ? 3 : 4) * D;
        if (anchor && anchor->size() != D) throw std::invalid_argument(name + ": the anchor must hold D values");
        if (starts.rows() != nvar || starts.cols() < 1)
            throw std::invalid_argument(name + ": starts must be 4D x S (3D x S with an anchor) with S >= 1");
        sls_lbfgs_opts o;
        sls_lbfgs_default_opts(&o);
        optim::SearchTolerances(&o.ftol_rel, &o.xtol_rel);   // the acquisition maximiser's local search tolerances
        VectorXd x(nvar);
        double   v   = 0.0;
        long     idx = 0;
        device::Check(sls_patch_maximize(m_path, grid_s, grid_t, baseline ? baseline->data() : nullptr, anchor ? anchor->data() : nullptr,
                                         starts.data(), static_cast<int>(starts.cols()),
                                         std::max(1, static_cast<int>(num_local_search_iters)), &o, 0, x.data(), &v, &idx, nullptr,
                                         nullptr),
                      "sls_patch_maximize");
        if (value) *value = v;
        std::vector<VectorXd> out;
        if (anchor) out.push_back(*anchor);
        for (long c = 0; c < (anchor ? 3 : 4); ++c) out.push_back(VectorXd(x.segment(c * D, D)));
        return out;
    }

    MatrixXd Regressor::SamplePosterior(const MatrixXd& Xs, int num_samples, unsigned long long seed, double* jitter_used) const
    {
        sls_gp* h = GetDeviceHandle();
        if (!h) return MatrixXd();
        const long M = Xs.cols();
        MatrixXd   F(M, num_samples);
        device::Check(sls_gp_sample_posterior(h, Xs.data(), static_cast<int>(M), num_samples, seed, F.data(), jitter_used),
                      "sls_gp_sample_posterior");
        return F;
    }

    // reference: src/regressor.cpp:45-59
    VectorXd CalcSmallK(const VectorXd& x, const MatrixXd& X, const VectorXd& theta, const Kernel kernel)
    {
        VectorXd k(X.cols());
        device::Check(sls_gram_cross(device::Context(), X.data(), static_cast<int>(X.rows()), static_cast<int>(X.cols()), x.data(), 1,
                                     theta.data(), KernelId(kernels::TypeOf(kernel)), k.data()),
                      "sls_gram_cross");
        return k;
    }

    // reference: src/regressor.cpp:61-71
    MatrixXd CalcLargeKY(const MatrixXd& X, const VectorXd& theta, const double noise_level, const Kernel kernel)
    {
        MatrixXd K(X.cols(), X.cols());
        device::Check(sls_gram(device::Context(), X.data(), static_cast<int>(X.rows()), static_cast<int>(X.cols()), theta.data(),
                               noise_level, KernelId(kernels::TypeOf(kernel)), K.data()),
                      "sls_gram");
        return K;
    }

    // reference: src/regressor.cpp:73-89
    MatrixXd CalcLargeKF(const MatrixXd& X, const VectorXd& theta, const Kernel kernel) { return CalcLargeKY(X, theta, 0.0, kernel); }

    // reference: src/regressor.cpp:91-108.  dk_i/dx = -c_i (x - x_i) / l^2 with the weights c from the device cross-Gram
    // (c = k for the squared-exponential kernel; for Matern the scalar form is evaluated per column).
    MatrixXd CalcSmallKSmallXDerivative(const VectorXd& x, const MatrixXd& X, const VectorXd& theta,
                                        const KernelFirstArgDerivative kernel_first_arg_derivative)
    {
        const KernelType t = kernels::TypeOf(kernel_first_arg_derivative, 0);
        MatrixXd         J(X.rows(), X.cols());
        if (t == KernelType::ArdSquaredExponentialKernel)
        {
            const VectorXd k = CalcSmallK(x, X, theta, kernels::ArdSquaredExp);
            for (long i = 0; i < X.cols(); ++i)
                for (long d = 0; d < X.rows(); ++d) J(d, i) = -k(i) * (x(d) - X(d, i)) / (theta(1 + d) * theta(1 + d));
        }
        else
        {
            for (long i = 0; i < X.cols(); ++i) eig::SetCol(J, i, kernel_first_arg_derivative(x, eig::Col(X, i), theta));
        }
        return J;
    }

    // reference: src/regressor.cpp:110-134 (API compatibility; the library's own MAP code never builds this tensor)
    std::vector<MatrixXd> CalcLargeKYThetaDerivative(const MatrixXd& X, const VectorXd& theta, const KernelThetaDerivative dk)
    {
        kernels::TypeOf(dk, 0);
        const long            N = X.cols();
        std::vector<MatrixXd> tensor(theta.size(), MatrixXd(N, N));
        for (long i = 0; i < N; ++i)
            for (long j = i; j < N; ++j)
            {
                const VectorXd g = dk(eig::Col(X, i), eig::Col(X, j), theta);
                for (long p = 0; p < theta.size(); ++p) tensor[p](i, j) = tensor[p](j, i) = g(p);
            }
        return tensor;
    }

    // reference: src/regressor.cpp:136-141
    MatrixXd CalcLargeKYNoiseLevelDerivative(const MatrixXd& X, const VectorXd&, const double) { return MatrixXd::Identity(X.cols(), X.cols()); }
} // namespace sequential_line_search
