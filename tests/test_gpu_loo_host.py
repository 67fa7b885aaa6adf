"""Leave-one-out cross-validation through the C++ host layer and the pybind11 module: GaussianProcessRegressor::
CalcLeaveOneOutPredictions against the ctypes path to the bit, and the estimating constructor with HyperparamCriterion::LeaveOneOut
(DIRECT(300), the prior medians, then the bounded L-BFGS in log-parameters on sls_gp_loo_grad) against scipy's L-BFGS-B on
tests/loo_ref.py's objective, under the tolerances of tests/test_gpu_map_fit.py.  A small C++ program built against
libsequential-line-search.so does the host side.

scipy runs from two starts: the prior medians (one of the two candidates the fit starts its local phase from; DIRECT's point is not
reported by the host layer) and the fit's own result, from where it can only climb: the fit must reach the better of the two.

The program runs once for the Matern kernel at (3, 40) with everything above, and once each for the fit alone under the other kernel
(squared exponential, (3, 40)) and beyond one tile (Matern, (2, 130): every objective call of the fit goes through the tiled
pipeline's second row and column tile), on data of the same construction.  On the CPU, scipy's L-BFGS-B on loo_ref's objective from
the prior medians and from four starts a unit normal away in log-parameters ends at one optimum for (2, 130) (413.83226286, cond(K_y)
3.9e5 there); for the squared exponential at (3, 40) the prior medians lead to the best optimum found (117.28978776; two of the four
other starts end lower, at 106.16 and 114.63).  Both are the optima the fit reaches on the device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import loo_ref
from util import sls, synth_clustered_ard_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, KERNEL = 3, 40, 1
FIT_CASES = {"squared_exponential_3_40": (0, 3, 40), "matern_2_130": (1, 2, 130)}
KERNEL_NAMES = {0: "ArdSquaredExponentialKernel", 1: "ArdMatern52Kernel"}
LOG_LO, LOG_HI = math.log(1e-8), math.log(50.0)

PROGRAM = r"""
#include <cstdio>
#include <sequential-line-search/gaussian-process-regressor.hpp>
using namespace sequential_line_search;
using Eigen::MatrixXd;
using Eigen::VectorXd;

static void print_vec(const char* what, const VectorXd& v) {
    std::printf("%s", what);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static void print_fit(const char* what, const GaussianProcessRegressor& gp) {
    const auto& s = gp.GetMapFitStats();
    std::printf("%s %.17g %.17g", what, gp.GetKernelHyperparams()(0), gp.GetNoiseHyperparam());
    for (long d = 1; d < gp.GetKernelHyperparams().size(); ++d) std::printf(" %.17g", gp.GetKernelHyperparams()(d));
    std::printf("\n%s_stats %.17g %.17g %.17g %d %d\n", what, s.final_value, s.direct_value, s.prior_value, s.evals_direct, s.evals_local);
}

int main() {
    const int D = @D@, N = @N@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double thd[] = {@theta@};
    MatrixXd X(D, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < D; ++i) X(i, j) = Xd[i + j * D];
    VectorXd y(N), theta(D + 1);
    for (int i = 0; i < N; ++i) y(i) = yd[i];
    for (int i = 0; i <= D; ++i) theta(i) = thd[i];
    GaussianProcessRegressor::s_materialize_matrices.store(false);
    {
        GaussianProcessRegressor gp(X, y, theta, 0.005, KernelType::@KERNEL@);
        VectorXd mu, var, logp;
        gp.CalcLeaveOneOutPredictions(mu, var, logp);
        print_vec("fixed_mu", mu);
        print_vec("fixed_var", var);
        print_vec("fixed_logp", logp);
    }
#if @ML@
    GaussianProcessRegressor ml(X, y, KernelType::@KERNEL@);
    print_fit("ml", ml);
    GaussianProcessRegressor ml2(X, y, KernelType::@KERNEL@, HyperparamCriterion::MarginalLikelihood);
    print_fit("ml_explicit", ml2);
#endif
    GaussianProcessRegressor loo(X, y, KernelType::@KERNEL@, HyperparamCriterion::LeaveOneOut);
    print_fit("loo", loo);
    VectorXd mu, var, logp;
    loo.CalcLeaveOneOutPredictions(mu, var, logp);
    print_vec("loo_mu", mu);
    print_vec("loo_var", var);
    print_vec("loo_logp", logp);
    return 0;
}
"""


@pytest.fixture(scope="module")
def data(oracle):
    X, y, _ = synth_clustered_ard_problem(oracle, D, N)
    return np.asfortranarray(X), y, np.array([0.5, 0.3, 0.4, 0.5])


def c_list(a):
    return ", ".join(repr(float(v)) for v in np.asarray(a).ravel(order="F"))


def run_program(tmp, kernel, X, y, theta, ml):
    """Builds and runs the host program for one kernel and data set (ml: with the two marginal-likelihood fits)."""
    text = PROGRAM
    for key, value in dict(D=X.shape[0], N=X.shape[1], X=c_list(X), y=c_list(y), theta=c_list(theta), KERNEL=KERNEL_NAMES[kernel],
                           ML=int(ml)).items():
        text = text.replace(f"@{key}@", str(value))
    src, exe = tmp / "loo_host.cpp", tmp / "loo_host"
    src.write_text(text)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}


@pytest.fixture(scope="module")
def program_output(data, tmp_path_factory):
    X, y, theta = data
    return run_program(tmp_path_factory.mktemp("loo_host"), KERNEL, X, y, theta, True)


@pytest.fixture(scope="module", params=sorted(FIT_CASES))
def fit_case(request, oracle, tmp_path_factory):
    """(kernel, X, y, theta, program output) of one further fit: a program run of its own, the LOO fit alone."""
    kernel, d, n = FIT_CASES[request.param]
    X, y, _ = synth_clustered_ard_problem(oracle, d, n)
    X, theta = np.asfortranarray(X), np.concatenate([[0.5], np.linspace(0.3, 0.5, d)])
    return kernel, X, y, theta, run_program(tmp_path_factory.mktemp("loo_host_" + request.param), kernel, X, y, theta, False)


def check_predictions_equal_the_ctypes_path(res, kernel, X, y, theta):
    m = sls()
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.005, kernel)
    mu, var, logp = gp.loo()
    gp.close()
    ctx.close()
    assert np.array_equal(res["fixed_mu"], mu) and np.array_equal(res["fixed_var"], var) and np.array_equal(res["fixed_logp"], logp)


def test_predictions_equal_the_ctypes_path(program_output, data):
    X, y, theta = data
    check_predictions_equal_the_ctypes_path(program_output, KERNEL, X, y, theta)


def test_default_criterion_is_the_marginal_likelihood(program_output):
    res = program_output
    assert np.array_equal(res["ml"], res["ml_explicit"]) and np.array_equal(res["ml_stats"], res["ml_explicit_stats"])
    assert not np.array_equal(res["ml"], res["loo"])


def neg_objective_log(z, kernel, X, y):
    x = np.exp(z)
    v, g = loo_ref.gp_loo_objective(kernel, X, y, x)
    return -v, -(g * x)


def check_loo_fit_reaches_scipys_optimum(res, kernel, X, y):
    from scipy.optimize import minimize
    dims = X.shape[0]
    x = res["loo"]
    final, direct, prior = res["loo_stats"][:3]
    f_np, g_np = loo_ref.gp_loo_objective(kernel, X, y, x)
    z = np.log(x)
    bounds = [(LOG_LO, LOG_HI)] * (dims + 2)
    z_prior = np.log(np.array([0.5, 1e-4] + [0.5] * dims))
    best = -np.inf
    for z0 in (z_prior, z):
        r = minimize(neg_objective_log, z0, args=(kernel, X, y), jac=True, method="L-BFGS-B", bounds=bounds,
                     options=dict(maxiter=2000, ftol=1e-15, gtol=1e-10))
        best = max(best, -r.fun)
    scale = max(1.0, abs(best))
    print("device", final, "numpy at the result", f_np, "direct", direct, "prior", prior, "scipy", best)
    assert abs(final - f_np) <= 1e-9 * scale, (final, f_np)
    assert final >= direct - 1e-9 * scale and final >= prior - 1e-9 * scale
    gz = g_np * x
    gz[(z <= LOG_LO + 1e-12) & (gz < 0)] = 0.0
    gz[(z >= LOG_HI - 1e-12) & (gz > 0)] = 0.0
    assert np.max(np.abs(gz)) <= 1e-4 * scale, np.max(np.abs(gz))
    assert f_np >= best - 1e-6 * scale, (f_np, best)
    assert 1 <= res["loo_stats"][3] <= 300 and 1 <= res["loo_stats"][4] <= 1000
    # the fitted object's predictions are those of its hyper-parameters
    mu, var, logp, L = loo_ref.loo_terms(kernel, X, y, np.concatenate([[x[0]], x[2:]]), x[1])
    np.testing.assert_allclose(res["loo_mu"], mu, rtol=1e-7, atol=1e-9 * max(np.abs(mu).max(), np.abs(y).max()))
    np.testing.assert_allclose(res["loo_var"], var, rtol=1e-7)
    np.testing.assert_allclose(res["loo_logp"], logp, rtol=1e-7, atol=1e-9 * np.abs(logp).max())


def test_loo_fit_reaches_scipys_optimum(program_output, data):
    X, y, _ = data
    check_loo_fit_reaches_scipys_optimum(program_output, KERNEL, X, y)


def test_further_fits_reach_scipys_optimum(fit_case):
    """The other kernel, and a fit whose every objective call runs the tiled pipeline beyond one tile: the same comparison, the same
    tolerances."""
    kernel, X, y, theta, res = fit_case
    check_predictions_equal_the_ctypes_path(res, kernel, X, y, theta)
    check_loo_fit_reaches_scipys_optimum(res, kernel, X, y)


def test_python_module(program_output, data):
    X, y, theta = data
    res = program_output
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.005, pysls.KernelType.ArdMatern52Kernel)
    mu, var, logp = reg.leave_one_out()
    assert np.array_equal(mu, res["fixed_mu"]) and np.array_equal(var, res["fixed_var"]) and np.array_equal(logp, res["fixed_logp"])
    fit = pysls.GaussianProcessRegressor(X, y, pysls.KernelType.ArdMatern52Kernel, criterion=pysls.HyperparamCriterion.LeaveOneOut)
    got = np.concatenate([[fit.kernel_hyperparams()[0], fit.noise_hyperparam()], fit.kernel_hyperparams()[1:]])
    assert np.array_equal(got, res["loo"])
    ml = pysls.GaussianProcessRegressor(X, y, pysls.KernelType.ArdMatern52Kernel)
    got = np.concatenate([[ml.kernel_hyperparams()[0], ml.noise_hyperparam()], ml.kernel_hyperparams()[1:]])
    assert np.array_equal(got, res["ml"])
