"""The expected utility of the best option of a query pair through the C++ host layer and the pybind11 module:
acquisition_func::CalcExpectedUtilitiesOfBestOption and FindNextQueryPairByExpectedUtility[FromStarts] on a GaussianProcessRegressor
and a PreferenceRegressor (a small C++ program built against libsequential-line-search.so) against the ctypes path and the pybind11
functions on the same data, and PreferentialBayesianOptimizer.determine_next_query_by_expected_utility in a simulated-user loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M, S = 3, 25, 7, 48

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/preference-regressor.hpp>
using namespace sequential_line_search;

static void print_vec(const char* who, const char* what, const Eigen::VectorXd& v) {
    std::printf("%s_%s", who, what);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static Eigen::VectorXd flat(const Eigen::MatrixXd& A) {
    Eigen::VectorXd f(A.rows() * A.cols());
    for (long j = 0; j < A.cols(); ++j)
        for (long i = 0; i < A.rows(); ++i) f(i + j * A.rows()) = A(i, j);
    return f;
}
static Eigen::VectorXd pair_and_value(const std::pair<Eigen::VectorXd, Eigen::VectorXd>& q, double value) {
    const long d = q.first.size();
    Eigen::VectorXd out(2 * d + 1);
    for (long i = 0; i < d; ++i) { out(i) = q.first(i); out(d + i) = q.second(i); }
    out(2 * d) = value;
    return out;
}
static void run(const char* who, const Regressor& r, const Eigen::MatrixXd& Xa, const Eigen::MatrixXd& Xb, const Eigen::MatrixXd& starts) {
    Eigen::MatrixXd ga, gb;
    print_vec(who, "val", acquisition_func::CalcExpectedUtilitiesOfBestOption(r, Xa, Xb, &ga, &gb));
    print_vec(who, "ga", flat(ga));
    print_vec(who, "gb", flat(gb));
    print_vec(who, "valonly", acquisition_func::CalcExpectedUtilitiesOfBestOption(r, Xa, Xb));
    double value = 0.0;
    const auto q = acquisition_func::FindNextQueryPairByExpectedUtilityFromStarts(r, starts, 20, &value);
    print_vec(who, "fromstarts", pair_and_value(q, value));
    const unsigned long long seeds[3] = {7, 7, 8};
    const char* tags[3] = {"seed7a", "seed7b", "seed8"};
    for (int k = 0; k < 3; ++k) {
        const auto p = acquisition_func::FindNextQueryPairByExpectedUtility(r, 32, 20, seeds[k], &value);
        print_vec(who, tags[k], pair_and_value(p, value));
    }
}

int main() {
    const int D = @D@, N = @N@, M = @M@, S = @S@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double Pd[] = {@P@};
    static const double Sd[] = {@starts@};
    Eigen::MatrixXd X(D, N), Xa(D, M), Xb(D, M), starts(2 * D, S);
    Eigen::VectorXd y(N), theta(D + 1);
    for (int i = 0; i < N; ++i) { y(i) = yd[i]; for (int d = 0; d < D; ++d) X(d, i) = Xd[d + i * D]; }
    for (int i = 0; i < M; ++i) for (int d = 0; d < D; ++d) { Xa(d, i) = Pd[d + i * 2 * D]; Xb(d, i) = Pd[D + d + i * 2 * D]; }
    for (int i = 0; i < S; ++i) for (int d = 0; d < 2 * D; ++d) starts(d, i) = Sd[d + i * 2 * D];
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    run("gp", gp, Xa, Xb, starts);
    std::vector<Preference> prefs;
    for (int i = 0; i + 1 < N; i += 2) prefs.push_back(y(i) > y(i + 1) ? Preference(i, i + 1) : Preference(i + 1, i));
    PreferenceRegressor pr(X, prefs, false);
    run("pr", pr, Xa, Xb, starts);
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_pair_criterion_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    P = rng.uniform(0, 1, (2 * D, M))
    starts = rng.uniform(0, 1, (2 * D, S))
    src = tmp_path / "eubo.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, S=S, X=c_list(X), y=c_list(y), P=c_list(P), starts=c_list(starts)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "eubo"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    for who in ("gp", "pr"):                                  # the PreferenceRegressor's handle runs in sigma mode 1
        val = res[who + "_val"]
        assert val.shape == (M,) and np.all(np.isfinite(val)) and np.array_equal(res[who + "_valonly"], val)
        assert np.abs(res[who + "_ga"]).max() > 0 and np.abs(res[who + "_gb"]).max() > 0
        a, b, c = res[who + "_seed7a"], res[who + "_seed7b"], res[who + "_seed8"]
        assert np.array_equal(a, b)                                               # the same seed gives the same pair
        for q in (a, c, res[who + "_fromstarts"]):
            assert q.shape == (2 * D + 1,) and np.all((q[:2 * D] >= 0) & (q[:2 * D] <= 1)) and np.isfinite(q[2 * D])

    # the GaussianProcessRegressor's numbers again through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    val, grad = gp.eubo_eval(P)
    assert np.array_equal(val, res["gp_val"])
    assert np.array_equal(grad[:D].ravel(order="F"), res["gp_ga"]) and np.array_equal(grad[D:].ravel(order="F"), res["gp_gb"])
    rm = gp.eubo_maximize(starts, 20, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))        # GetLocalSearchTolerances' defaults
    assert np.array_equal(np.append(rm["x"], rm["value"]), res["gp_fromstarts"])
    assert abs(gp.eubo_eval(rm["x"][:, None], want_grad=False)[0] - rm["value"]) <= 1e-12
    gp.close()
    ctx.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    assert np.array_equal(pysls.calc_expected_utilities_of_best_option(reg, P[:D], P[D:]), res["gp_val"])
    xa, xb, value = pysls.find_next_query_pair_by_expected_utility(reg, 32, 20, 7)
    assert np.array_equal(np.concatenate([xa, xb, [value]]), res["gp_seed7a"])


def test_simulated_user_with_pair_queries():
    """Six two-option queries built by determine_next_query_by_expected_utility on a 2-D toy utility, answered by its argmax: the
    optimiser's maximiser ends better than the (deliberately poor) initial one, and every query lies in the box."""
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    pysls.set_random_seed(3)
    utility = lambda x: -float(np.sum((np.asarray(x) - 0.3) ** 2))
    first = [np.array([0.95, 0.95]), np.array([0.9, 0.05])]
    opt = pysls.PreferentialBayesianOptimizer(num_dims=2, use_map_hyperparams=False, initial_query_generator=lambda nd, no: first)
    with pytest.raises(Exception):
        opt.determine_next_query_by_expected_utility(0)       # before any feedback: as determine_next_query
    u0 = utility(opt.get_maximizer())
    for it in range(6):
        options = opt.get_current_options()
        assert len(options) == 2 and all(np.all((o >= 0) & (o <= 1)) for o in options)
        opt.submit_feedback_data(int(np.argmax([utility(o) for o in options])))
        opt.determine_next_query_by_expected_utility(it, 64, 20)
        a, b = opt.get_current_options()
        assert opt.get_preference_value_mean(a) >= opt.get_preference_value_mean(b)     # option 0 has the larger posterior mean
    u1 = utility(opt.get_maximizer())
    print(f"utility of the maximiser: {u0:.4f} -> {u1:.4f}")
    assert u1 > u0
    three = pysls.PreferentialBayesianOptimizer(num_dims=2, num_options=3)
    with pytest.raises(ValueError):
        three.determine_next_query_by_expected_utility(0)
