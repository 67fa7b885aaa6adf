"""The expected utility of the best slider position through the C++ host layer and the pybind11 module:
PosteriorFunctionSamples::CalcExpectedUtilitiesOfBestSliderPosition, acquisition_func::FindNextSliderByExpectedUtility[FromStarts]
(a small C++ program built against libsequential-line-search.so) against the ctypes path on the same data, to the bit, and
SequentialLineSearchOptimizer::SubmitFeedbackDataByExpectedUtility in a simulated-user loop beside plain SubmitFeedbackData."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M, S, Q, ND, NF = 3, 25, 7, 48, 5, 24, 128
OD, STEPS = 4, 5                                    # the optimiser loop

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/preference-regressor.hpp>
#include <sequential-line-search/sequential-line-search.hpp>
#include <sequential-line-search/utils.hpp>
using namespace sequential_line_search;
using Eigen::MatrixXd;
using Eigen::VectorXd;

static std::string g_dir;   // argv[1]: a scratch directory
static void print_vec(const char* what, const VectorXd& v) {
    std::printf("%s", what);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static VectorXd flat(const MatrixXd& A) {
    VectorXd f(A.rows() * A.cols());
    for (long j = 0; j < A.cols(); ++j)
        for (long i = 0; i < A.rows(); ++i) f(i + j * A.rows()) = A(i, j);
    return f;
}
static VectorXd ends_and_value(const std::pair<VectorXd, VectorXd>& e, double value) {
    const long d = e.first.size();
    VectorXd out(2 * d + 1);
    for (long k = 0; k < d; ++k) { out(k) = e.first(k); out(d + k) = e.second(k); }
    out(2 * d) = value;
    return out;
}
static double utility(const VectorXd& x) {
    double s = 0.0;
    for (long i = 0; i < x.size(); ++i) s -= (x(i) - 0.3) * (x(i) - 0.3);
    return s;
}
// the simulated user: the best of 11 positions on the slider
static double choose(const SequentialLineSearchOptimizer& opt) {
    double best = 0.0, ub = -1e300;
    for (int k = 0; k <= 10; ++k) {
        const double u = utility(opt.CalcPointFromSliderPosition(0.1 * k));
        if (u > ub) { ub = u; best = 0.1 * k; }
    }
    return best;
}
static std::pair<VectorXd, VectorXd> fixed_ends(const int d) {
    VectorXd a(d), b(d);
    for (int i = 0; i < d; ++i) { a(i) = 0.9 - 0.1 * i; b(i) = 0.15 + 0.2 * i; }
    return {a, b};
}
// OD-dimensional loop; by_utility: the new route.  Prints per step: the ends, the maximiser, the number of data points, and whether
// the maximiser is the arg-max of a regressor fitted to the same data.
static void loop(const char* tag, bool by_utility) {
    const int OD = @OD@, STEPS = @STEPS@;
    utils::SetRandomSeed(11);
    SequentialLineSearchOptimizer opt(OD, true, false, KernelType::ArdMatern52Kernel, AcquisitionFuncType::ExpectedImprovement, fixed_ends);
    VectorXd out(STEPS * (3 * OD + 2));
    long at = 0;
    for (int it = 0; it < STEPS; ++it) {
        const double pos = choose(opt);
        if (by_utility) opt.SubmitFeedbackDataByExpectedUtility(pos, 9, 32, 100, 24, 20, 100 + it, 128);
        else opt.SubmitFeedbackData(pos, 100, 10, 20);
        const auto ends = opt.GetSliderEnds();
        const VectorXd xm = opt.GetMaximizer();
        for (int k = 0; k < OD; ++k) out(at++) = ends.first(k);
        for (int k = 0; k < OD; ++k) out(at++) = ends.second(k);
        for (int k = 0; k < OD; ++k) out(at++) = xm(k);
        const MatrixXd& X = opt.GetRawDataPoints();
        out(at++) = static_cast<double>(X.cols());
        // the regressor's arg-max from a second regressor on the same points and preferences (the optimiser's hyper-parameters)
        opt.DampData(g_dir);
        std::vector<Preference> prefs;
        for (const auto& p : utils::ImportPreferencesFromCsv(g_dir + "/D.csv")) prefs.push_back(Preference(p));
        const PreferenceRegressor again(X, prefs, false, 0.5, 0.5, 0.005, 0.25, 0.01, 100, KernelType::ArdMatern52Kernel);
        const VectorXd xa = again.FindArgMax();
        bool same = true;
        for (int k = 0; k < OD; ++k) same = same && xa(k) == xm(k);
        out(at++) = same ? 1.0 : 0.0;
    }
    print_vec(tag, out);
}

int main(int argc, char** argv) {
    g_dir = argc > 1 ? argv[1] : ".";
    const int D = @D@, N = @N@, M = @M@, S = @S@, Q = @Q@, ND = @ND@, NF = @NF@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double Ld[] = {@L@};
    static const double Sd[] = {@starts@};
    MatrixXd X(D, N), A(D, M), B(D, M), starts(2 * D, S), startsb(D, S);
    VectorXd y(N), theta(D + 1);
    for (int i = 0; i < N; ++i) { y(i) = yd[i]; for (int d = 0; d < D; ++d) X(d, i) = Xd[d + i * D]; }
    for (int i = 0; i < M; ++i) for (int d = 0; d < D; ++d) { A(d, i) = Ld[d + i * 2 * D]; B(d, i) = Ld[D + d + i * 2 * D]; }
    for (int i = 0; i < S; ++i) for (int d = 0; d < 2 * D; ++d) starts(d, i) = Sd[d + i * 2 * D];
    for (int i = 0; i < S; ++i) for (int d = 0; d < D; ++d) startsb(d, i) = starts(D + d, i);
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    long best = 0;
    for (long i = 1; i < N; ++i) if (y(i) > y(best)) best = i;
    VectorXd anchor(D);
    for (int d = 0; d < D; ++d) anchor(d) = X(d, best);
    const PosteriorFunctionSamples draws = gp.SamplePosteriorFunctions(ND, 5, NF);
    MatrixXd ga, gb;
    Eigen::MatrixXi wins;
    print_vec("val", draws.CalcExpectedUtilitiesOfBestSliderPosition(A, B, Q, &ga, &gb, &wins));
    print_vec("ga", flat(ga));
    print_vec("gb", flat(gb));
    VectorXd w(Q * M);
    for (int i = 0; i < M; ++i) for (int o = 0; o < Q; ++o) w(o + i * Q) = wins(o, i);
    print_vec("wins", w);
    print_vec("valonly", draws.CalcExpectedUtilitiesOfBestSliderPosition(A, B, Q));
    double value = 0.0;
    const VectorXd none;
    const auto e1 = acquisition_func::FindNextSliderByExpectedUtilityFromStarts(gp, none, starts, Q, ND, 20, 5, NF, &value);
    print_vec("free_fromstarts", ends_and_value(e1, value));
    const auto e2 = acquisition_func::FindNextSliderByExpectedUtilityFromStarts(gp, anchor, startsb, Q, ND, 20, 5, NF, &value);
    print_vec("anch_fromstarts", ends_and_value(e2, value));
    const unsigned long long seeds[3] = {7, 7, 8};
    const char* ftags[3] = {"free7a", "free7b", "free8"};
    const char* atags[3] = {"anch7a", "anch7b", "anch8"};
    for (int k = 0; k < 3; ++k) {
        const auto f = acquisition_func::FindNextSliderByExpectedUtility(gp, none, Q, ND, 32, 20, seeds[k], NF, &value);
        print_vec(ftags[k], ends_and_value(f, value));
        const auto a = acquisition_func::FindNextSliderByExpectedUtility(gp, anchor, Q, ND, 32, 20, seeds[k], NF, &value);
        print_vec(atags[k], ends_and_value(a, value));
    }
    loop("plain_before", false);
    loop("by_utility", true);
    loop("plain_after", false);
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_slider_criterion_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    L = rng.uniform(0, 1, (2 * D, M))
    starts = rng.uniform(0, 1, (2 * D, S))
    src = tmp_path / "line.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, S=S, Q=Q, ND=ND, NF=NF, OD=OD, STEPS=STEPS, X=c_list(X), y=c_list(y), L=c_list(L),
                           starts=c_list(starts)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "line"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    val = res["val"]
    assert val.shape == (M,) and np.all(np.isfinite(val)) and np.array_equal(res["valonly"], val)
    assert np.array_equal(res["wins"].reshape(M, Q).sum(axis=1), np.full(M, ND))
    anchor = X[:, int(np.argmax(y))]
    for form in ("free", "anch"):
        assert np.array_equal(res[f"{form}7a"], res[f"{form}7b"])                  # the same seed, the same slider
        assert not np.array_equal(res[f"{form}7a"], res[f"{form}8"])
        for e in (res[f"{form}7a"], res[f"{form}8"], res[f"{form}_fromstarts"]):
            assert e.shape == (2 * D + 1,) and np.all((e[:2 * D] >= 0) & (e[:2 * D] <= 1)) and np.isfinite(e[2 * D])
    for k in ("anch7a", "anch8", "anch_fromstarts"):
        assert np.array_equal(res[k][:D], anchor)

    # the same numbers through ctypes, bit for bit
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    ps = m.PathSamples(gp, ND, NF, seed=5)
    v, g, w = ps.line_eval(L, Q, want_wins=True)
    assert np.array_equal(v, val) and np.array_equal(w.ravel(order="F"), res["wins"])
    assert np.array_equal(g[:D].ravel(order="F"), res["ga"]) and np.array_equal(g[D:].ravel(order="F"), res["gb"])
    tol = m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6)                                # GetLocalSearchTolerances' defaults
    rm = ps.line_maximize(starts, Q, 20, opts=tol)
    assert np.array_equal(np.append(rm["x"], rm["value"]), res["free_fromstarts"])
    ra = ps.line_maximize(starts[D:], Q, 20, anchor=anchor, opts=tol)
    assert np.array_equal(np.concatenate([anchor, ra["x"], [ra["value"]]]), res["anch_fromstarts"])
    ps.close()
    gp.close()
    ctx.close()

    # the optimiser: ends in the box, the maximiser is the regressor's arg-max, the data grow as under SubmitFeedbackData, and the
    # plain route gives the same bits before and after the new one was used
    per = 3 * OD + 2
    eu, plain = res["by_utility"].reshape(STEPS, per), res["plain_before"].reshape(STEPS, per)
    assert np.array_equal(res["plain_before"], res["plain_after"])
    assert np.all((eu[:, :2 * OD] >= 0.0) & (eu[:, :2 * OD] <= 1.0))
    assert np.all(eu[:, 3 * OD + 1] == 1.0) and np.all(plain[:, 3 * OD + 1] == 1.0)
    assert np.array_equal(eu[:, 3 * OD], plain[:, 3 * OD]) and np.all(np.diff(eu[:, 3 * OD]) > 0)
    assert not np.array_equal(eu[:, :2 * OD], plain[:, :2 * OD])                   # the two criteria do choose different sliders


def test_python_names_exist_and_run():
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    theta = np.array([0.5] + [0.3] * D)
    L = rng.uniform(0, 1, (2 * D, M))
    starts = rng.uniform(0, 1, (2 * D, S))
    anchor = X[:, int(np.argmax(y))]
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    draws = pysls.sample_posterior_functions(reg, ND, 5, NF)
    pv, pga, pgb, pw = draws.calc_expected_utilities_of_best_slider_position(L[:D], L[D:], Q)
    m = sls()
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    ps = m.PathSamples(gp, ND, NF, seed=5)
    v, g, w = ps.line_eval(L, Q, want_wins=True)
    assert np.array_equal(pv, v) and np.array_equal(pga, g[:D]) and np.array_equal(pgb, g[D:]) and np.array_equal(pw, w)
    tol = m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6)
    (e0, e1), value = pysls.find_next_slider_by_expected_utility_from_starts(reg, anchor, starts[D:], Q, ND, 20, 5, NF)
    ra = ps.line_maximize(starts[D:], Q, 20, anchor=anchor, opts=tol)
    assert np.array_equal(e0, anchor) and np.array_equal(e1, ra["x"]) and value == ra["value"]
    (f0, f1), fvalue = draws.maximize_expected_utility_of_best_slider_position(Q, starts, 20)
    rf = ps.line_maximize(starts, Q, 20, opts=tol)
    assert np.array_equal(np.concatenate([f0, f1]), rf["x"]) and fvalue == rf["value"]
    (a0, a1), avalue = pysls.find_next_slider_by_expected_utility(reg, anchor, Q, ND, 32, 20, 7, NF)
    (b0, b1), bvalue = pysls.find_next_slider_by_expected_utility(reg, anchor, Q, ND, 32, 20, 7, NF)
    assert np.array_equal(a1, b1) and avalue == bvalue and np.all((a1 >= 0) & (a1 <= 1))
    (c0, c1), cvalue = pysls.find_next_slider_by_expected_utility(reg, num_positions=Q, num_draws=ND, num_global_search_iters=32,
                                                                  num_local_search_iters=20, seed=7, num_frequencies=NF)
    assert c0.shape == (D,) and c1.shape == (D,) and np.isfinite(cvalue)
    with pytest.raises(ValueError):
        pysls.find_next_slider_by_expected_utility(reg, anchor, 1)
    ps.close()
    gp.close()
    ctx.close()

    pysls.set_random_seed(3)
    utility = lambda x: -float(np.sum((np.asarray(x) - 0.3) ** 2))
    opt = pysls.SequentialLineSearchOptimizer(num_dims=2, use_map_hyperparams=False)
    for it in range(3):
        pos = max(np.linspace(0, 1, 11), key=lambda t: utility(opt.calc_point_from_slider_position(t)))
        opt.submit_feedback_data_by_expected_utility(float(pos), num_draws=32, num_global_search_iters=16, num_local_search_iters=10,
                                                     seed=it, num_frequencies=128)
        e0, e1 = opt.get_slider_ends()
        assert np.all((e0 >= 0) & (e0 <= 1)) and np.all((e1 >= 0) & (e1 <= 1))
    assert opt.get_maximizer().shape == (2,)
