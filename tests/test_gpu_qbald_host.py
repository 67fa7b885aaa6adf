"""The information gain of a choice query on posterior draws through the C++ host layer and the pybind11 module:
PosteriorFunctionSamples::CalcChoiceInformationGains / MaximizeChoiceInformationGain and
acquisition_func::FindNextQueryByInformationGain[FromStarts] (a small C++ program built against libsequential-line-search.so) against
the ctypes path and the pybind11 functions on the same data, to the bit, the predicted choice probabilities included, and
PreferentialBayesianOptimizer.determine_next_query_by_information_gain with three options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M, S, Q, ND, NF = 3, 25, 7, 48, 3, 24, 128
TAU = 0.05

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
using namespace sequential_line_search;

static void print_vec(const char* what, const Eigen::VectorXd& v) {
    std::printf("%s", what);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static Eigen::VectorXd flat(const Eigen::MatrixXd& A) {
    Eigen::VectorXd f(A.rows() * A.cols());
    for (long j = 0; j < A.cols(); ++j)
        for (long i = 0; i < A.rows(); ++i) f(i + j * A.rows()) = A(i, j);
    return f;
}
static Eigen::VectorXd query_and_value(const std::vector<Eigen::VectorXd>& q, double value) {
    const long d = q[0].size(), n = static_cast<long>(q.size());
    Eigen::VectorXd out(n * d + 1);
    for (long i = 0; i < n; ++i)
        for (long k = 0; k < d; ++k) out(i * d + k) = q[i](k);
    out(n * d) = value;
    return out;
}

int main() {
    const int D = @D@, N = @N@, M = @M@, S = @S@, Q = @Q@, ND = @ND@, NF = @NF@;
    const double TAU = @TAU@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double Pd[] = {@P@};
    static const double Sd[] = {@starts@};
    Eigen::MatrixXd X(D, N), starts(Q * D, S);
    Eigen::VectorXd y(N), theta(D + 1);
    for (int i = 0; i < N; ++i) { y(i) = yd[i]; for (int d = 0; d < D; ++d) X(d, i) = Xd[d + i * D]; }
    std::vector<Eigen::MatrixXd> options(Q, Eigen::MatrixXd(D, M));
    for (int o = 0; o < Q; ++o)
        for (int i = 0; i < M; ++i) for (int d = 0; d < D; ++d) options[o](d, i) = Pd[o * D + d + i * Q * D];
    for (int i = 0; i < S; ++i) for (int d = 0; d < Q * D; ++d) starts(d, i) = Sd[d + i * Q * D];
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    const PosteriorFunctionSamples draws = gp.SamplePosteriorFunctions(ND, 5, NF);
    std::vector<Eigen::MatrixXd> grads;
    Eigen::MatrixXd prob;
    Eigen::MatrixXi wins;
    print_vec("val", draws.CalcChoiceInformationGains(options, TAU, &grads, &prob, &wins));
    for (int o = 0; o < Q; ++o) {
        char name[16];
        std::snprintf(name, sizeof name, "g%d", o);
        print_vec(name, flat(grads[o]));
    }
    print_vec("prob", flat(prob));
    Eigen::VectorXd w(Q * M);
    for (int i = 0; i < M; ++i) for (int o = 0; o < Q; ++o) w(o + i * Q) = wins(o, i);
    print_vec("wins", w);
    print_vec("valdefault", draws.CalcChoiceInformationGains(options, SLS_QBALD_SCALE));
    double value = 0.0;
    const auto a = draws.MaximizeChoiceInformationGain(Q, TAU, starts, 20, &value);
    print_vec("maximize", query_and_value(a, value));
    const auto b = acquisition_func::FindNextQueryByInformationGainFromStarts(gp, Q, TAU, starts, ND, 20, 5, NF, &value);
    print_vec("fromstarts", query_and_value(b, value));
    const auto c = acquisition_func::FindNextQueryByInformationGain(gp, Q, TAU, ND, 32, 20, 7, NF, &value);
    print_vec("seed7", query_and_value(c, value));
    try {
        draws.CalcChoiceInformationGains(options, 0.0);
        std::printf("refused 0\n");
    } catch (const std::exception&) {
        std::printf("refused 1\n");
    }
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_information_gain_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    P = rng.uniform(0, 1, (Q * D, M))
    starts = rng.uniform(0, 1, (Q * D, S))
    src = tmp_path / "qbald.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, S=S, Q=Q, ND=ND, NF=NF, TAU=TAU, X=c_list(X), y=c_list(y), P=c_list(P),
                           starts=c_list(starts)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "qbald"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    val = res["val"]
    assert val.shape == (M,) and np.all(val > 0) and np.all(val <= np.log(Q)) and res["refused"][0] == 1
    assert np.array_equal(res["maximize"], res["fromstarts"])
    for q in (res["seed7"], res["fromstarts"]):
        assert q.shape == (Q * D + 1,) and np.all((q[:Q * D] >= 0) & (q[:Q * D] <= 1)) and 0 < q[Q * D] <= np.log(Q)

    # the same numbers through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    ps = m.PathSamples(gp, ND, NF, seed=5)
    v, g, pr, w = ps.qbald_eval(P, Q, TAU, want_prob=True, want_wins=True)
    assert np.array_equal(v, val) and np.array_equal(w.ravel(order="F"), res["wins"])
    assert np.array_equal(pr.ravel(order="F"), res["prob"])
    for o in range(Q):
        assert np.array_equal(g[o * D:(o + 1) * D].ravel(order="F"), res[f"g{o}"])
    assert np.array_equal(ps.qbald_eval(P, Q, want_grad=False), res["valdefault"])
    tol = m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6)      # GetLocalSearchTolerances' defaults
    rm = ps.qbald_maximize(starts, Q, 20, TAU, opts=tol)
    assert np.array_equal(np.append(rm["x"], rm["value"]), res["fromstarts"])
    ps.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    draws = pysls.sample_posterior_functions(reg, ND, 5, NF)
    pv, pg, pp, pw = draws.calc_choice_information_gains([P[o * D:(o + 1) * D] for o in range(Q)], TAU)
    assert np.array_equal(pv, val) and np.array_equal(pp, pr) and np.array_equal(pw, w) and pw.dtype == np.int32
    for o in range(Q):
        assert np.array_equal(pg[o], g[o * D:(o + 1) * D])
    pv = draws.calc_choice_information_gains([P[o * D:(o + 1) * D] for o in range(Q)])[0]
    assert np.array_equal(pv, res["valdefault"])
    pts, value = draws.maximize_choice_information_gain(Q, starts, 20, TAU)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["maximize"])
    pts, value = pysls.find_next_query_by_information_gain_from_starts(reg, Q, starts, TAU, ND, 20, 5, NF)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["fromstarts"])
    pts, value = pysls.find_next_query_by_information_gain(reg, Q, TAU, ND, 32, 20, 7, NF)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["seed7"])
    # the seeded search is the ctypes maximiser from the seeded starts on the draws of the same stream: the value is that maximiser's
    p7 = m.PathSamples(gp, ND, NF, seed=7)
    r7 = p7.qbald_maximize(pysls.seeded_uniform_starts(Q * D, 32, 7), Q, 20, TAU, opts=tol)
    assert np.array_equal(np.append(r7["x"], r7["value"]), res["seed7"])
    p7.close()
    gp.close()
    ctx.close()


def test_next_query_with_three_options():
    """determine_next_query_by_information_gain on a 2-D toy utility: a query of three options inside [0,1]^2, all of them from the
    joint maximiser, the one with the largest posterior mean in position 0; the optimiser's own btl_scale (the default argument) and an
    explicit one."""
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    pysls.set_random_seed(3)
    utility = lambda x: -float(np.sum((np.asarray(x) - 0.3) ** 2))
    first = [np.array([0.95, 0.95]), np.array([0.9, 0.05]), np.array([0.05, 0.9])]
    opt = pysls.PreferentialBayesianOptimizer(num_dims=2, use_map_hyperparams=False, initial_query_generator=lambda nd, no: first,
                                              num_options=3)
    with pytest.raises(Exception):
        opt.determine_next_query_by_information_gain(0)  # before any feedback: as determine_next_query
    for it in range(3):
        options = opt.get_current_options()
        opt.submit_feedback_data(int(np.argmax([utility(o) for o in options])))
        for scale in (0.0, TAU):
            opt.determine_next_query_by_information_gain(it, 64, 64, 20, scale)
            options = opt.get_current_options()
            assert len(options) == 3 and all(o.shape == (2,) and np.all((o >= 0) & (o <= 1)) for o in options)
            mus = [opt.get_preference_value_mean(o) for o in options]
            assert mus[0] == max(mus) and np.array_equal(options[0], opt.get_maximizer())
        again = opt.get_current_options()
        opt.determine_next_query_by_information_gain(it, 64, 64, 20, TAU)
        assert all(np.array_equal(a, b) for a, b in zip(again, opt.get_current_options()))     # the same seed, the same query
