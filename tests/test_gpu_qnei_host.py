"""Noisy expected improvement on posterior draws through the C++ host layer and the pybind11 module:
PosteriorFunctionSamples::MaxOverPoints / CalcNoisyExpectedImprovements / MaximizeNoisyExpectedImprovement and
acquisition_func::FindNextPointsByNoisyExpectedImprovement[FromStarts] (a small C++ program built against
libsequential-line-search.so) against the ctypes path and the pybind11 functions on the same data, to the bit, and
PreferentialBayesianOptimizer.determine_next_query_by_noisy_expected_improvement with three options in a simulated-user loop."""
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
    Eigen::VectorXi arg;
    const Eigen::VectorXd t = draws.MaxOverPoints(X, &arg);
    print_vec("t", t);
    print_vec("tonly", draws.MaxOverPoints(X));
    Eigen::VectorXd av(ND);
    for (int s = 0; s < ND; ++s) av(s) = arg(s);
    print_vec("arg", av);
    std::vector<Eigen::MatrixXd> grads;
    Eigen::MatrixXi wins;
    print_vec("val", draws.CalcNoisyExpectedImprovements(options, t, &grads, &wins));
    for (int o = 0; o < Q; ++o) {
        char name[16];
        std::snprintf(name, sizeof name, "g%d", o);
        print_vec(name, flat(grads[o]));
    }
    Eigen::VectorXd w(Q * M);
    for (int i = 0; i < M; ++i) for (int o = 0; o < Q; ++o) w(o + i * Q) = wins(o, i);
    print_vec("wins", w);
    print_vec("valonly", draws.CalcNoisyExpectedImprovements(options, t));
    double value = 0.0;
    const auto a = draws.MaximizeNoisyExpectedImprovement(Q, t, starts, 20, &value);
    print_vec("maximize", query_and_value(a, value));
    const auto b = acquisition_func::FindNextPointsByNoisyExpectedImprovementFromStarts(gp, Q, starts, ND, 20, 5, NF, &value);
    print_vec("fromstarts", query_and_value(b, value));
    const unsigned long long seeds[3] = {7, 7, 8};
    const char* tags[3] = {"seed7a", "seed7b", "seed8"};
    for (int k = 0; k < 3; ++k) {
        const auto p = acquisition_func::FindNextPointsByNoisyExpectedImprovement(gp, Q, ND, 32, 20, seeds[k], NF, &value);
        print_vec(tags[k], query_and_value(p, value));
    }
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_batch_criterion_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    P = rng.uniform(0, 1, (Q * D, M))
    starts = rng.uniform(0, 1, (Q * D, S))
    src = tmp_path / "qnei.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, S=S, Q=Q, ND=ND, NF=NF, X=c_list(X), y=c_list(y), P=c_list(P), starts=c_list(starts)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "qnei"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    val, t = res["val"], res["t"]
    assert t.shape == (ND,) and np.all(np.isfinite(t)) and np.array_equal(res["tonly"], t)
    assert np.all((res["arg"] >= 0) & (res["arg"] < N))
    assert val.shape == (M,) and np.all(val >= 0.0) and np.array_equal(res["valonly"], val)
    assert np.all(res["wins"].reshape(M, Q).sum(axis=1) <= ND)
    assert np.array_equal(res["maximize"], res["fromstarts"]) and np.array_equal(res["seed7a"], res["seed7b"])
    for q in (res["seed7a"], res["seed8"], res["fromstarts"]):
        assert q.shape == (Q * D + 1,) and np.all((q[:Q * D] >= 0) & (q[:Q * D] <= 1)) and q[Q * D] >= 0.0
    assert res["fromstarts"][Q * D] > 0.0

    # the same numbers through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    ps = m.PathSamples(gp, ND, NF, seed=5)
    ct, carg = ps.max_over_points(X)
    assert np.array_equal(ct, t) and np.array_equal(carg, res["arg"])
    v, g, w = ps.qnei_eval(P, Q, ct, want_wins=True)
    assert np.array_equal(v, val) and np.array_equal(w.ravel(order="F"), res["wins"])
    for o in range(Q):
        assert np.array_equal(g[o * D:(o + 1) * D].ravel(order="F"), res[f"g{o}"])
    rm = ps.qnei_maximize(starts, Q, 20, ct, opts=m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6))   # GetLocalSearchTolerances' defaults
    assert np.array_equal(np.append(rm["x"], rm["value"]), res["fromstarts"])
    ps.close()
    gp.close()
    ctx.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    draws = pysls.sample_posterior_functions(reg, ND, 5, NF)
    pt, parg = draws.max_over_points(X)
    assert np.array_equal(pt, t) and np.array_equal(parg, carg) and parg.dtype == np.int32
    pv, pg, pw = draws.calc_noisy_expected_improvements([P[o * D:(o + 1) * D] for o in range(Q)], pt)
    assert np.array_equal(pv, val) and np.array_equal(pw, w) and pw.dtype == np.int32
    for o in range(Q):
        assert np.array_equal(pg[o], g[o * D:(o + 1) * D])
    pts, value = draws.maximize_noisy_expected_improvement(Q, pt, starts, 20)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["maximize"])
    pts, value = pysls.find_next_points_by_noisy_expected_improvement_from_starts(reg, Q, starts, ND, 20, 5, NF)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["fromstarts"])
    pts, value = pysls.find_next_points_by_noisy_expected_improvement(reg, Q, ND, 32, 20, 7, NF)
    assert np.array_equal(np.append(np.concatenate(pts), value), res["seed7a"])


def test_simulated_user_with_three_option_queries():
    """Six three-option queries built by determine_next_query_by_noisy_expected_improvement on a 2-D toy utility, answered by its
    argmax: every option lies in the box, option 0 is the current maximiser (the data point determine_next_query puts
    there), and the maximiser ends better than the (deliberately poor) initial one."""
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    pysls.set_random_seed(3)
    utility = lambda x: -float(np.sum((np.asarray(x) - 0.3) ** 2))
    first = [np.array([0.95, 0.95]), np.array([0.9, 0.05]), np.array([0.05, 0.9])]
    opt = pysls.PreferentialBayesianOptimizer(num_dims=2, use_map_hyperparams=False, initial_query_generator=lambda nd, no: first,
                                              num_options=3)
    with pytest.raises(Exception):
        opt.determine_next_query_by_noisy_expected_improvement(0)      # before any feedback: as determine_next_query
    u0 = utility(opt.get_maximizer())
    for it in range(6):
        options = opt.get_current_options()
        assert len(options) == 3 and all(np.all((o >= 0) & (o <= 1)) for o in options)
        opt.submit_feedback_data(int(np.argmax([utility(o) for o in options])))
        opt.determine_next_query(64, 20)
        x_plus = opt.get_current_options()[0]
        opt.determine_next_query_by_noisy_expected_improvement(it, 64, 64, 20)
        options = opt.get_current_options()
        data = opt.get_raw_data_points()                               # D x N
        assert np.array_equal(options[0], x_plus) and np.array_equal(options[0], opt.get_maximizer())
        assert any(np.array_equal(options[0], data[:, j]) for j in range(data.shape[1]))
    options = opt.get_current_options()
    assert len(options) == 3 and all(np.all((o >= 0) & (o <= 1)) for o in options)
    u1 = utility(opt.get_maximizer())
    print(f"utility of the maximiser: {u0:.4f} -> {u1:.4f}")
    assert u1 > u0
