"""The expected utility of the best of q options on posterior draws without a GPU: the numpy restatement (tests/qeubo_ref.py) against
the draw mean (q = 1), central differences of its own values, and the closed form of the pair criterion with the pathwise variance of
the same frequency set (the exact expectation of the q = 2 estimator); the C ABI's declarations; the host layer's refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import eubo_ref
import path_ref as ph
import qeubo_ref as qr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")


def problem(D, N, seed, ell=0.5, a=0.5):
    """tests/test_gpu_path_sample.py's generator."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[a], np.full(D, ell) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta


def test_one_option_is_the_draw_mean():
    D, N, F, S = 3, 60, 200, 37
    X, y, theta = problem(D, N, seed=4)
    ref = ph.PathRef(X, y, theta, 0.02, ph.MATERN52, S, F, seed=11)
    Xs = np.random.default_rng(0).uniform(0, 1, (D, 20))
    val, grad, wins, gap = qr.qeubo(ref, Xs, 1)
    allv = ref.eval_all(Xs)
    assert np.abs(val - allv.mean(axis=1)).max() <= 4 * S * np.finfo(float).eps * np.abs(allv).max()
    assert np.array_equal(wins, np.full((1, 20), S)) and np.all(np.isinf(gap))
    # the gradient of the mean of the draws is the mean of their gradients
    g = sum(ref.eval(Xs, np.full(20, s))[1] for s in range(S)) / S
    assert np.abs(grad - g).max() <= 1e-12 * (1 + np.abs(g).max())


@pytest.mark.parametrize("kernel,q", [(ph.SE, 2), (ph.MATERN52, 3), (ph.SE, 5)])
def test_gradient_matches_central_differences(kernel, q):
    D, N, F, S, M = 3, 50, 150, 5, 64
    X, y, theta = problem(D, N, seed=21 + q)
    a = theta[0]
    ref = ph.PathRef(X, y, theta, 0.02, kernel, S, F, seed=3)
    sets = np.random.default_rng(7).uniform(0.05, 0.95, (q * D, M))
    val, grad, wins, gap = qr.qeubo(ref, sets, q)
    assert np.array_equal(wins.sum(axis=0), np.full(M, S))
    # no winner may change inside the stencil: a draw's value moves by at most h |grad f_s|, far below 1e-4 a at h = 1e-6
    ok = gap >= 1e-4 * a
    assert ok.sum() >= 8, ok.sum()
    h = 1e-6
    for r in range(q * D):
        E = np.zeros((q * D, M))
        E[r] = h
        fd = (qr.qeubo(ref, sets + E, q)[0] - qr.qeubo(ref, sets - E, q)[0]) / (2 * h)
        assert np.abs(fd - grad[r])[ok].max() <= 1e-6 * (a + np.abs(grad[:, ok]).max())
    # an option that wins no draw has an exactly zero gradient
    for i in range(q):
        none = wins[i] == 0
        assert np.all(grad[i * D:(i + 1) * D][:, none] == 0.0)


@pytest.mark.parametrize("F,S", [(1024, 4096), (8192, 4096), (1024, 512)])
def test_two_options_against_the_fixed_basis_closed_form(F, S):
    """E[max(f(x), f(x'))] of two jointly normal values with the exact posterior means and the variance of the difference THIS basis
    gives is the expectation of the estimator; the sample mean over S draws lies within 5 standard errors of it."""
    D, N, b = 3, 200, 0.02
    X, y, theta = problem(D, N, seed=9, ell=0.35)
    ref = ph.PathRef(X, y, theta, b, ph.SE, S, F, seed=F)
    pairs = np.random.default_rng(2).uniform(0, 1, (2 * D, 64))
    val, _, wins, _ = qr.qeubo(ref, pairs, 2)
    exact = eubo_ref.eubo(X, y, theta, b, eubo_ref.SE, pairs, s2=qr.pair_variance(ref, pairs[:D], pairs[D:]))[0]
    best = np.maximum(ref.eval_all(pairs[:D]), ref.eval_all(pairs[D:]))
    se = best.std(axis=1, ddof=1) / np.sqrt(S)
    dev = np.abs(val - exact) / se
    print(f"F = {F}, S = {S}: largest deviation {dev.max():.2f} standard errors")
    assert dev.max() <= 5.0, dev.max()
    assert np.array_equal(wins.sum(axis=0), np.full(64, S))


def test_guard_of_the_restatement():
    D, N, F, S = 2, 20, 32, 4
    X, y, theta = problem(D, N, seed=1)
    ref = ph.PathRef(X, y, theta, 0.02, ph.SE, S, F, seed=1)
    sets = np.full((2 * D, 3), 0.25)
    sets[1, 1] = np.nan
    with np.errstate(all="ignore"):
        val, grad, _, _ = qr.qeubo(ref, sets, 2)
    assert val[1] == qr.FLOOR and np.all(grad[:, 1] == 0.0) and np.all(np.isfinite(val[[0, 2]]))
    # a duplicated option never wins: x_1 = x_0
    assert np.array_equal(qr.qeubo(ref, sets[:, :1], 2)[2][:, 0], [S, 0])


def test_header_declares_and_binding_exports():
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    for name in ("sls_qeubo_eval", "sls_qeubo_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
    assert re.search(r"#define\s+SLS_QEUBO_MAX_OPTIONS\s+16\b", code) and re.search(r"#define\s+SLS_QEUBO_FLOOR\s+\(-1\.0e300\)", code)
    assert callable(m.PathSamples.qeubo_eval) and callable(m.PathSamples.qeubo_maximize)
    assert '"qeubo"' in txt and '"qeubo_agg"' in txt
    ps = m.PathSamples.__new__(m.PathSamples)            # q outside 1 .. 16 is refused before anything is allocated or called
    ps.D, ps.h = 2, None
    for q in (0, 17, -1):
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qeubo_eval(np.zeros((2, 1)), q)
        with pytest.raises(m.SlsError, match="1 .. 16"):
            ps.qeubo_maximize(np.zeros((2, 1)), q, 3)


PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/preferential-bayesian-optimizer.hpp>
using namespace sequential_line_search;

// a user subclass of Regressor: no device handle
struct HostOnly : Regressor {
    Eigen::MatrixXd X = Eigen::MatrixXd(2, 1);
    Eigen::VectorXd y = Eigen::VectorXd(1), theta = Eigen::VectorXd(3);
    HostOnly() : Regressor(KernelType::ArdMatern52Kernel) {}
    double PredictMu(const Eigen::VectorXd&) const override { return 0.0; }
    double PredictSigma(const Eigen::VectorXd&) const override { return 1.0; }
    Eigen::VectorXd PredictMuDerivative(const Eigen::VectorXd& x) const override { return Eigen::VectorXd::Zero(x.size()); }
    Eigen::VectorXd PredictSigmaDerivative(const Eigen::VectorXd& x) const override { return Eigen::VectorXd::Zero(x.size()); }
    const Eigen::VectorXd& GetKernelHyperparams() const override { return theta; }
    double GetNoiseHyperparam() const override { return 0.0; }
    const Eigen::MatrixXd& GetLargeX() const override { return X; }
    const Eigen::VectorXd& GetSmallY() const override { return y; }
};

template <class F> static int refuses(F&& f) {
    try { f(); } catch (const std::invalid_argument&) { return 1; } catch (...) { return -1; }
    return 0;
}

int main() {
    HostOnly r;
    Eigen::MatrixXd S(6, 5);
    std::printf("find %d\n", refuses([&] { acquisition_func::FindNextQueryByExpectedUtility(r, 3, 8, 4, 3, 1, 16); }));
    std::printf("starts %d\n", refuses([&] { acquisition_func::FindNextQueryByExpectedUtilityFromStarts(r, 3, S, 8, 3, 1, 16); }));
    std::printf("draws %d\n", refuses([&] { r.SamplePosteriorFunctions(4, 1, 16); }));
    PreferentialBayesianOptimizer three(2, false, KernelType::ArdMatern52Kernel, AcquisitionFuncType::ExpectedImprovement,
                                        GenerateRandomPoints, CurrentBestSelectionStrategy::LargestExpectValue, 3);
    int logic = 0;
    try { three.DetermineNextQueryByExpectedUtilityOfDraws(0); } catch (const std::logic_error&) { logic = 1; }
    std::printf("nodata %d\n", logic);
    std::printf("pairs_only %d\n", refuses([&] { three.DetermineNextQueryByExpectedUtility(0); }));
    return 0;
}
"""


def test_host_layer_refusals_without_a_device(tmp_path):
    """A regressor without a device handle is refused (std::invalid_argument, no host fallback); before any feedback the optimiser
    method throws what DetermineNextQuery throws; the pair criterion keeps refusing three options.  None of this touches the device."""
    import __graft_entry__ as g
    g.build()
    src, exe = tmp_path / "qeubo_host.cpp", tmp_path / "qeubo_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    got = dict(ln.split() for ln in p.stdout.splitlines() if ln.strip())
    assert got == dict(find="1", starts="1", draws="1", nodata="1", pairs_only="1"), p.stdout
