"""The expected utility of the best option of a query pair without a GPU: the numpy restatement (tests/eubo_ref.py) of the formulas
in include/sls_hip.h against the joint posterior covariance, central differences, the two-sided invariant, the swap symmetry and the
guard; the bindings and the header; and the host layer's refusals that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import eubo_ref
import posterior_ref
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
EPS = np.finfo(np.float64).eps
SE, MATERN52 = 0, 1
SHAPES = [(2, 30), (8, 90)]


def problem(D, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (D, N))
    y = np.sin(2.0 * X.sum(axis=0) / np.sqrt(D)) + 0.05 * rng.standard_normal(N)
    theta = np.concatenate([[0.5], 0.3 * np.sqrt(D) * rng.uniform(0.8, 1.25, D)])
    return X, y, theta, 0.05


def pairs_of(D, seed):
    """40 random pairs and 10 pairs 1e-3 apart."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 1.0, (2 * D, 50))
    step = rng.standard_normal((D, 10))
    P[D:, 40:] = np.clip(P[:D, 40:] + 1e-3 * step / np.linalg.norm(step, axis=0), 0.0, 1.0)
    return P


@pytest.fixture(scope="module", params=[(k, D, N) for k in (SE, MATERN52) for D, N in SHAPES], ids=lambda p: f"k{p[0]}-D{p[1]}-N{p[2]}")
def case(request):
    kernel, D, N = request.param
    X, y, theta, b = problem(D, N, seed=100 + D)
    P = pairs_of(D, seed=7 + D)
    val, grad, info = eubo_ref.eubo(X, y, theta, b, kernel, P)
    return dict(kernel=kernel, D=D, N=N, X=X, y=y, theta=theta, b=b, P=P, val=val, grad=grad, info=info)


def test_variance_of_the_difference_against_the_joint_covariance(case):
    c = case
    D, a = c["D"], c["theta"][0]
    worst = 0.0
    for m in range(c["P"].shape[1]):
        two = np.stack([c["P"][:D, m], c["P"][D:, m]], axis=1)
        mu, cov, cond = posterior_ref.posterior(c["X"], c["y"], two, c["theta"], c["b"], c["kernel"])
        s2 = cov[0, 0] + cov[1, 1] - 2.0 * cov[0, 1]
        tol = 64 * EPS * a * cond
        worst = max(worst, abs(s2 - c["info"]["own_s2"][m]) / tol)
        assert abs(s2 - c["info"]["own_s2"][m]) <= tol
        assert np.allclose(mu, c["info"]["mu"][:, m], rtol=0, atol=tol * np.abs(c["info"]["alpha"]).max() * np.sqrt(c["N"]))
    print(f"largest |s^2 - (cov00 + cov11 - 2 cov01)| / bound: {worst:.3g}")
    assert not c["info"]["bad"].any()


def test_gradient_against_central_differences(case):
    c = case
    D, h = c["D"], 1e-6
    fd = np.empty_like(c["grad"])
    for r in range(2 * D):
        E = np.zeros_like(c["P"])
        E[r] = h
        up = eubo_ref.eubo(c["X"], c["y"], c["theta"], c["b"], c["kernel"], c["P"] + E)[0]
        dn = eubo_ref.eubo(c["X"], c["y"], c["theta"], c["b"], c["kernel"], c["P"] - E)[0]
        fd[r] = (up - dn) / (2 * h)
    err = np.abs(fd - c["grad"]).max(axis=0)
    tol = 1e-5 * (1.0 + np.abs(c["grad"]).max(axis=0))
    print(f"largest central-difference error / bound: {(err / tol).max():.3g} (far pairs {(err / tol)[:40].max():.3g}, "
          f"close pairs {(err / tol)[40:].max():.3g})")
    assert np.all(err <= tol)


def test_two_sided_invariant(case):
    """max(mu, mu') <= E[max(f, f')] <= max(mu, mu') + s / sqrt(2 pi): EUBO - max(mu, mu') = s (phi(u) - |u| Phi(-|u|)), which lies in
    [0, s phi(0)]."""
    info = case["info"]
    mu, s = info["mu"], info["s"]
    excess = case["val"] - np.maximum(mu[0], mu[1])
    slack = 8 * EPS * (np.abs(mu[0]) + np.abs(mu[1]) + s)
    assert np.all(excess >= -slack) and np.all(excess <= s / np.sqrt(2 * np.pi) + slack)


def test_swap_symmetry(case):
    c = case
    D = c["D"]
    swapped = np.concatenate([c["P"][D:], c["P"][:D]], axis=0)
    v2, g2, _ = eubo_ref.eubo(c["X"], c["y"], c["theta"], c["b"], c["kernel"], swapped)
    assert np.abs(v2 - c["val"]).max() <= 1e-13
    assert np.abs(g2[:D] - c["grad"][D:]).max() <= 1e-13 * (1.0 + np.abs(c["grad"]).max())
    assert np.abs(g2[D:] - c["grad"][:D]).max() <= 1e-13 * (1.0 + np.abs(c["grad"]).max())


def test_guard(case):
    c = case
    D = c["D"]
    x = c["P"][:D, :3]
    P = np.concatenate([x, x], axis=0)                    # x = x': s^2 = 0 exactly
    P = np.concatenate([P, c["P"][:, :2]], axis=1)
    P[1, 3] = np.nan                                      # a NaN coordinate of x
    P[D, 4] = np.nan                                      # ... and of x'
    val, grad, info = eubo_ref.eubo(c["X"], c["y"], c["theta"], c["b"], c["kernel"], P)
    assert info["bad"].all()
    assert np.array_equal(grad, np.zeros_like(grad))
    assert np.array_equal(val[:3], np.maximum(info["mu"][0, :3], info["mu"][1, :3])) and np.all(np.isfinite(val[:3]))
    assert val[3] == info["mu"][1, 3] and val[4] == info["mu"][0, 4]          # fmax: the option that is a number
    ok = eubo_ref.eubo(c["X"], c["y"], c["theta"], c["b"], c["kernel"], c["P"][:, :2])
    assert not ok[2]["bad"].any() and np.abs(ok[1]).max() > 0


def test_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "sls_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = sls()
    for name in ("sls_eubo_eval", "sls_eubo_maximize"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in m.EXPORTS
    assert callable(m.GP.eubo_eval) and callable(m.GP.eubo_maximize)
    assert "expected utility of the best option" in txt and '"eubo"' in txt


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
    Eigen::MatrixXd A(2, 3), B(2, 3), S(4, 5);
    std::printf("eval %d\n", refuses([&] { acquisition_func::CalcExpectedUtilitiesOfBestOption(r, A, B); }));
    std::printf("find %d\n", refuses([&] { acquisition_func::FindNextQueryPairByExpectedUtility(r, 4, 3, 1); }));
    std::printf("starts %d\n", refuses([&] { acquisition_func::FindNextQueryPairByExpectedUtilityFromStarts(r, S, 3); }));
    PreferentialBayesianOptimizer three(2, false, KernelType::ArdMatern52Kernel, AcquisitionFuncType::ExpectedImprovement,
                                        GenerateRandomPoints, CurrentBestSelectionStrategy::LargestExpectValue, 3);
    std::printf("three %d\n", refuses([&] { three.DetermineNextQueryByExpectedUtility(0); }));
    PreferentialBayesianOptimizer two(2, false);
    int logic = 0;
    try { two.DetermineNextQueryByExpectedUtility(0); } catch (const std::logic_error&) { logic = 1; }
    std::printf("nodata %d\n", logic);
    return 0;
}
"""


def test_host_layer_refusals_without_a_device(tmp_path):
    """A regressor without a device handle is refused (std::invalid_argument, no host fallback), so is an optimiser with three
    options; before any feedback the optimiser method throws what DetermineNextQuery throws.  None of this touches the device."""
    import __graft_entry__ as g
    g.build()
    src, exe = tmp_path / "eubo_host.cpp", tmp_path / "eubo_host"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-3000:]
    got = dict(ln.split() for ln in p.stdout.splitlines() if ln.strip())
    assert got == dict(eval="1", find="1", starts="1", three="1", nodata="1"), p.stdout
