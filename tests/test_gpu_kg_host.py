"""The knowledge gradient through the C++ host layer and the pybind11 module: acquisition_func::CalcKnowledgeGradients,
KnowledgeGradientReferencePoints and FindNextPointByKnowledgeGradient on a GaussianProcessRegressor and a PreferenceRegressor (a small
C++ program built against libsequential-line-search.so), against the ctypes path and the pybind11 functions on the same data; the
default reference set with more than 1024 data points."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M = 3, 25, 7
D2, N2 = 2, 1100

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/preference-regressor.hpp>
using namespace sequential_line_search;

static void print_vec(const char* tag, const Eigen::VectorXd& v) {
    std::printf("%s", tag);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static Eigen::VectorXd flat(const Eigen::MatrixXd& A) {
    Eigen::VectorXd f(A.rows() * A.cols());
    for (long j = 0; j < A.cols(); ++j)
        for (long i = 0; i < A.rows(); ++i) f(i + j * A.rows()) = A(i, j);
    return f;
}
static void next(const char* who, const char* what, const Regressor& r, unsigned long long seed) {
    char tag[64];
    double value = 0.0;
    Eigen::VectorXd x = acquisition_func::FindNextPointByKnowledgeGradient(r, 32, 20, seed, &value);
    Eigen::VectorXd xv(x.size() + 1);
    for (long i = 0; i < x.size(); ++i) xv(i) = x(i);
    xv(x.size()) = value;
    std::snprintf(tag, sizeof tag, "%s_%s", who, what); print_vec(tag, xv);
}
static void run(const char* who, const Regressor& r, const Eigen::MatrixXd& Xs) {
    char tag[64];
    const Eigen::MatrixXd ref = acquisition_func::KnowledgeGradientReferencePoints(r);
    std::snprintf(tag, sizeof tag, "%s_ref", who); print_vec(tag, flat(ref));
    Eigen::MatrixXd grad;
    const Eigen::VectorXd v = acquisition_func::CalcKnowledgeGradients(r, Xs, ref, &grad);
    std::snprintf(tag, sizeof tag, "%s_val", who); print_vec(tag, v);
    std::snprintf(tag, sizeof tag, "%s_grad", who); print_vec(tag, flat(grad));
    std::snprintf(tag, sizeof tag, "%s_valonly", who); print_vec(tag, acquisition_func::CalcKnowledgeGradients(r, Xs, ref));
    std::snprintf(tag, sizeof tag, "%s_fixed", who); print_vec(tag, acquisition_func::CalcKnowledgeGradients(r, Xs, ref, nullptr, false));
    next(who, "next0", r, 7);
    next(who, "next1", r, 7);
    next(who, "next2", r, 8);
}

int main() {
    const int D = @D@, N = @N@, M = @M@, D2 = @D2@, N2 = @N2@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double Xsd[] = {@Xs@};
    static const double X2d[] = {@X2@};
    static const double y2d[] = {@y2@};
    Eigen::MatrixXd X(D, N), Xs(D, M), X2(D2, N2);
    Eigen::VectorXd y(N), theta(D + 1), y2(N2), theta2(D2 + 1);
    for (int i = 0; i < N; ++i) { y(i) = yd[i]; for (int d = 0; d < D; ++d) X(d, i) = Xd[d + i * D]; }
    for (int i = 0; i < M; ++i) for (int d = 0; d < D; ++d) Xs(d, i) = Xsd[d + i * D];
    for (int i = 0; i < N2; ++i) { y2(i) = y2d[i]; for (int d = 0; d < D2; ++d) X2(d, i) = X2d[d + i * D2]; }
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    theta2(0) = 0.5;
    for (int d = 0; d < D2; ++d) theta2(d + 1) = 0.2;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    run("gp", gp, Xs);
    std::vector<Preference> prefs;
    for (int i = 0; i + 1 < N; i += 2) prefs.push_back(y(i) > y(i + 1) ? Preference(i, i + 1) : Preference(i + 1, i));
    PreferenceRegressor pr(X, prefs, false);
    run("pr", pr, Xs);
    GaussianProcessRegressor big(X2, y2, theta2, 0.05, KernelType::ArdMatern52Kernel);
    print_vec("big_ref", flat(acquisition_func::KnowledgeGradientReferencePoints(big)));
    next("big", "next0", big, 3);
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_knowledge_gradient_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    Xs = rng.uniform(0, 1, (D, M))
    X2 = rng.uniform(0, 1, (D2, N2))
    y2 = np.sin(5 * X2[0]) * np.cos(3 * X2[1]) + 0.2 * rng.standard_normal(N2)
    src = tmp_path / "kg.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, D2=D2, N2=N2, X=c_list(X), y=c_list(y), Xs=c_list(Xs), X2=c_list(X2), y2=c_list(y2)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "kg"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    for who in ("gp", "pr"):
        assert np.array_equal(res[who + "_ref"], X.ravel(order="F"))                  # N <= 1024: the data points
        n0, n1, n2 = res[who + "_next0"], res[who + "_next1"], res[who + "_next2"]
        assert np.array_equal(n0, n1)                                                 # the same seed: the same point
        assert np.all((n2[:D] >= 0) & (n2[:D] <= 1)) and np.isfinite(n2[D])           # (another seed may end at the same maximiser)
        assert np.all((n0[:D] >= 0) & (n0[:D] <= 1)) and np.isfinite(n0[D]) and n0[D] >= 0.0
        val = res[who + "_val"]
        assert np.all(np.isfinite(val)) and np.all(val >= 0.0) and np.array_equal(val, res[who + "_valonly"])
        assert np.all(res[who + "_fixed"] >= 0.0)

    # the GaussianProcessRegressor's numbers again through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    kg = gp.kg_create(X)
    val, grad = kg.eval(Xs, 0.01, want_grad=True)
    assert np.array_equal(val, res["gp_val"]) and np.array_equal(grad.ravel(order="F"), res["gp_grad"])
    assert np.array_equal(kg.eval(Xs, 0.01, include_self=False), res["gp_fixed"])
    kg.close()
    gp.close()
    # the default reference set above 1024 data points: the 1024 highest posterior means, ties to the lower index, in index order
    theta2 = np.array([0.5] + [0.2] * D2)
    big = m.GP(ctx, X2, y2, theta2, 0.05, m.KERNEL_MATERN52)
    mu = big.predict(X2)[0]
    keep = np.sort(np.argsort(-mu, kind="stable")[:1024])
    assert np.array_equal(res["big_ref"], X2[:, keep].ravel(order="F"))
    kb = big.kg_create(X2[:, keep])
    assert res["big_next0"][D2] >= 0.0 and np.all((res["big_next0"][:D2] >= 0) & (res["big_next0"][:D2] <= 1))
    assert np.array_equal(kb.eval(res["big_next0"][:D2, None], 0.05), res["big_next0"][D2:])   # the value is the knowledge gradient there
    kb.close()
    big.close()
    ctx.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    assert np.array_equal(pysls.knowledge_gradient_reference_points(reg), X)
    assert np.array_equal(pysls.calc_knowledge_gradients(reg, Xs, X), res["gp_val"])
    assert np.array_equal(pysls.calc_knowledge_gradients(reg, Xs, X, include_candidate=False), res["gp_fixed"])
    x, value = pysls.find_next_point_by_knowledge_gradient(reg, 32, 20, 7)
    assert np.array_equal(np.append(x, value), res["gp_next0"])
