"""Max-value entropy search through the C++ host layer and the pybind11 module: acquisition_func::SampleMaxValues,
CalcMaxValueEntropies and FindNextPointByMaxValueEntropySearch on a GaussianProcessRegressor and a PreferenceRegressor (a small C++
program built against libsequential-line-search.so), against the ctypes path and the pybind11 functions on the same data."""
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

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
#include <sequential-line-search/preference-regressor.hpp>
using namespace sequential_line_search;

static void device_check(int rc) { if (rc != 0) { std::fprintf(stderr, "%s\n", sls_last_error()); std::exit(2); } }
static void print_vec(const char* tag, const Eigen::VectorXd& v) {
    std::printf("%s", tag);
    for (long i = 0; i < v.size(); ++i) std::printf(" %.17g", v(i));
    std::printf("\n");
}
static void run(const char* who, const Regressor& r, const Eigen::MatrixXd& Xs) {
    char tag[64];
    const Eigen::VectorXd ya = acquisition_func::SampleMaxValues(r, 16, 32, 20, 7, 512);
    const Eigen::VectorXd yb = acquisition_func::SampleMaxValues(r, 16, 32, 20, 7, 512);
    const Eigen::VectorXd yc = acquisition_func::SampleMaxValues(r, 16, 32, 20, 8, 512);
    std::snprintf(tag, sizeof tag, "%s_ya", who); print_vec(tag, ya);
    std::snprintf(tag, sizeof tag, "%s_yb", who); print_vec(tag, yb);
    std::snprintf(tag, sizeof tag, "%s_yc", who); print_vec(tag, yc);
    Eigen::VectorXd best(1);
    device_check(sls_gp_get_summary(r.GetDeviceHandle(), nullptr, &best(0), nullptr));
    std::snprintf(tag, sizeof tag, "%s_mubest", who); print_vec(tag, best);
    Eigen::MatrixXd grad;
    const Eigen::VectorXd v = acquisition_func::CalcMaxValueEntropies(r, Xs, ya, &grad);
    std::snprintf(tag, sizeof tag, "%s_val", who); print_vec(tag, v);
    Eigen::VectorXd gflat(grad.rows() * grad.cols());
    for (long j = 0; j < grad.cols(); ++j)
        for (long i = 0; i < grad.rows(); ++i) gflat(i + j * grad.rows()) = grad(i, j);
    std::snprintf(tag, sizeof tag, "%s_grad", who); print_vec(tag, gflat);
    // without the gradient sigma takes the value-only form of the evaluation: the same number to rounding, not to the bit
    std::snprintf(tag, sizeof tag, "%s_valonly", who); print_vec(tag, acquisition_func::CalcMaxValueEntropies(r, Xs, ya));
    for (int rep = 0; rep < 2; ++rep) {
        double value = 0.0;
        Eigen::VectorXd x = acquisition_func::FindNextPointByMaxValueEntropySearch(r, 16, 32, 20, 7, 512, &value);
        Eigen::VectorXd xv(x.size() + 1);
        for (long i = 0; i < x.size(); ++i) xv(i) = x(i);
        xv(x.size()) = value;
        std::snprintf(tag, sizeof tag, "%s_next%d", who, rep); print_vec(tag, xv);
    }
}

int main() {
    const int D = @D@, N = @N@, M = @M@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double Xsd[] = {@Xs@};
    Eigen::MatrixXd X(D, N), Xs(D, M);
    Eigen::VectorXd y(N), theta(D + 1);
    for (int i = 0; i < N; ++i) { y(i) = yd[i]; for (int d = 0; d < D; ++d) X(d, i) = Xd[d + i * D]; }
    for (int i = 0; i < M; ++i) for (int d = 0; d < D; ++d) Xs(d, i) = Xsd[d + i * D];
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    run("gp", gp, Xs);
    std::vector<Preference> prefs;
    for (int i = 0; i + 1 < N; i += 2) prefs.push_back(y(i) > y(i + 1) ? Preference(i, i + 1) : Preference(i + 1, i));
    PreferenceRegressor pr(X, prefs, false);
    run("pr", pr, Xs);
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def test_max_value_entropy_search_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    Xs = rng.uniform(0, 1, (D, M))
    src = tmp_path / "mes.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, X=c_list(X), y=c_list(y), Xs=c_list(Xs)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "mes"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    for who in ("gp", "pr"):
        ya, yb, yc = res[who + "_ya"], res[who + "_yb"], res[who + "_yc"]
        assert ya.shape == (16,) and np.array_equal(ya, yb) and not np.array_equal(ya, yc)
        assert np.all(np.isfinite(ya)) and np.all(ya >= res[who + "_mubest"][0]) and np.all(yc >= res[who + "_mubest"][0])
        n0, n1 = res[who + "_next0"], res[who + "_next1"]
        assert np.array_equal(n0, n1) and np.all((n0[:D] >= 0) & (n0[:D] <= 1)) and np.isfinite(n0[D]) and n0[D] > 0
        assert np.all(np.isfinite(res[who + "_val"])) and np.all(res[who + "_val"] >= 0)

    # the GaussianProcessRegressor's numbers again through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    val, grad = gp.mes_eval(res["gp_ya"], Xs)
    assert np.array_equal(val, res["gp_val"]) and np.array_equal(grad.ravel(order="F"), res["gp_grad"])
    assert np.array_equal(gp.mes_eval(res["gp_ya"], Xs, want_grad=False), res["gp_valonly"])
    np.testing.assert_allclose(res["gp_valonly"], res["gp_val"], rtol=1e-8, atol=1e-12)
    gp.close()
    ctx.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    ya = pysls.sample_max_values(reg, 16, 32, 20, 7, 512)
    assert np.array_equal(ya, res["gp_ya"])
    assert np.array_equal(pysls.calc_max_value_entropies(reg, Xs, ya), res["gp_valonly"])
    x, value = pysls.find_next_point_by_max_value_entropy_search(reg, 16, 32, 20, 7, 512)
    assert np.array_equal(np.append(x, value), res["gp_next0"])
