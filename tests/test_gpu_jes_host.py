"""Joint entropy search through the C++ host layer and the pybind11 module: acquisition_func::SampleOptima, CalcJointEntropies and
FindNextPointByJointEntropySearch on a GaussianProcessRegressor and a PreferenceRegressor (a small C++ program built against
libsequential-line-search.so), against SampleMaxValues, the ctypes path and the pybind11 functions on the same data."""
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
static Eigen::VectorXd flat(const Eigen::MatrixXd& A) {
    Eigen::VectorXd f(A.rows() * A.cols());
    for (long j = 0; j < A.cols(); ++j)
        for (long i = 0; i < A.rows(); ++i) f(i + j * A.rows()) = A(i, j);
    return f;
}
static void run(const char* who, const Regressor& r, const Eigen::MatrixXd& Xs) {
    char tag[64];
    const std::pair<Eigen::MatrixXd, Eigen::VectorXd> oa = acquisition_func::SampleOptima(r, 16, 32, 20, 7, 512);
    const std::pair<Eigen::MatrixXd, Eigen::VectorXd> ob = acquisition_func::SampleOptima(r, 16, 32, 20, 7, 512);
    const std::pair<Eigen::MatrixXd, Eigen::VectorXd> oc = acquisition_func::SampleOptima(r, 16, 32, 20, 8, 512);
    const Eigen::VectorXd ya = oa.second, yb = ob.second, yc = oc.second;
    std::snprintf(tag, sizeof tag, "%s_ym", who); print_vec(tag, acquisition_func::SampleMaxValues(r, 16, 32, 20, 7, 512));
    std::snprintf(tag, sizeof tag, "%s_xa", who); print_vec(tag, flat(oa.first));
    std::snprintf(tag, sizeof tag, "%s_xb", who); print_vec(tag, flat(ob.first));
    std::snprintf(tag, sizeof tag, "%s_ya", who); print_vec(tag, ya);
    std::snprintf(tag, sizeof tag, "%s_yb", who); print_vec(tag, yb);
    std::snprintf(tag, sizeof tag, "%s_yc", who); print_vec(tag, yc);
    Eigen::VectorXd best(1);
    device_check(sls_gp_get_summary(r.GetDeviceHandle(), nullptr, &best(0), nullptr));
    std::snprintf(tag, sizeof tag, "%s_mubest", who); print_vec(tag, best);
    Eigen::MatrixXd grad;
    const Eigen::VectorXd v = acquisition_func::CalcJointEntropies(r, Xs, oa.first, ya, &grad);
    std::snprintf(tag, sizeof tag, "%s_val", who); print_vec(tag, v);
    std::snprintf(tag, sizeof tag, "%s_grad", who); print_vec(tag, flat(grad));
    // without the gradient: the same bits (sigma is formed as the gradient evaluations form it either way)
    std::snprintf(tag, sizeof tag, "%s_valonly", who); print_vec(tag, acquisition_func::CalcJointEntropies(r, Xs, oa.first, ya));
    for (int rep = 0; rep < 2; ++rep) {
        double value = 0.0;
        Eigen::VectorXd x = acquisition_func::FindNextPointByJointEntropySearch(r, 16, 32, 20, 7, 512, &value);
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


def test_joint_entropy_search_through_the_host_layer(tmp_path):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    Xs = rng.uniform(0, 1, (D, M))
    src = tmp_path / "jes.cpp"
    text = PROGRAM
    for key, value in dict(D=D, N=N, M=M, X=c_list(X), y=c_list(y), Xs=c_list(Xs)).items():
        text = text.replace(f"@{key}@", str(value))
    src.write_text(text)
    exe = tmp_path / "jes"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}
    for who in ("gp", "pr"):
        ya, yb, yc = res[who + "_ya"], res[who + "_yb"], res[who + "_yc"]
        assert ya.shape == (16,) and np.array_equal(ya, yb) and not np.array_equal(ya, yc)
        assert np.array_equal(ya, res[who + "_ym"])                                   # the values of SampleMaxValues
        xa = res[who + "_xa"]
        assert xa.shape == (16 * D,) and np.array_equal(xa, res[who + "_xb"]) and np.all((xa >= 0) & (xa <= 1))
        assert np.all(np.isfinite(ya)) and np.all(ya >= res[who + "_mubest"][0])
        n0, n1 = res[who + "_next0"], res[who + "_next1"]
        assert np.array_equal(n0, n1) and np.all((n0[:D] >= 0) & (n0[:D] <= 1)) and np.isfinite(n0[D])
        assert np.all(np.isfinite(res[who + "_val"])) and np.array_equal(res[who + "_val"], res[who + "_valonly"])

    # the GaussianProcessRegressor's numbers again through ctypes (bit for bit) ...
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, X, y, theta, 0.01, m.KERNEL_SE)
    xa = res["gp_xa"].reshape((D, 16), order="F")
    j = gp.jes_create(xa, res["gp_ya"], 1e-8 * theta[0])
    val, grad = j.eval(Xs, 0.01)
    assert np.array_equal(val, res["gp_val"]) and np.array_equal(grad.ravel(order="F"), res["gp_grad"])
    j.close()
    gp.close()
    ctx.close()
    # ... and through the pybind11 module
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    reg = pysls.GaussianProcessRegressor(X, y, theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    ox, of = pysls.sample_optima(reg, 16, 32, 20, 7, 512)
    assert np.array_equal(of, res["gp_ya"]) and np.array_equal(ox.ravel(order="F"), res["gp_xa"])
    assert np.array_equal(of, pysls.sample_max_values(reg, 16, 32, 20, 7, 512))
    assert np.array_equal(pysls.calc_joint_entropies(reg, Xs, ox, of), res["gp_val"])
    x, value = pysls.find_next_point_by_joint_entropy_search(reg, 16, 32, 20, 7, 512)
    assert np.array_equal(np.append(x, value), res["gp_next0"])
