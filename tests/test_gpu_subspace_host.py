"""The search over affine subspaces through the C++ host layer and the pybind11 module: SearchSubspace (Box, Segment, Centered, Point),
acquisition_func::CalcAcquisitionValuesInSubspace, FindNextPointInSubspacesFromStarts, FindNextPointInSubspace, FindNextPointInBox,
FindNextPointsByThompsonSamplingInBox and PosteriorFunctionSamples::MaximizeInSubspace (a small C++ program built against
libsequential-line-search.so) against the ctypes path on the same data, to the bit: the explicit-start forms from the same starts, the seeded forms from the starts
acquisition_func::SeededUniformStarts gives for their seed under the tolerances of GetLocalSearchTolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

import subspace_ref as sr
from util import sls

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequential-line-search_amd")
D, N, M, S, ND, NF, SD = 3, 25, 7, 48, 3, 128, 16      # SD: starts per draw
UCB_H = 1.5

PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <sls_hip.h>
#include <sequential-line-search/acquisition-function.hpp>
#include <sequential-line-search/gaussian-process-regressor.hpp>
using namespace sequential_line_search;
using Eigen::MatrixXd;
using Eigen::VectorXd;

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
static VectorXd with(const VectorXd& x, double a, double b = 0.0, bool two = false) {
    VectorXd out(x.size() + (two ? 2 : 1));
    for (long k = 0; k < x.size(); ++k) out(k) = x(k);
    out(x.size()) = a;
    if (two) out(x.size() + 1) = b;
    return out;
}
static VectorXd join(const std::vector<VectorXd>& xs) {
    VectorXd out(static_cast<long>(xs.size()) * (xs.empty() ? 0 : xs[0].size()));
    long at = 0;
    for (const VectorXd& x : xs) for (long k = 0; k < x.size(); ++k) out(at++) = x(k);
    return out;
}
static MatrixXd matrix(const double* p, int r, int c) {
    MatrixXd A(r, c);
    for (int j = 0; j < c; ++j) for (int i = 0; i < r; ++i) A(i, j) = p[i + j * r];
    return A;
}
static VectorXd vec(const double* p, int n) {
    VectorXd v(n);
    for (int i = 0; i < n; ++i) v(i) = p[i];
    return v;
}
template <class F> static double throws(F&& f) {
    try { f(); } catch (const std::invalid_argument&) { return 1.0; }
    return 0.0;
}
// a regressor without a device handle
struct HostOnly : Regressor {
    MatrixXd X; VectorXd y, theta;
    HostOnly(const MatrixXd& X_, const VectorXd& y_, const VectorXd& t) : Regressor(KernelType::ArdMatern52Kernel), X(X_), y(y_), theta(t) {}
    double PredictMu(const VectorXd&) const override { return 0.0; }
    double PredictSigma(const VectorXd&) const override { return 1.0; }
    VectorXd PredictMuDerivative(const VectorXd& x) const override { return VectorXd::Zero(x.size()); }
    VectorXd PredictSigmaDerivative(const VectorXd& x) const override { return VectorXd::Zero(x.size()); }
    const VectorXd& GetKernelHyperparams() const override { return theta; }
    double GetNoiseHyperparam() const override { return 0.01; }
    const MatrixXd& GetLargeX() const override { return X; }
    const VectorXd& GetSmallY() const override { return y; }
};

int main() {
    const int D = @D@, N = @N@, M = @M@, S = @S@, ND = @ND@, NF = @NF@, SD = @SD@;
    static const double Xd[] = {@X@};
    static const double yd[] = {@y@};
    static const double lod[] = {@lo@};
    static const double hid[] = {@hi@};
    static const double ctrd[] = {@ctr@};
    static const double dird[] = {@dirs@};
    static const double Zd[] = {@Z@};
    static const double Sd[] = {@starts@};
    static const double S2d[] = {@starts2@};
    static const double STd[] = {@startsT@};
    static const int sos[] = {@sos@};
    const MatrixXd X = matrix(Xd, D, N), starts = matrix(Sd, D, S), starts2 = matrix(S2d, 2, S), Z = matrix(Zd, 2, M);
    const MatrixXd startsT = matrix(STd, D, ND * SD), lo = matrix(lod, D, 2), hi = matrix(hid, D, 2);
    const VectorXd y = vec(yd, N);
    VectorXd theta(D + 1);
    theta(0) = 0.5;
    for (int d = 0; d < D; ++d) theta(d + 1) = 0.3;
    GaussianProcessRegressor gp(X, y, theta, 0.01, KernelType::ArdSquaredExponentialKernel);
    const SearchSubspace box0 = SearchSubspace::Box(lo.col(0), hi.col(0)), box1 = SearchSubspace::Box(lo.col(1), hi.col(1));
    const SearchSubspace cen = SearchSubspace::Centered(vec(ctrd, D), matrix(dird, D, 2));
    print_vec("cen_offset", cen.offset);
    print_vec("cen_basis", flat(cen.basis));
    print_vec("box0_offset", box0.offset);
    print_vec("box0_basis", flat(box0.basis));

    // the constructors
    VectorXd bad(3);
    VectorXd below = lo.col(0), above = hi.col(0);
    below(1) = -0.1;
    above(2) = 1.0 + 1e-12;
    bad(0) = throws([&] { SearchSubspace::Box(below, hi.col(0)); });
    bad(1) = throws([&] { SearchSubspace::Box(lo.col(0), above); });
    bad(2) = throws([&] { SearchSubspace::Box(hi.col(0), lo.col(0)); });
    print_vec("box_throws", bad);
    const SearchSubspace seg = SearchSubspace::Segment(lo.col(0), hi.col(1));
    VectorXd z0(1), z1(1);
    z0(0) = 0.0;
    z1(0) = 1.0;
    print_vec("segment_at_0", seg.Point(z0));
    print_vec("segment_at_1", seg.Point(z1));
    print_vec("cen_point", cen.Point(Z.col(0)));

    // evaluation and the maximisers from explicit starts
    MatrixXd gz;
    print_vec("vals", acquisition_func::CalcAcquisitionValuesInSubspace(gp, cen, Z, AcquisitionFuncType::GaussianProcessUpperConfidenceBound, @H@, &gz));
    print_vec("gz", flat(gz));
    double value = 0.0;
    int winner = -1;
    const std::vector<int> of(sos, sos + S);
    const VectorXd xb = acquisition_func::FindNextPointInSubspacesFromStarts(gp, {box0, box1}, of, starts, 20, AcquisitionFuncType::ExpectedImprovement,
                                                                            1.0, &value, &winner);
    print_vec("boxes_fromstarts", with(xb, value, winner, true));
    const VectorXd xc = acquisition_func::FindNextPointInSubspacesFromStarts(gp, {cen}, {}, starts2, 20,
                                                                            AcquisitionFuncType::GaussianProcessUpperConfidenceBound, @H@, &value, &winner);
    print_vec("cen_fromstarts", with(xc, value, winner, true));
    const PosteriorFunctionSamples draws = gp.SamplePosteriorFunctions(ND, 5, NF);
    VectorXd dv;
    const VectorXd dx = join(draws.MaximizeInSubspace(box0, startsT, 20, &dv));
    print_vec("draws_inbox", dx);
    print_vec("draws_inbox_values", dv);

    // the seeded forms, and the starts they draw
    print_vec("starts7_box", flat(acquisition_func::SeededUniformStarts(D, 32, 7)));
    print_vec("starts7_cen", flat(acquisition_func::SeededUniformStarts(2, 32, 7)));
    print_vec("starts7_ts", flat(acquisition_func::SeededUniformStarts(D, ND * SD, 7)));
    const unsigned long long seeds[3] = {7, 7, 8};
    const char* btags[3] = {"inbox7a", "inbox7b", "inbox8"};
    const char* ctags[3] = {"insub7a", "insub7b", "insub8"};
    const char* ttags[3] = {"ts7a", "ts7b", "ts8"};
    for (int k = 0; k < 3; ++k) {
        const VectorXd b = acquisition_func::FindNextPointInBox(gp, lo.col(0), hi.col(0), 32, 20, AcquisitionFuncType::ExpectedImprovement, 1.0,
                                                                seeds[k], &value);
        print_vec(btags[k], with(b, value));
        const VectorXd c = acquisition_func::FindNextPointInSubspace(gp, cen, 32, 20, AcquisitionFuncType::GaussianProcessUpperConfidenceBound, @H@,
                                                                     seeds[k], &value);
        print_vec(ctags[k], with(c, value));
        print_vec(ttags[k], join(acquisition_func::FindNextPointsByThompsonSamplingInBox(gp, ND, lo.col(0), hi.col(0), SD, 20, seeds[k], NF)));
    }

    // a regressor without a device handle
    const HostOnly host(X, y, theta);
    VectorXd refused(4);
    refused(0) = throws([&] { acquisition_func::FindNextPointInBox(host, lo.col(0), hi.col(0)); });
    refused(1) = throws([&] { acquisition_func::FindNextPointInSubspace(host, cen); });
    refused(2) = throws([&] { acquisition_func::CalcAcquisitionValuesInSubspace(host, cen, Z); });
    refused(3) = throws([&] { acquisition_func::FindNextPointsByThompsonSamplingInBox(host, 2, lo.col(0), hi.col(0)); });
    print_vec("host_only_throws", refused);
    return 0;
}
"""


def c_list(a):
    return ", ".join(float(v).hex() for v in np.asarray(a).ravel(order="F"))


def inputs():
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (D, N))
    y = -np.sum((X - 0.3) ** 2, axis=0)
    best = X[:, int(np.argmax(y))]
    lo = np.stack([np.clip(best - 0.2, 0, 1), np.clip(X[:, 1] - 0.25, 0, 1)], axis=1)
    hi = np.stack([np.clip(best + 0.2, 0, 1), np.clip(X[:, 1] + 0.25, 0, 1)], axis=1)
    ctr = rng.uniform(0.3, 0.7, D)
    dirs = rng.standard_normal((D, 2))
    dirs[0] *= 0.05                                       # one row that needs no scaling
    return dict(X=X, y=y, lo=lo, hi=hi, ctr=ctr, dirs=dirs, Z=rng.uniform(0, 1, (2, M)), starts=rng.uniform(-0.1, 1.1, (D, S)),
                starts2=rng.uniform(-0.1, 1.1, (2, S)), startsT=rng.uniform(0, 1, (D, ND * SD)), sos=rng.integers(0, 2, S))


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("subspace_host")
    inp = inputs()
    text = PROGRAM
    keys = dict(D=D, N=N, M=M, S=S, ND=ND, NF=NF, SD=SD, H=repr(UCB_H), sos=", ".join(str(int(v)) for v in inp["sos"]))
    keys.update({k: c_list(v) for k, v in inp.items() if k != "sos"})
    for key, value in keys.items():
        text = text.replace(f"@{key}@", str(value))
    src, exe = tmp / "subspace.cpp", tmp / "subspace"
    src.write_text(text)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", PKG,
                        "-lsequential-line-search", "-lsls_hip", f"-Wl,-rpath,{PKG}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in p.stdout.splitlines() if ln.strip()}


def centred_ref(ctr, dirs):
    """SearchSubspace::Centered: rows that would cross a face are scaled down so that they just reach it."""
    B = dirs.copy()
    for r in range(B.shape[0]):
        half = 0.0
        for j in range(B.shape[1]):
            half += 0.5 * abs(dirs[r, j])
        room = min(ctr[r], 1.0 - ctr[r])
        if half > room:
            B[r] *= room / half
    off = np.array([ctr[r] - 0.5 * sum(B[r, j] for j in range(B.shape[1])) for r in range(B.shape[0])])
    return off, B


def test_constructors(program_output):
    res, inp = program_output, inputs()
    assert np.array_equal(res["box_throws"], np.ones(3)), "Box accepts bounds outside 0 <= lower <= upper <= 1"
    assert np.array_equal(res["box0_offset"], inp["lo"][:, 0])
    assert np.array_equal(res["box0_basis"].reshape(D, D, order="F"), np.diag(inp["hi"][:, 0] - inp["lo"][:, 0]))
    off, B = centred_ref(inp["ctr"], inp["dirs"])
    assert np.allclose(res["cen_offset"], off, rtol=0, atol=1e-15) and np.allclose(res["cen_basis"].reshape(D, 2, order="F"), B, rtol=0, atol=1e-15)
    assert np.array_equal(B[0], inp["dirs"][0]) and not np.array_equal(B[1:], inp["dirs"][1:]), "premise: one row unscaled, the others scaled"
    corners = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=float).T
    img = res["cen_offset"][:, None] + res["cen_basis"].reshape(D, 2, order="F") @ corners
    assert img.min() >= -1e-15 and img.max() <= 1 + 1e-15, "the image of [0,1]^d leaves the cube"
    assert np.allclose(img.mean(axis=1), inp["ctr"], rtol=0, atol=1e-15), "the image is not centred at the centre"
    # a slider: z = 0 is the first end to the bit; z = 1 is a + (b - a), the second end to one rounding of each of the two operations
    assert np.array_equal(res["segment_at_0"], inp["lo"][:, 0])
    assert np.array_equal(res["segment_at_1"], inp["lo"][:, 0] + (inp["hi"][:, 1] - inp["lo"][:, 0]))
    assert np.abs(res["segment_at_1"] - inp["hi"][:, 1]).max() <= 2.0 ** -52
    A, c = res["cen_basis"].reshape(D, 2, order="F"), res["cen_offset"]
    assert np.array_equal(res["cen_point"], sr.expand(A, c, None, inp["Z"][:, :1])[:, 0]), "Point is not the contract's expand"
    assert np.array_equal(res["host_only_throws"], np.ones(4)), "a regressor without a device handle is not refused"


def test_host_layer_returns_what_the_c_abi_returns(program_output, monkeypatch):
    res, inp = program_output, inputs()
    m = sls()
    theta = np.array([0.5] + [0.3] * D)
    ctx = m.Context(0)
    gp = m.GP(ctx, inp["X"], inp["y"], theta, 0.01, m.KERNEL_SE)
    tol = m.LbfgsOpts(ftol_rel=1e-6, xtol_rel=1e-6)                                # GetLocalSearchTolerances' defaults
    cen = m.SubMaps(res["cen_basis"].reshape(D, 2, order="F"), res["cen_offset"])
    v, gz = gp.acq_eval_sub(cen, inp["Z"], m.ACQ_UCB, UCB_H)
    assert np.array_equal(v, res["vals"]) and np.array_equal(gz.ravel(order="F"), res["gz"])
    A = np.stack([np.diag(inp["hi"][:, k] - inp["lo"][:, k]) for k in range(2)])
    boxes = m.SubMaps(A, inp["lo"].T, inp["sos"])
    rb = gp.acq_maximize_sub(boxes, inp["starts"], 20, m.ACQ_EI, 1.0, opts=tol)
    assert np.array_equal(np.concatenate([rb["x"], [rb["value"], inp["sos"][rb["index"]]]]), res["boxes_fromstarts"])
    rc = gp.acq_maximize_sub(cen, inp["starts2"], 20, m.ACQ_UCB, UCB_H, opts=tol)
    assert np.array_equal(np.concatenate([rc["x"], [rc["value"], 0.0]]), res["cen_fromstarts"])
    ps = m.PathSamples(gp, ND, NF, seed=5)
    rd = ps.maximize_sub(m.SubMaps(A[0], inp["lo"][:, 0]), inp["startsT"], 20, opts=tol)
    assert np.array_equal(rd["x"].ravel(order="F"), res["draws_inbox"]) and np.array_equal(rd["value"], res["draws_inbox_values"])
    ps.close()

    # the seeded forms are the C ABI's result from the starts of their seed (SeededUniformStarts) under the default tolerances, bit for bit
    s_box, s_cen, s_ts = (res[k].reshape(r, -1, order="F") for k, r in (("starts7_box", D), ("starts7_cen", 2), ("starts7_ts", D)))
    assert s_box.shape == (D, 32) and s_ts.shape == (D, ND * SD) and np.all((s_ts >= 0.0) & (s_ts < 1.0))
    box0 = m.SubMaps(A[0], inp["lo"][:, 0])
    rs = gp.acq_maximize_sub(box0, s_box, 20, m.ACQ_EI, 1.0, opts=tol)
    assert np.array_equal(np.append(rs["x"], rs["value"]), res["inbox7a"]), "FindNextPointInBox is not the C ABI's result from its seed's starts"
    rs = gp.acq_maximize_sub(cen, s_cen, 20, m.ACQ_UCB, UCB_H, opts=tol)
    assert np.array_equal(np.append(rs["x"], rs["value"]), res["insub7a"]), "FindNextPointInSubspace is not the C ABI's result from its seed's starts"
    ps7 = m.PathSamples(gp, ND, NF, seed=7)
    rs = ps7.maximize_sub(box0, s_ts, 20, opts=tol)
    assert np.array_equal(rs["x"].ravel(order="F"), res["ts7a"]), "FindNextPointsByThompsonSamplingInBox is not the C ABI's result from its seed"
    ps7.close()

    # the same seed gives the same result (another seed may well end at the same optimum of a small box: nothing is
    # asserted on it); the points lie in their box / subspace and the value is the acquisition function's there (the tiled evaluation: the _sub routes never take another)
    monkeypatch.setenv("SLS_WAVE_PATH", "0")
    lo, hi = inp["lo"][:, 0], inp["hi"][:, 0]
    for tag, acq, h in (("inbox", m.ACQ_EI, 1.0), ("insub", m.ACQ_UCB, UCB_H)):
        a, b, c = res[f"{tag}7a"], res[f"{tag}7b"], res[f"{tag}8"]
        assert np.array_equal(a, b)
        for e in (a, c):
            assert e.shape == (D + 1,) and gp.acq_eval(e[:D, None], acq, h)[0][0] == e[D]
    for e, box in ((res["inbox7a"], 0), (res["inbox8"], 0), (res["boxes_fromstarts"], int(res["boxes_fromstarts"][D + 1]))):
        assert np.all(e[:D] >= inp["lo"][:, box]) and np.all(e[:D] <= inp["lo"][:, box] + (inp["hi"][:, box] - inp["lo"][:, box]))
    Ac, cc = res["cen_basis"].reshape(D, 2, order="F"), res["cen_offset"]
    for e in (res["insub7a"], res["insub8"], res["cen_fromstarts"]):
        z, *_ = np.linalg.lstsq(Ac, e[:D] - cc, rcond=None)
        assert np.all(z >= -1e-12) and np.all(z <= 1 + 1e-12) and np.abs(cc + Ac @ z - e[:D]).max() <= 1e-14, "the point is not in the subspace"
    assert np.array_equal(res["ts7a"], res["ts7b"])
    for t in (res["ts7a"], res["ts8"]):
        pts = t.reshape(D, ND, order="F")
        assert np.all(pts >= lo[:, None]) and np.all(pts <= (lo + (hi - lo))[:, None]), "a Thompson point leaves the box"
    gp.close()
    ctx.close()


def test_python_names_exist_and_agree(program_output):
    res, inp = program_output, inputs()
    sys.path.insert(0, PKG)
    import pySequentialLineSearch as pysls
    theta = np.array([0.5] + [0.3] * D)
    reg = pysls.GaussianProcessRegressor(inp["X"], inp["y"], theta, 0.01, pysls.KernelType.ArdSquaredExponentialKernel)
    lo, hi = inp["lo"][:, 0], inp["hi"][:, 0]
    for key, rows, count in (("starts7_box", D, 32), ("starts7_cen", 2, 32), ("starts7_ts", D, ND * SD)):
        assert np.array_equal(pysls.seeded_uniform_starts(rows, count, 7).ravel(order="F"), res[key])
    x, value = pysls.find_next_point_in_box(reg, lo, hi, 32, 20, pysls.AcquisitionFuncType.ExpectedImprovement, 1.0, 7)
    assert np.array_equal(np.append(x, value), res["inbox7a"])
    x, value = pysls.find_next_point_in_subspace(reg, res["cen_offset"], res["cen_basis"].reshape(D, 2, order="F"), num_global_search_iters=32,
                                                 num_local_search_iters=20, func_type=pysls.AcquisitionFuncType.GaussianProcessUpperConfidenceBound,
                                                 gaussian_process_upper_confidence_bound_hyperparam=UCB_H, seed=7)
    assert np.array_equal(np.append(x, value), res["insub7a"])
    pts = pysls.find_next_points_by_thompson_sampling_in_box(reg, ND, lo, hi, SD, 20, 7, NF)
    assert np.array_equal(np.concatenate(pts), res["ts7a"])
    with pytest.raises(ValueError):
        pysls.find_next_point_in_box(reg, lo - 0.5, hi)
