"""CPU-side checks of the joint-posterior surface (sls_gp_predict_cov, sls_gp_sample_posterior, sls_random_normal): the header still
compiles as pedantic C99 and a C program that calls the new entry points links; without a device they return the library's errors
instead of computing anything on the host; and the numpy restatement of the generator (tests/posterior_ref.py) stands on numpy's
Philox with its counter convention pinned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import posterior_ref as pr
from util import sls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_header_declares_the_posterior_calls_and_compiles_as_c99(tmp_path):
    src = tmp_path / "post.c"
    src.write_text('#include <stdio.h>\n#include "sls_hip.h"\n'
                   'int main(void) {\n'
                   '    sls_ctx* c = 0;\n'
                   '    double xs[2] = {0.5, 0.5}, mu[1], cov[1], f[1], j = -1.0, z[1];\n'
                   '    int rc0 = sls_ctx_create(0, &c);\n'
                   '    int rc1 = sls_gp_predict_cov((sls_gp*)0, xs, 1, mu, cov);\n'
                   '    int rc2 = sls_gp_sample_posterior((sls_gp*)0, xs, 1, 1, 42ULL, f, &j);\n'
                   '    int rc3 = sls_random_normal(c, 42ULL, 0L, 1L, z);\n'
                   '    printf("rc %d %d %d %d msg %s\\n", rc0, rc1, rc2, rc3, sls_last_error());\n'
                   '    if (c) sls_ctx_destroy(c);\n'
                   '    return 0;\n}\n')
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "sequential-line-search_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if not os.path.exists(os.path.join(libdir, "libsls_hip.so")):
        import __graft_entry__ as g
        g.build()
    exe = tmp_path / "post"
    r = subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lsls_hip", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"rc (-?\d+) (-?\d+) (-?\d+) (-?\d+) msg", r.stdout)
    assert m, r.stdout
    rcs = [int(v) for v in m.groups()]
    # a NULL handle is refused on any machine, before anything touches a device
    assert rcs[1] == -1 and rcs[2] == -1, r.stdout
    if _no_gpu():
        assert rcs[0] == -4 and rcs[3] == -1, r.stdout


def test_no_cpu_fallback_for_the_posterior_calls():
    """Without a device there is no context and so no handle: the entry points return errors, the binding raises."""
    if not _no_gpu():
        pytest.skip("GPU present")
    m = sls()
    with pytest.raises(m.SlsError) as e:
        m.Context(0)
    assert "no CPU fallback" in str(e.value)
    lib = m.lib()
    xs = np.full(4, 0.5)
    out = np.zeros(4)
    dp = C.POINTER(C.c_double)
    assert lib.sls_gp_predict_cov(None, xs.ctypes.data_as(dp), 2, None, out.ctypes.data_as(dp)) == -1
    assert lib.sls_gp_sample_posterior(None, xs.ctypes.data_as(dp), 2, 1, C.c_ulonglong(1), out.ctypes.data_as(dp), None) == -1
    assert lib.sls_random_normal(None, C.c_ulonglong(1), C.c_long(0), C.c_long(4), out.ctypes.data_as(dp)) == -1
    assert np.all(out == 0.0)


@pytest.mark.parametrize("seed,block", [(0, 0), (1, 0), (42, 1), (42, 3), (2 ** 63 + 5, 7), (12345, (2 ** 32 + 1) // 4),
                                        (7, 2 ** 64 - 1)])
def test_numpy_philox_counter_convention(seed, block):
    """numpy.random.Philox(key=k, counter=c) produces block c + 1 first (it increments before it generates): the restatement sets
    the counter one below the block it wants, and agrees with the published round function on fixed key / counter pairs."""
    assert pr.philox_block(seed, block) == pr.philox_rounds(seed, block)
    g = np.random.Philox(key=np.array([seed & pr.MASK64, 0], dtype=np.uint64),
                         counter=np.array([block & pr.MASK64, 0, 0, 0], dtype=np.uint64))
    if block < pr.MASK64:      # (block + 1 would carry into the second counter word, which philox_rounds keeps at 0)
        assert [int(v) for v in g.random_raw(4)] == pr.philox_rounds(seed, block + 1)


def test_known_answer_of_the_round_function():
    """Random123's known-answer vector for philox4x64-10 (counter 0, key 0): kat_vectors, 'philox4x64 10'."""
    assert [hex(v) for v in pr.philox_rounds(0, 0)] == ["0x16554d9eca36314c", "0xdb20fe9d672d0fdc", "0xd7e772cee186176b",
                                                        "0x7e68b68aec7ba23b"]


def test_normal_restatement_layout():
    """Four normals per block in the order r01 cos, r01 sin, r23 cos, r23 sin; a window at any offset is a slice of the stream."""
    z = pr.normals(9, 0, 12)
    x = pr.philox_block(9, 1)
    r01 = np.sqrt(-2.0 * np.log(pr.uniform(x[0])))
    r23 = np.sqrt(-2.0 * np.log(pr.uniform(x[2])))
    th01, th23 = 2 * np.pi * pr.uniform(x[1]), 2 * np.pi * pr.uniform(x[3])
    assert z[4:8].tolist() == [r01 * np.cos(th01), r01 * np.sin(th01), r23 * np.cos(th23), r23 * np.sin(th23)]
    assert pr.normals(9, 5, 6).tolist() == z[5:11].tolist()


@pytest.mark.parametrize("kernel", [pr.SE, pr.MATERN52])
def test_row_subset_posterior_equals_the_full_posterior(kernel):
    """posterior_rows (the reference of the M = 8191 / 8192 covariance tests) against posterior at M = 300."""
    D, N, M, b = 5, 40, 300, 0.01
    rng = np.random.default_rng(21 + kernel)
    X, Xs = rng.uniform(0, 1, (D, N)), rng.uniform(0, 1, (D, M))
    y = np.sin(2 * X.sum(0))
    theta = np.concatenate([[0.5], rng.uniform(0.3, 0.6, D)])
    rows = pr.pick_rows(M, 32, seed=3, always=(0, 127, 128, 299, 300, 8191))
    assert rows.size == 32 and np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == 299
    assert {0, 127, 128, 299} <= set(rows.tolist()) and rows.max() < M
    assert np.array_equal(rows, pr.pick_rows(M, 32, seed=3, always=(0, 127, 128, 299, 300, 8191)))
    mu, cov, _ = pr.posterior(X, y, Xs, theta, b, kernel)
    mu_r, cov_r = pr.posterior_rows(X, y, Xs, theta, b, kernel, rows)
    assert cov_r.shape == (32, M)
    # the same factor and the same triangular solve; only the blocking of the products differs
    assert np.abs(cov_r - cov[rows]).max() <= 1e-14 * theta[0] * N
    assert np.abs(mu_r - mu[rows]).max() <= 1e-14 * (np.abs(mu).max() + theta[0]) * N


def test_sample_chunk_rule():
    """The host rule of sls_gp_sample_posterior as the GPU tests restate it: 4096 samples per pass at M = 4096, 2048 at 8192."""
    assert pr.sample_chunk(4096) == 4096 and pr.sample_chunk(8192) == 2048 and pr.sample_chunk(128) == 131072
    assert pr.sample_chunk(3 * 128) == (2 ** 24 // 384) // 128 * 128 and pr.sample_chunk(2 ** 24) == 128
    src = open(os.path.join(ROOT, "sequential-line-search_amd", "csrc", "capi_post.hip")).read()
    assert "std::max(128, ((1 << 24) / Mp) / 128 * 128)" in src
