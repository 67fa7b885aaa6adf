// Host side of the maps of a *_sub call (include/sls_hip.h "maximisation over affine subspaces"): validation before any launch, ONE
// upload per call, and the expand / fold launches under their profiler scopes (kernels_sub.hip).
#pragma once
#include <cmath>

#include "common.hpp"

namespace slsk {

// The maps of one call on the device: A | c | map_of_column in ONE pooled block
struct SubMapsDev {
    DBuf blk;
    SubMaps m;
};

// Every refusal of the contract, then the upload on the context's stream.  D: the handle's; ncols: the call's columns (points /
// starts), the length of map_of_column.
inline void upload_sub_maps(const char* who, sls_ctx* c, const sls_submaps* maps, int D, long ncols, SubMapsDev& up) {
    SLS_REQUIRE(maps != nullptr, "%s: maps is NULL", who);
    SLS_REQUIRE(maps->struct_size == (int)sizeof(sls_submaps), "%s: sls_submaps.struct_size = %d: expected %d", who, maps->struct_size,
                (int)sizeof(sls_submaps));
    const int d = maps->d, K = maps->n_maps;
    SLS_REQUIRE(d >= 1 && d <= D, "%s: sls_submaps.d = %d (1 .. D = %d)", who, d, D);
    SLS_REQUIRE(K >= 1, "%s: sls_submaps.n_maps = %d (>= 1)", who, K);
    SLS_REQUIRE(maps->A && maps->c, "%s: sls_submaps.A / c is NULL", who);
    const size_t nA = (size_t)K * D * d, nc = (size_t)K * D;
    for (size_t i = 0; i < nA; ++i) SLS_REQUIRE(std::isfinite(maps->A[i]), "%s: sls_submaps.A[%zu] is not finite", who, i);
    for (size_t i = 0; i < nc; ++i) SLS_REQUIRE(std::isfinite(maps->c[i]), "%s: sls_submaps.c[%zu] is not finite", who, i);
    if (maps->map_of_column)
        for (long i = 0; i < ncols; ++i)
            SLS_REQUIRE(maps->map_of_column[i] >= 0 && maps->map_of_column[i] < K, "%s: sls_submaps.map_of_column[%ld] = %d (n_maps = %d)",
                        who, i, maps->map_of_column[i], K);
    const size_t nints = maps->map_of_column && ncols > 0 ? (size_t)ncols : 0;
    up.blk.ensure(nA + nc + (nints + 1) / 2);
    h2d(c, up.blk.p, maps->A, nA);
    h2d(c, up.blk.p + nA, maps->c, nc);
    int* moc = reinterpret_cast<int*>(up.blk.p + nA + nc);
    if (nints) SLS_HIP(hipMemcpyAsync(moc, maps->map_of_column, nints * sizeof(int), hipMemcpyHostToDevice, c->stream));
    up.m.D = D; up.m.d = d; up.m.n_maps = K;
    up.m.A = up.blk.p; up.m.c = up.blk.p + nA; up.m.map_of_column = nints ? moc : nullptr;
}

inline void sub_expand(sls_ctx* c, const SubMaps& m, int ncols, const int* live, const double* z, long ld, double* X, long ldx) {
    ProfScope ps(c, "sub_expand");
    launch_sub_expand(c->stream, m, ncols, live, z, ld, X, ldx);
}
inline void sub_fold(sls_ctx* c, const SubMaps& m, int ncols, const int* live, const double* gx, long ldx, double* gz, long ldo) {
    ProfScope ps(c, "sub_fold");
    launch_sub_fold(c->stream, m, ncols, live, gx, ldx, gz, ldo);
}

// An objective at x = c + A z: expand the candidate-major variables z[n + j*ld] (n < count; column n is start live[n], nullptr:
// identity) into x (D x ld, grown here), inner(x, gx) -- the unchanged evaluation at the count points x[n + r*ld], its gradient into
// gx[n + r*ld] (nullptr: not asked for) --, then the fold of gx onto grad_z[n + j*ld] (may be nullptr).
// The expand pads the last 128-wide tile of the points with 0.5; gx is written by inner and read by the fold for n < count only.
template <class Inner>
void sub_eval(sls_ctx* c, const SubMaps& m, DBuf& x, DBuf& gx, const double* z, long ld, int count, const int* live, double* grad_z,
              Inner&& inner) {
    x.ensure((size_t)m.D * ld);
    if (grad_z) gx.ensure((size_t)m.D * ld);
    sub_expand(c, m, count, live, z, ld, x.p, ld);
    inner(x.p, grad_z ? gx.p : nullptr);
    if (grad_z) sub_fold(c, m, count, live, gx.p, ld, grad_z, ld);
}

}  // namespace slsk
