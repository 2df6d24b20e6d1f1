// bb_solver_spectral.hip -- the spectral start of the 3D-structure solver, device resident
// (bb_solver_spectral_init / _tol): a block power iteration on B = -1/2 J (D o D) J whose
// products are the core's matvec sweep (launch_grad) summed over the ranks (exchange_sum), and
// whose N x 3 algebra is bb_spectral_kernels.h.  gfx950 only.
#include <math.h>

#include <algorithm>

#include "bb_solver_internal.h"
#include "bb_spectral_kernels.h"

using namespace bb::solver;

namespace {

// small dense helpers on the host (3 x 3, row-major)
void jacobi3(double *a, double *z) {   // a symmetric 3 x 3 -> eigenvalues on its diagonal, vectors in z
    for (int q = 0; q < 9; ++q) z[q] = (q % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
        if (off < 1e-300) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k * 3 + p], akq = a[k * 3 + q];
                    a[k * 3 + p] = c * akp - sn * akq;
                    a[k * 3 + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p * 3 + k], aqk = a[q * 3 + k];
                    a[p * 3 + k] = c * apk - sn * aqk;
                    a[q * 3 + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double zkp = z[k * 3 + p], zkq = z[k * 3 + q];
                    z[k * 3 + p] = c * zkp - sn * zkq;
                    z[k * 3 + q] = sn * zkp + c * zkq;
                }
            }
    }
}

template <typename T>
int spectral_init_t(TypeTag<T>, bb_solver *s, int n_iter, const double *v0, double tol, int *iters_done,
                    double *residual_out) {
    const int64_t n = s->L.n_bins, n_pad = s->L.n_pad, n3 = n_pad * 3;
    if (!s->d_mv_in) BB_TRY(bb::alloc_status(s->d_mv_in, (size_t)n3 * sizeof(T)));
    // V, Z: (n_pad,3) doubles; dS: 12 sums (the two host steps at the end); dP0 / dP1: the
    // per-workgroup partial sums a pass leaves for the next one (two buffers: a pass reads its
    // producer's while it writes its own); dF: rank-loss flag
    bb::DevBuf bV, bZ, bS, bP, bF;
    if (bV.alloc((size_t)n3 * 8) != hipSuccess || bZ.alloc((size_t)n3 * 8) != hipSuccess ||
        bS.alloc(24 * 8) != hipSuccess || bP.alloc((size_t)2 * kSpMaxGroups * 12 * 8) != hipSuccess ||
        bF.alloc(sizeof(int)) != hipSuccess)
        return bb::fail(BB_ERR_NOMEM, "bb_solver_spectral_init: out of device memory");
    double *dV = (double *)bV.p, *dZ = (double *)bZ.p, *dS = (double *)bS.p;
    double *dP0 = (double *)bP.p, *dP1 = dP0 + kSpMaxGroups * 12;
    int *dF = (int *)bF.p;
    hipStream_t st = s->stream;
    const dim3 gvec((unsigned)((n_pad + kSpWG - 1) / kSpWG)), bwg(kSpWG);
    const int groups = (int)std::min<int64_t>(kSpMaxGroups, (n_pad + kSpWG - 1) / kSpWG);
    const dim3 ggrp((unsigned)groups);
    const Affine3 ident = {{0, 0, 0}, {1, 0, 0, 0, 1, 0, 0, 0, 1}, 1.0};
    double sums[12];
    auto fetch_sums = [&]() -> int {
        BB_HIP_CHECK(hipStreamSynchronize(st));
        BB_HIP_CHECK(hipMemcpy(sums, dS, sizeof(sums), hipMemcpyDeviceToHost));
        return BB_OK;
    };
    // dZ (any basis of the subspace, its 12 sums in dP1) -> dV orthonormal by Cholesky-QR, twice
    // (the second pass removes what the first leaves at cond(Z)^2 * eps), and the sweep's
    // right-hand sides d_mv_in = (T)(V - mean V): two kernels, the 3 x 3 steps in their prologues
    auto orthonormalise = [&]() -> int {
        BB_HIP_CHECK(bb::launch(sp_affine_stats_kernel<double>, ggrp, bwg, 0, st, (const double *)dZ, dV,
                                n, n_pad, (const double *)dP1, groups, (int)kSpChol, 1.0, dF, dP0));
        BB_HIP_CHECK(bb::launch(sp_affine_centre_kernel<T>, gvec, bwg, 0, st, (const double *)dV, dV,
                                s->d_mv_in.as<T>(), n, n_pad, (const double *)dP0, groups, dF));
        return BB_OK;
    };
    // dZ = -1/2 J (D o D) J V  (J = I - 11'/n) from the centred V in d_mv_in: sweep, sum over
    // the ranks, centre; the 12 sums of dZ are left in dP1
    auto apply_B = [&]() -> int {
        BB_TRY(launch_grad(s, kOpMatvec2, s->d_mv_in.p));
        BB_TRY(exchange_sum(s));
        BB_HIP_CHECK(bb::launch(sp_stats_kernel<T>, ggrp, bwg, 0, st, (const T *)s->d_exch, n, n_pad, dP0));
        BB_HIP_CHECK(bb::launch(sp_affine_stats_kernel<T>, ggrp, bwg, 0, st, (const T *)s->d_exch, dZ, n,
                                n_pad, (const double *)dP0, groups, (int)kSpMean, -0.5, dF, dP1));
        return BB_OK;
    };
    BB_HIP_CHECK(hipMemsetAsync(dF, 0, sizeof(int), st));
    BB_HIP_CHECK(hipMemsetAsync(s->d_V, 0, (size_t)n3 * sizeof(T), st));   // exchange_sum reads it
    BB_HIP_CHECK(upload_padded(s, dZ, v0, st));
    BB_HIP_CHECK(bb::launch(sp_stats_kernel<double>, ggrp, bwg, 0, st, (const double *)dZ, n, n_pad, dP1));
    BB_TRY(orthonormalise());
    // tol > 0: after every product but the first (a random V cannot have converged), the
    // relative distance of Z = B V from span(V), ||Z - V (V^T Z)||_F / ||Z||_F -- from the
    // Gram matrix V^T Z and the sums of Z^T Z the product left in dP1: V is orthonormal, so
    // the squared distance is ||Z||_F^2 - ||V^T Z||_F^2 (the difference of two sums resolves
    // a ratio down to about 1e-7).  Below tol the loop ends; the product just made is the
    // Rayleigh-Ritz step's.  Costs two small kernels and a read of 24 doubles per product.  Every
    // rank holds the same V and Z bit for bit (the summed products are identical on all
    // ranks), so all ranks leave at the same product.
    double zsums[12];
    double residual = -1.0;
    int done = 0;
    bool have_product = false;
    for (int it = 0; it < n_iter; ++it) {
        BB_TRY(apply_B());
        if (tol > 0.0 && it > 0) {
            BB_HIP_CHECK(bb::launch(gram3_kernel<double, double>, dim3(1), dim3(1024), 0, st,
                                    (const double *)dV, (const double *)dZ, n, dS));
            BB_HIP_CHECK(bb::launch(sp_fold_partials_kernel, dim3(1), dim3(64), 0, st,
                                    (const double *)dP1, groups, dS + 12));
            BB_TRY(fetch_sums());
            BB_HIP_CHECK(hipMemcpy(zsums, dS + 12, sizeof(zsums), hipMemcpyDeviceToHost));
            double gg = 0.0;
            const double zz = zsums[0] + zsums[4] + zsums[8];
            for (int q = 0; q < 9; ++q) gg += sums[q] * sums[q];
            residual = zz > 0.0 ? sqrt(std::max(0.0, zz - gg) / zz) : 0.0;
            if (residual < tol) { have_product = true; break; }
        }
        BB_TRY(orthonormalise());
        done = it + 1;
    }
    if (iters_done) *iters_done = done;
    if (residual_out) *residual_out = residual;
    // Rayleigh-Ritz on span(V): M = sym(V^T B V), X0 = V E sqrt(max(lambda, 0)).  From here on
    // the host takes part: three reads of 12 doubles for the whole start.
    if (!have_product) {
        BB_TRY(apply_B());
        BB_HIP_CHECK(bb::launch(gram3_kernel<double, double>, dim3(1), dim3(1024), 0, st,
                                (const double *)dV, (const double *)dZ, n, dS));
        BB_TRY(fetch_sums());
    }
    int lost = 0;
    BB_HIP_CHECK(hipMemcpy(&lost, dF, sizeof(int), hipMemcpyDeviceToHost));
    if (lost)
        return bb::fail(BB_ERR_STATE, "bb_solver_spectral_init: the iterate lost rank "
                                      "(fewer than 3 independent directions in the map)");
    double m[9], z[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i * 3 + j] = 0.5 * (sums[i * 3 + j] + sums[j * 3 + i]);
    jacobi3(m, z);
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return m[a * 4] > m[b * 4]; });
    // An eigenvector's sign is arbitrary: every Ritz vector V z_c is turned to the side of
    // the start's first column p (p . V z_c >= 0), as solver.py's spectral_init does, so one
    // seed gives one start whichever of the two computed it.
    BB_HIP_CHECK(upload_padded(s, dZ, v0, st));
    BB_HIP_CHECK(bb::launch(gram3_kernel<double, double>, dim3(1), dim3(1024), 0, st, (const double *)dV,
                            (const double *)dZ, n, dS));
    BB_TRY(fetch_sums());                                  // sums[r * 3 + 0] = V[:, r] . p
    Affine3 f = ident;
    for (int c = 0; c < 3; ++c) {
        const double lam = m[order[c] * 4] > 0.0 ? m[order[c] * 4] : 0.0;
        double side = 0.0;
        for (int r = 0; r < 3; ++r) side += z[r * 3 + order[c]] * sums[r * 3];
        const double sg = side < 0.0 ? -1.0 : 1.0;
        for (int r = 0; r < 3; ++r) f.m[r * 3 + c] = sg * z[r * 3 + order[c]] * sqrt(lam);
    }
    BB_HIP_CHECK(bb::launch(affine3_kernel<double, T>, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0,
                            st, (const double *)dV, (T *)s->d_X, n, n_pad, f));
    BB_HIP_CHECK(hipMemsetAsync(s->d_V, 0, (size_t)n3 * sizeof(T), st));
    BB_HIP_CHECK(hipStreamSynchronize(st));
    return BB_OK;
}

}  // namespace

extern "C" int bb_solver_spectral_init_tol(bb_solver *s, int n_iter, double tol, const double *v0,
                                           int *iters_done, double *residual);
extern "C" int bb_solver_spectral_init(bb_solver *s, int n_iter, const double *v0) {
    return bb_solver_spectral_init_tol(s, n_iter, 0.0, v0, nullptr, nullptr);
}
extern "C" int bb_solver_spectral_init_tol(bb_solver *s, int n_iter, double tol, const double *v0,
                                           int *iters_done, double *residual) {
    BB_REQUIRE(s != nullptr && v0 != nullptr, "bb_solver_spectral_init: NULL argument");
    BB_REQUIRE(n_iter >= 0 && n_iter <= 100000, "bb_solver_spectral_init: bad n_iter");
    BB_REQUIRE(tol >= 0.0 && tol < 1.0, "bb_solver_spectral_init: need 0 <= tol < 1");
    if (!s->have_wish) return bb::fail(BB_ERR_STATE, "bb_solver_spectral_init: no wish distances set");
    if (s->world != 1 && !s->peer.connected && !s->comm)
        return bb::fail(BB_ERR_STATE, "bb_solver_spectral_init: with world > 1 the ranks need their "
                                      "exchange first (bb_solver_peer_connect, or bb_solver_comm_init "
                                      "/ _attach); without one the caller sums bb_solver_matvec_sq "
                                      "over the ranks");
    if (s->grad_pending)
        return bb::fail(BB_ERR_STATE, "bb_solver_spectral_init: a bb_solver_grad is pending");
    if (s->n_maps > 1)
        return bb::fail(BB_ERR_STATE, "bb_solver_spectral_init: not for a solver of several maps "
                                      "(start each map with a solver of its own)");
    BB_REQUIRE(s->L.n_bins >= 3, "bb_solver_spectral_init: needs at least 3 bins");
    BB_TRY(bb::enter_device(s->device));
    BB_TRY(by_dtype(s, [&](auto t) { return spectral_init_t(t, s, n_iter, v0, tol, iters_done, residual); }));
    s->have_coords = true;
    s->hist_n = 0;
    s->grad_pending = false;
    return BB_OK;
}
