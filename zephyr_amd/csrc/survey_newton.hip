// What the full Newton Hessian-vector product of the exact MiniZephyr derivatives (HelmBaseProblem.Hvec with resid=) adds to the kernels of survey_frechet.hip,
// each beside the C entry point that launches it: the second derivative of the operator contracted with nine lag products (k_velocity_curvature), and the
// TRANSPOSED application of a set of perturbation planes to stored columns (k_stencil_sources_t), and the planes of the mass term alone (k_mass_planes).  The walk, the readers of a stored field and the row factors
// at a cell are in survey_internal.hpp.
//
// With lambda = A^-T (back-source of the residual), du = -A^-1 dA[p] u and dlambda = A^-T (R^H R du - dA[p]^T lambda),
//     (H p)_i = -Re[ <dlambda, d_i A u> + <lambda, d_i A du> + <lambda, (d_i dA[p]) u> ].
// The first two terms are k_velocity_adjoint / k_buoyancy_adjoint on the lag products of (dlambda, u) and (lambda, du); dA[p]^T lambda is k_stencil_sources_t; the
// third term is k_velocity_curvature on the lag products of (lambda, u).
#include "survey_internal.hpp"

// ------------------------------------------------------------------------------------------
// the second derivative of the operator along (p, e_j), contracted with the lag products
// ------------------------------------------------------------------------------------------
// With an explicit density a row is mz_star(row_i(c_i), bn, Kn_k = kappa(c_j) b_j), and mz_star has no product of a row factor with a mass term: d^2 A / dc_i dc_j = 0
// for i != j, and the second derivative along (p, e_j) is p_j mz_star(d^2 row_j / dc^2, bn[b], Kn = (d^2 kappa_j / dc^2) b_j) in the rows that see cell j.  So
//     G[j] += w p[j] [ (d^2 kappa_j / dc^2) b_j (the mass gather of P over the interior rows i = j - o) + (the stretch part of row j with d^2 row_j / dc^2) ]
// k_velocity_adjoint with the twice-differentiated factors: both are mz_transpose_at (survey_internal.hpp), of order 1 and 2.  One lane per cell j, one writer per
// cell, a fixed order, no atomics, no scratch; the boundary rows of P are not read.  STRETCH false: the mass term alone (linearisation='operator').  CONJ: the conjugated coefficients.
template <bool CONJ, bool STRETCH>
__global__ __launch_bounds__(256) void k_velocity_curvature(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ Pl,
                                                            const double *__restrict__ p, cplx w, cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const cplx sum = cscale(mz_transpose_at<2, CONJ, STRETCH>(P, c, rho, Pl, j), p[j]);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w p[j] sum_(k, i) (d^2 A / dc_j^2)_(k, i) P_k[i] for j < N (conj != 0: the conjugated coefficients; stretch == 0: the mass term alone) for the operator
// the handle holds, at the density it assembled with: P [9][N] complex128 (its boundary rows are not read), p N float64, G N complex128.  G must not overlap P or
// p.  Returns when G is complete.
extern "C" int helm_velocity_curvature_device(helm_op *op, const void *dP, const void *dp, double w_re, double w_im, int conj, int stretch, void *dG) {
    helm_tuning_refresh();
    if (!op || !dP || !dp || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_velocity_curvature_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15) || (((uintptr_t)dp) & 7)) return HELM_ERR_ARG;
    const size_t gbytes = (size_t)op->N * sizeof(cplx);
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, gbytes) || ranges_overlap(dp, (size_t)op->N * 8, dG, gbytes)) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_velocity_curvature_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    const cplx w = cmake(w_re, w_im);
#define CURVATURE(CJ, ST) HELM_LAUNCH((k_velocity_curvature<CJ, ST>), grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, \
                                      (const cplx *)dP, (const double *)dp, w, (cplx *)dG)
    if (conj && stretch) CURVATURE(true, true);
    else if (conj) CURVATURE(true, false);
    else if (stretch) CURVATURE(false, true);
    else CURVATURE(false, false);
#undef CURVATURE
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the planes of the mass term alone (linearisation='operator')
// ------------------------------------------------------------------------------------------
// dC_k[i] = m_k (d kappa_j / dc) b_j dc_j, j = i + off_k, on the interior rows, zero on the boundary rows: k_velocity_planes without the stretch part, the planes
// whose application to a column is k_virtual_sources_op.  The Newton product needs them as planes, for the transposed application.  One lane per cell.
__global__ __launch_bounds__(256) void k_mass_planes(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ dc,
                                                     cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    const bool inside = iz >= 1 && iz <= P.nz - 2 && ix >= 1 && ix <= P.nx - 2;
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            cplx out = cmake(0.0, 0.0);
            if (inside) {                                        // (an interior row has every neighbour inside the grid)
                const long long j = i + (long long)sz * P.nx + sx;
                const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
                out = cscale(mz_kappa_dc(P, c[j]), m * (dc[j] / rho[j]));
            }
            C[(long long)mz_slot(sz, sx) * N + i] = out;
        }
}

// dC[9][N] = the mass term of helm_velocity_planes_device alone, for the operator the handle holds: dc N float64, dC 9 N complex128, boundary rows zero.  Returns
// when dC is complete.
extern "C" int helm_mass_planes_device(helm_op *op, const void *dDc, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDc || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_mass_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dDc) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dDc, (size_t)op->N * 8, dC, (size_t)op->N * 9 * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_mass_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_mass_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const double *)dDc,
                (cplx *)dC);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the transposed application of a plane set
// ------------------------------------------------------------------------------------------
// (dA u)[i] = sum_k C_k[i] u[i + off_k], so ((dA)^T v)[j] = sum_k C_(8-k)[j + off_k] v[j + off_k]: the stencil of k_stencil_sources with plane 8 - k read at the
// NEIGHBOURING cell j + off_k, nothing where that cell is outside the grid.  The transposed plane set is never formed in memory.  The boundary rows of a dC made by
// k_velocity_planes / k_buoyancy_planes are zero, so the boundary columns of the transpose get nothing; the kernel reads whatever planes it is given.
// R[s ldr + j] = coef sum_k (CONJ ? conj(C_(8-k)) : C_(8-k))[j + off_k] U[s][j + off_k] for the nsrc columns: (dC)^T U, or (dC)^H U with CONJ.  The walk, the column
// blocking and the store formats of k_stencil_sources; the nine (shifted) plane values are read once per group of columns.  The sum runs k = 0 .. 8: the same bits
// on every run.  accumulate != 0: R += the CONJUGATE of that value -- the columns a pipeline holds are the conjugates of the fields, and the right-hand side of the
// third solve of the Newton product is the gathered samples plus conj(coef (dC)^H lambda~), so the result goes where it is needed without a block of its own.
template <class F, bool CONJ>
__global__ __launch_bounds__(256) void k_stencil_sources_t(F U, int nsrc, long long ldu, const cplx *__restrict__ C, cplx coef, cplx *__restrict__ R, long long ldr,
                                                           int nz, int nx, int accumulate) {
    const OpJob job(nz, nx);
    if (!job.live) return;                                  // (a whole wave: the lane exchanges below stay complete)
    const long long N = (long long)nz * nx;
    const int s0 = blockIdx.y * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
    const int x = job.x;
    typename F::raw raw[OP_UNROLL];
    LagRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    double sc[OP_UNROLL];
#pragma unroll
    for (int j = 0; j < OP_UNROLL; ++j) sc[j] = U.scale(s0 + min(j, ncol - 1));
    auto fetch = [&](int z) {
        const bool in = job.xin && z >= 0 && z < nz;
        const long long i = (long long)z * nx + x;
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) raw[j] = (in && j < ncol) ? U.load((long long)(s0 + j) * ldu + i) : typename F::raw{};
    };
    auto make = [&](LagRow *row) {
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) {
            const cplx u = U.scaled(raw[j], sc[j]);
            row[j].t = u;
            lane_left_right(u, row[j].l, row[j].r);
        }
    };
    fetch(job.z0 - 1); make(up);
    fetch(job.z0); make(mid);
    fetch(job.z0 + 1);
    for (int z = job.z0; z < job.z1; ++z) {
        make(dn);
        if (z + 1 < job.z1) fetch(z + 2);                  // (wave-uniform)
        if (job.store) {                                    // (0 <= x < nx and 0 <= z < nz here)
            const long long i = (long long)z * nx + x;
            cplx ck[9];
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int k = mz_slot(dz, dx);
                    const bool in = z + dz >= 0 && z + dz < nz && x + dx >= 0 && x + dx < nx;      // (the neighbouring cell is inside the grid: the load is in bounds)
                    cplx v = in ? C[(long long)(8 - k) * N + i + (long long)dz * nx + dx] : cmake(0.0, 0.0);
                    if (CONJ) v = cconj(v);
                    ck[k] = v;
                }
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j)
                if (j < ncol) {
                    cplx acc = cmake(0.0, 0.0);
                    cfma(acc, ck[0], up[j].l); cfma(acc, ck[1], up[j].t); cfma(acc, ck[2], up[j].r);
                    cfma(acc, ck[3], mid[j].l); cfma(acc, ck[4], mid[j].t); cfma(acc, ck[5], mid[j].r);
                    cfma(acc, ck[6], dn[j].l); cfma(acc, ck[7], dn[j].t); cfma(acc, ck[8], dn[j].r);
                    const cplx v = cmul(coef, acc);
                    cplx *r = R + (long long)(s0 + j) * ldr + i;
                    *r = accumulate ? cadd(*r, cconj(v)) : v;                 // (wave-uniform)
                }
        }
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
    }
}

// R[s][j] = coef sum_k C_(8-k)[j + off_k] U[s][j + off_k] (conj != 0: conj(C)) for s < nsrc, j < N (the handle's nz x nx grid): U [nsrc][ldu] complex128, C [9][N]
// complex128 (helm_velocity_planes_device, helm_buoyancy_planes_device, helm_mass_planes_device), R [nsrc][ldr] complex128, ldu, ldr >= N; accumulate != 0: the
// conjugate of that value is added to R.  R must not overlap U or C.  Returns when R is complete.
static int stencil_sources_t_launch(helm_op *op, HostField U, int nsrc, long long ldu, const void *dC, cplx coef, int conj, int accumulate, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !U.u || !dC || !dR || nsrc < 1 || nsrc > 65535 * OP_UNROLL || ldu < op->N || ldr < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_stencil_sources_t_device")) return rc;       // (both entry points refuse under this name)
    if (op->nz < 3 || op->nx < 3) return HELM_ERR_ARG;
    const size_t rbytes = (size_t)nsrc * ldr * sizeof(cplx);
    if (ranges_overlap(U.u, U.bytes(nsrc, ldu), dR, rbytes) || ranges_overlap(dC, (size_t)op->N * 9 * sizeof(cplx), dR, rbytes)) return HELM_ERR_ARG;
    if (!U.ok() || ((((uintptr_t)dC) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle; 16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    return U.with([&](auto F) {
        if (conj) HELM_LAUNCH((k_stencil_sources_t<decltype(F), true>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dC, coef, (cplx *)dR, ldr, op->nz, op->nx, accumulate);
        else HELM_LAUNCH((k_stencil_sources_t<decltype(F), false>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dC, coef, (cplx *)dR, ldr, op->nz, op->nx, accumulate);
        return launched(op);
    });
}
extern "C" int helm_stencil_sources_t_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im, int conj,
                                             int accumulate, void *dR, long long ldr) {
    return stencil_sources_t_launch(op, HostField::c128(dU), nsrc, ldu, dC, cmake(coef_re, coef_im), conj, accumulate, dR, ldr);
}
extern "C" int helm_stencil_sources_t_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im,
                                                 int conj, int accumulate, void *dR, long long ldr) {
    return stencil_sources_t_launch(op, HostField::packed(dU32, dExp), nsrc, ldu, dC, cmake(coef_re, coef_im), conj, accumulate, dR, ldr);
}
