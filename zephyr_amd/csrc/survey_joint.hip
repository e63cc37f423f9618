// What the joint (c, rho) Newton Hessian-vector product (HelmBaseProblem.Hvec with parameter='joint' and resid=) adds to the kernels of survey_frechet.hip and
// survey_newton.hip, each beside the C entry point that launches it: the two transposes of the mixed second derivative of the 2-D MiniZephyr operator with respect to
// the velocity and the buoyancy.  The row factors at a cell and the body the velocity transposes share are in survey_internal.hpp.
//
// A row is mz_star(row_i(c_i), bn[b], Kn_k = kappa(c_j) b_j): bilinear in (row, bn) and linear in Kn, so d^2 A / db^2 = 0 and along a velocity perturbation p and a
// buoyancy perturbation beta
//     d^2 A / dc db [p, beta] = mz_star(p_i d row_i / dc, bn[beta], Kn_k = (d kappa_j / dc) beta_j p_j)
// -- the planes of k_velocity_planes with beta in the place of the buoyancy.  Contracted with the lag products P0 of (lambda, u), the gradient's own, its transpose in p
// joins the velocity half of the product (k_velocity_adjoint_b) and its transpose in beta the buoyancy half (k_mixed_adjoint).
#include "survey_internal.hpp"

// ------------------------------------------------------------------------------------------
// the transpose in the velocity: k_velocity_adjoint at a buoyancy read from an array
// ------------------------------------------------------------------------------------------
// G[j] += w sum_(k, i) (d / dp_j of the planes above)_(k, i) P_k[i]: mz_transpose_at of order 1 with B[j] where k_velocity_adjoint has 1 / rho[j].  B is a
// perturbation: any sign, zeros included, so it is read as it is and never inverted.  One lane per cell j, one writer per cell, a fixed order, no atomics, no scratch;
// the boundary rows of P are not read.  STRETCH false: the mass term alone (linearisation='operator').  CONJ: the conjugated coefficients.
template <bool CONJ, bool STRETCH>
__global__ __launch_bounds__(256) void k_velocity_adjoint_b(MzParams P, const cplx *__restrict__ c, const double *__restrict__ B, const cplx *__restrict__ Pl, cplx w,
                                                            cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const cplx sum = mz_transpose_at<1, CONJ, STRETCH, true>(P, c, B, Pl, j);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// what both entry points check before they launch: P [9][N] complex128, a real field of N float64, G N complex128 that overlaps neither
static int joint_args(helm_op *op, const char *what, const void *dP, const void *dv, void *dG, MzParams *P) {
    helm_tuning_refresh();
    if (!op || !dP || !dv || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, what)) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15) || (((uintptr_t)dv) & 7)) return HELM_ERR_ARG;
    const size_t gbytes = (size_t)op->N * sizeof(cplx);
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, gbytes) || ranges_overlap(dv, (size_t)op->N * 8, dG, gbytes)) return HELM_ERR_ARG;
    if (helm_mz_params(op, P)) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no assembled operator", what);
    HIP_TRY(op, hipSetDevice(op->device));
    return HELM_OK;
}

// G[j] += w sum_(k, i) (V at the buoyancy B)_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients; stretch == 0: the mass term alone), V the map of
// helm_velocity_planes_device for the operator the handle holds with B in the place of 1 / rho: P [9][N] complex128 (its boundary rows are not read), B N float64 of
// any sign, G N complex128.  G must not overlap P or B.  Returns when G is complete.
extern "C" int helm_velocity_adjoint_b_device(helm_op *op, const void *dP, const void *dB, double w_re, double w_im, int conj, int stretch, void *dG) {
    MzParams P;
    if (int rc = joint_args(op, "helm_velocity_adjoint_b_device", dP, dB, dG, &P)) return rc;
    const dim3 grid((unsigned)((op->N + 255) / 256));
    const cplx w = cmake(w_re, w_im);
#define VADJOINT_B(CJ, ST) HELM_LAUNCH((k_velocity_adjoint_b<CJ, ST>), grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)dB, (const cplx *)dP, w, (cplx *)dG)
    if (conj && stretch) VADJOINT_B(true, true);
    else if (conj) VADJOINT_B(true, false);
    else if (stretch) VADJOINT_B(false, true);
    else VADJOINT_B(false, false);
#undef VADJOINT_B
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the transpose in the buoyancy: the gather of k_buoyancy_adjoint with the differentiated factors of every row
// ------------------------------------------------------------------------------------------
// G[j] += w sum_(k, i) (d / dbeta_j of the planes above)_(k, i) P_k[i], a gather over the interior rows i = j - o of the 3 x 3 block around cell j as in
// k_buoyancy_adjoint, with the stiffness factors of ROW i those of p_i d row_i / dc (mz_stiffness is linear in the row: the factor p_i multiplies the row's sum) and
// kappa_j replaced by (d kappa_j / dc) p_j.  Row i holds beta_j three ways: in the mass term of the lag o; in the average (beta_i + beta_j) / 2 of that lag; and, for
// i = j, in all eight averages.  This is the piece that is not local: cell j sees p at the eight rows around it and at its own.  STRETCH false: the mass term
// alone, which is local.  One lane per cell, one writer per cell, a fixed order, no atomics, no scratch; the boundary rows of P are not read.
template <bool CONJ, bool STRETCH>
__global__ __launch_bounds__(256) void k_mixed_adjoint(MzParams P, const cplx *__restrict__ c, const cplx *__restrict__ Pl, const double *__restrict__ p, cplx w,
                                                       cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int jz = (int)(j / P.nx), jx = (int)(j % P.nx);
    cplx mass = cmake(0.0, 0.0), avg = cmake(0.0, 0.0);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int iz = jz - sz, ix = jx - sx;                 // row i sees cell j at the lag (sz, sx)
            if (iz < 1 || iz > P.nz - 2 || ix < 1 || ix > P.nx - 2) continue;
            const long long i = (long long)iz * P.nx + ix;
            const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
            const cplx pl = Pl[(long long)mz_slot(sz, sx) * N + i];
            mass.x += m * pl.x; mass.y += m * pl.y;
            if (STRETCH) {
                const MzStiff t = mz_stiffness<CONJ>(P, mz_row_dc_at(P, c, iz, ix));
                cplx q = cmake(0.0, 0.0);
                if (sz == 0 && sx == 0) {
#pragma unroll
                    for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
                        for (int ox = -1; ox <= 1; ++ox)
                            if (oz != 0 || ox != 0) q = cadd(q, lag_coefficient(t, Pl, N, i, oz, ox));
                } else q = lag_coefficient(t, Pl, N, i, sz, sx);
                avg = cadd(avg, cscale(q, p[i]));
            }
        }
    cplx dk = cscale(mz_kappa_dc(P, c[j]), p[j]);
    if (CONJ) dk = cconj(dk);
    cplx sum = cscale(avg, 0.5);
    cfma(sum, dk, mass);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w sum_(k, i) (d^2 A / dc db [p, e_j])_(k, i) P_k[i] for j < N (conj != 0: the conjugated coefficients; stretch == 0: the mass term alone) for the operator the
// handle holds: the transpose in the buoyancy of the mixed second derivative along the velocity perturbation p.  P [9][N] complex128 (its boundary rows are not
// read), p N float64 of any sign, G N complex128.  G must not overlap P or p.  Returns when G is complete.
extern "C" int helm_mixed_adjoint_device(helm_op *op, const void *dP, const void *dp, double w_re, double w_im, int conj, int stretch, void *dG) {
    MzParams P;
    if (int rc = joint_args(op, "helm_mixed_adjoint_device", dP, dp, dG, &P)) return rc;
    const dim3 grid((unsigned)((op->N + 255) / 256));
    const cplx w = cmake(w_re, w_im);
#define MIXED(CJ, ST) HELM_LAUNCH((k_mixed_adjoint<CJ, ST>), grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const cplx *)dP, (const double *)dp, w, (cplx *)dG)
    if (conj && stretch) MIXED(true, true);
    else if (conj) MIXED(true, false);
    else if (stretch) MIXED(false, true);
    else MIXED(false, false);
#undef MIXED
    return launched(op);
}
