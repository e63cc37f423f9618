// The exact velocity and Q derivatives of a visco-acoustic problem on the 2-D MiniZephyr operator (HelmBaseProblem.JvecBorn / Jtvec / Hvec with parameter 'c', 'Q',
// 'cQ' on a Helm2DViscoProblem), each kernel beside the C entry point that launches it.  The wrapper makes the complex velocity of frequency f from the real
// velocity c and the quality factor Q of a cell,
//     c~ = c (1 + lam q) (1 + i q / 2),     q = 1 / Q,     lam = ln(f / freqBase) / pi   (0 without dispersion),
// and with an explicit density every coefficient of the operator is a holomorphic function of c~.  So the derivative of A along real (dc, dQ) is the derivative
// along the COMPLEX perturbation dc~ = gamma dc + chi dQ,
//     gamma = d c~ / d c = (1 + lam q) (1 + i q / 2),      chi = d c~ / d Q = -c~ q^2 [ lam / (1 + lam q) + (i / 2) / (1 + i q / 2) ],
// and both gradients come out of one back-propagation: g_c = Re sum_f gamma_f t_f, g_Q = Re sum_f chi_f t_f with t_f the complex cell gradient with respect to c~.
// The chain is computed here from the handle's own c~ (d_c), a float64 Q array and the scalar lam: nothing model-sized goes up per frequency.  Q = inf is q = 0:
// gamma = 1 and chi = 0 with no infinity in any product.  One lane per cell, one writer per entry, a fixed order: the same bits on every run.
#include "survey_internal.hpp"

struct ViscoChain { cplx gamma, chi; };
__device__ __forceinline__ ViscoChain visco_chain(cplx ct, double Q, double lam) {
    const double q = 1.0 / Q;
    const double disp = 1.0 + lam * q;
    const cplx att = cmake(1.0, 0.5 * q);
    ViscoChain ch;
    ch.gamma = cscale(att, disp);
    cplx br = cdiv(cmake(0.0, 0.5), att);
    br.x += lam / disp;
    const double q2 = q * q;
    ch.chi = cneg(cmul(ct, cscale(br, q2)));
    return ch;
}

// dcz[i] = gamma_i vc[i] + chi_i vQ[i]: the perturbation of the complex velocity that goes with real perturbations of c and of Q.  Either of vc, vQ may be NULL.
__global__ __launch_bounds__(256) void k_visco_perturbation(long long N, const cplx *__restrict__ c, const double *__restrict__ Q, double lam, const double *__restrict__ vc,
                                                            const double *__restrict__ vQ, cplx *__restrict__ dcz) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const ViscoChain ch = visco_chain(c[i], Q[i], lam);
    cplx out = cmake(0.0, 0.0);
    if (vc) out = cscale(ch.gamma, vc[i]);
    if (vQ) { const double v = vQ[i]; out.x = fma(ch.chi.x, v, out.x); out.y = fma(ch.chi.y, v, out.y); }
    dcz[i] = out;
}

// dDcz[i] = gamma_i vc[i] + chi_i vQ[i] for i < N, the chain of the model the handle holds (its d_c is c~ of its frequency): dQ, dVc, dVq N float64 (dVc or dVq
// may be NULL, not both), lam the dispersion scalar of the frequency, dDcz N complex128.  Returns when dDcz is complete.
extern "C" int helm_visco_perturbation_device(helm_op *op, const void *dQ, double lam, const void *dVc, const void *dVq, void *dDcz) {
    helm_tuning_refresh();
    if (!op || !dQ || (!dVc && !dVq) || !dDcz) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_visco_perturbation_device")) return rc;
    if (((((uintptr_t)dQ) | ((uintptr_t)dVc) | ((uintptr_t)dVq)) & 7) || (((uintptr_t)dDcz) & 15) || !(lam == lam)) return HELM_ERR_ARG;
    const size_t rbytes = (size_t)op->N * 8, zbytes = (size_t)op->N * sizeof(cplx);
    if (ranges_overlap(dQ, rbytes, dDcz, zbytes) || (dVc && ranges_overlap(dVc, rbytes, dDcz, zbytes)) || (dVq && ranges_overlap(dVq, rbytes, dDcz, zbytes))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_visco_perturbation_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_visco_perturbation, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, (long long)op->N, (const cplx *)op->d_c, (const double *)dQ, lam,
                (const double *)dVc, (const double *)dVq, (cplx *)dDcz);
    return launched(op);
}

// dC = V[dc~]: the body of k_velocity_planes (survey_frechet.hip) with a complex perturbation of the row's own cell and of the nine neighbours, and no db -- the
// differentiated row factors and d kappa / dc are holomorphic in c, so they multiply dc~ as they multiply a real dc.  One lane per cell; an interior row reads
// only cells inside the grid.
__global__ __launch_bounds__(256) void k_velocity_planes_z(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ dcz,
                                                           cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    cplx out[9];
    if (iz == 0 || iz == P.nz - 1 || ix == 0 || ix == P.nx - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
    } else {
        MzRow drow = mz_row_dc_at(P, c, iz, ix);
        const cplx v0 = dcz[i];
        drow.X = cmul(drow.X, v0); drow.Z = cmul(drow.Z, v0); drow.px = cmul(drow.px, v0); drow.pz = cmul(drow.pz, v0);
        double bn[9];
        cplx Kn[9];
        const double b0 = 1.0 / rho[i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const long long j = i + (long long)sz * P.nx + sx;
                const double bj = 1.0 / rho[j];
                bn[mz_slot(sz, sx)] = (b0 + bj) / 2.0;
                Kn[mz_slot(sz, sx)] = cmul(cscale(mz_kappa_dc(P, c[j]), bj), dcz[j]);
            }
        mz_star(P, drow, bn, Kn, out);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// dC[9][N] = V[dc~] for the operator the handle holds (its c~ and rho, PML and the frequency of its last assembly): dDcz N complex128 (helm_visco_perturbation_device),
// dC 9 N complex128, boundary rows zero.  Returns when dC is complete.
extern "C" int helm_velocity_planes_z_device(helm_op *op, const void *dDcz, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDcz || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_velocity_planes_z_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dDcz) | ((uintptr_t)dC)) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dDcz, (size_t)op->N * sizeof(cplx), dC, (size_t)op->N * 9 * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_velocity_planes_z_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_velocity_planes_z, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const cplx *)dDcz,
                (cplx *)dC);
    return launched(op);
}

// Gc[j] += gamma_j T[j], GQ[j] += chi_j T[j] (CONJ: the conjugated chain): the transpose of k_visco_perturbation on an item's complex cell gradient T.  The survey
// pipelines hold the conjugates of the fields, so their T is the conjugate of t_f and they ask for CONJ; the real part is the caller's, after the sum over
// frequencies.  Either of Gc, GQ may be NULL.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_visco_chain_adjoint(long long N, const cplx *__restrict__ c, const double *__restrict__ Q, double lam, const cplx *__restrict__ T,
                                                             cplx *__restrict__ Gc, cplx *__restrict__ GQ) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    ViscoChain ch = visco_chain(c[j], Q[j], lam);
    if (CONJ) { ch.gamma = cconj(ch.gamma); ch.chi = cconj(ch.chi); }
    const cplx t = T[j];
    if (Gc) { cplx g = Gc[j]; cfma(g, ch.gamma, t); Gc[j] = g; }
    if (GQ) { cplx g = GQ[j]; cfma(g, ch.chi, t); GQ[j] = g; }
}

// dGc[j] += gamma_j T[j], dGq[j] += chi_j T[j] for j < N (conj != 0: conj(gamma), conj(chi)), the chain of the model the handle holds: dQ N float64, dT, dGc, dGq N
// complex128 (dGc or dGq may be NULL, not both).  The outputs must not overlap T, Q or each other.  Returns when they are complete.
extern "C" int helm_visco_chain_adjoint_device(helm_op *op, const void *dQ, double lam, const void *dT, int conj, void *dGc, void *dGq) {
    helm_tuning_refresh();
    if (!op || !dQ || !dT || (!dGc && !dGq)) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_visco_chain_adjoint_device")) return rc;
    if ((((uintptr_t)dQ) & 7) || ((((uintptr_t)dT) | ((uintptr_t)dGc) | ((uintptr_t)dGq)) & 15) || !(lam == lam)) return HELM_ERR_ARG;
    const size_t rbytes = (size_t)op->N * 8, zbytes = (size_t)op->N * sizeof(cplx);
    for (const void *g : {(const void *)dGc, (const void *)dGq})
        if (g && (ranges_overlap(dQ, rbytes, g, zbytes) || ranges_overlap(dT, zbytes, g, zbytes))) return HELM_ERR_ARG;
    if (dGc && dGq && ranges_overlap(dGc, zbytes, dGq, zbytes)) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_visco_chain_adjoint_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    if (conj) HELM_LAUNCH(k_visco_chain_adjoint<true>, grid, dim3(256), 0, op->stream, (long long)op->N, (const cplx *)op->d_c, (const double *)dQ, lam, (const cplx *)dT,
                          (cplx *)dGc, (cplx *)dGq);
    else HELM_LAUNCH(k_visco_chain_adjoint<false>, grid, dim3(256), 0, op->stream, (long long)op->N, (const cplx *)op->d_c, (const double *)dQ, lam, (const cplx *)dT,
                     (cplx *)dGc, (cplx *)dGq);
    return launched(op);
}
