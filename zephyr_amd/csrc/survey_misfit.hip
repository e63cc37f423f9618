// The data misfit in data space (zephyr_amd/misfit.py states the functional): what turns the sample panel of a work item into the adjoint source that is
// back-propagated, without the panel leaving the device.  A panel is what the sampling kernels write, [nrec][ld] complex128 with the item's k columns
// adjacent (sample [r][j] at r * ld + j); dobs and the weights w2 are panels of the same leading dimension.  p = the sample, d = dobs, s = the source
// factor of the column, q = s p, r = q - d.
//
//   k_misfit_moments      per column  a_j = sum_r w2 conj(p) d,  b_j = sum_r w2 |p|^2           (the source estimate is a / b over the columns of a group)
//   k_misfit_terms<KIND>  the panel psi = grad_q phi and per column  phi_j,  c_j = sum_r conj(psi) p
//   k_misfit_adjoint      v = conj(s) psi + w2 (e_j d - f_j p)  [times a per-receiver phase], e_j = c / b and f_j = 2 Re(c s) / b of the column's group, in
//                         place of the sample panel; optionally the Gauss-Newton weight panel
//
// Every per-column sum is ONE lane walking r = 0, 1, ... upwards: the order depends on nrec alone, not on the launch geometry, on ncol or on where the column
// sits in the batch, so a column has the same bits alone, anywhere in a batch and on every run.  With the columns adjacent the 64 lanes of a wave read 1 KiB
// of consecutive bytes per row: the mapping is the coalesced one.  No atomics, no LDS.  A sample with w2 = 0 is selected away after it is computed (a NaN in
// its dobs never reaches a sum or a panel).  Contraction is off for the whole file and every operation is written out, so that the rounding count the tests
// hold these kernels to can be read off the code: a complex product is two products and a sum per component.
#include "survey_internal.hpp"
#pragma clang fp contract(off)

enum { MISFIT_L2 = 0, MISFIT_HUBER = 1, MISFIT_HYBRID = 2, MISFIT_LOG = 3 };
constexpr int MISFIT_LANES = 64;         // a wave per workgroup: 64 adjacent columns

__device__ __forceinline__ cplx mf_mul(cplx a, cplx b) { return cmake(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cplx mf_conjmul(cplx a, cplx b) { return cmake(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }      // conj(a) b
__device__ __forceinline__ double mf_abs2(cplx a) { return a.x * a.x + a.y * a.y; }

// phi and psi of one live sample (w > 0).  par0, par1: the threshold ('huber'), epsilon ('hybrid'), amplitude and phase weights ('logarithmic').
template <int KIND>
__device__ __forceinline__ cplx misfit_sample(cplx p, cplx d, cplx s, double w, double par0, double par1, double &phi) {
    const cplx q = mf_mul(s, p);
    if (KIND == MISFIT_LOG) {
        // rho = q / d = q conj(d) / |d|^2;  L = ln |rho| = ln(|rho|^2) / 2;  psi = w (alpha L + i beta theta) / conj(q) = w (alpha L + i beta theta) q / |q|^2
        const double d2 = mf_abs2(d), q2 = mf_abs2(q);
        const cplx n = mf_conjmul(d, q);
        const cplx rho = cmake(n.x / d2, n.y / d2);
        const double L = 0.5 * log(mf_abs2(rho)), th = atan2(rho.y, rho.x);
        const double aL = par0 * L, bt = par1 * th;
        phi = 0.5 * (w * (aL * L + bt * th));
        const cplx z = mf_mul(cmake(aL, bt), q);
        const double f = w / q2;
        return cmake(f * z.x, f * z.y);
    }
    const cplx r = cmake(q.x - d.x, q.y - d.y);
    const double r2 = mf_abs2(r);
    if (KIND == MISFIT_HUBER) {
        const double sw = sqrt(w), ar = sqrt(r2), a = sw * ar;
        const bool small = a <= par0;
        phi = small ? 0.5 * (a * a) : par0 * a - 0.5 * (par0 * par0);
        const double f = small ? w : par0 * sw / ar;
        return cmake(f * r.x, f * r.y);
    }
    if (KIND == MISFIT_HYBRID) {
        const double x = w * r2, root = sqrt(1.0 + x / (par0 * par0));
        phi = x / (1.0 + root);                          // eps^2 (root - 1) without the cancellation
        const double f = w / root;
        return cmake(f * r.x, f * r.y);
    }
    phi = 0.5 * (w * r2);
    return cmake(w * r.x, w * r.y);
}

// the Gauss-Newton weight of one live sample: the real diagonal W with d psi ~ W dq, times |s|^2 ('logarithmic', alpha == beta: alpha w2 / |p|^2)
template <int KIND>
__device__ __forceinline__ double misfit_gn_weight(cplx p, cplx d, cplx s, double w, double par0) {
    if (KIND == MISFIT_LOG) return par0 * w / mf_abs2(p);
    const double s2 = mf_abs2(s);
    if (KIND == MISFIT_L2) return s2 * w;
    const cplx q = mf_mul(s, p);
    const double r2 = mf_abs2(cmake(q.x - d.x, q.y - d.y));
    if (KIND == MISFIT_HUBER) {
        const double sw = sqrt(w), ar = sqrt(r2);
        return s2 * (sw * ar <= par0 ? w : par0 * sw / ar);
    }
    return s2 * (w / sqrt(1.0 + w * r2 / (par0 * par0)));
}

// mom[j] = (Re a_j, Im a_j, b_j): one lane per column, r upwards
__global__ __launch_bounds__(MISFIT_LANES) void k_misfit_moments(const cplx *__restrict__ P, const cplx *__restrict__ D, const double *__restrict__ W2, long long ld,
                                                                 int nrec, int ncol, double *__restrict__ mom) {
    const int j = blockIdx.x * MISFIT_LANES + threadIdx.x;
    if (j >= ncol) return;
    double ax = 0.0, ay = 0.0, b = 0.0;
    for (int r = 0; r < nrec; ++r) {
        const long long i = (long long)r * ld + j;
        const cplx p = P[i], d = D[i];
        const double w = W2 ? W2[i] : 1.0;
        const bool live = w > 0.0;
        const cplx t = mf_conjmul(p, d);
        ax += live ? w * t.x : 0.0;
        ay += live ? w * t.y : 0.0;
        b += live ? w * mf_abs2(p) : 0.0;
    }
    mom[3 * (long long)j] = ax;
    mom[3 * (long long)j + 1] = ay;
    mom[3 * (long long)j + 2] = b;
}

// PSI[r][j] = psi (0 where w2 = 0), out[j] = (phi_j, Re c_j, Im c_j): one lane per column, r upwards
template <int KIND>
__global__ __launch_bounds__(MISFIT_LANES) void k_misfit_terms(const cplx *__restrict__ P, const cplx *__restrict__ D, const double *__restrict__ W2,
                                                               const cplx *__restrict__ S, long long ld, int nrec, int ncol, double par0, double par1,
                                                               cplx *__restrict__ PSI, double *__restrict__ out) {
    const int j = blockIdx.x * MISFIT_LANES + threadIdx.x;
    if (j >= ncol) return;
    const cplx s = S[j];
    double phi = 0.0, cx = 0.0, cy = 0.0;
    for (int r = 0; r < nrec; ++r) {
        const long long i = (long long)r * ld + j;
        const cplx p = P[i], d = D[i];
        const double w = W2 ? W2[i] : 1.0;
        const bool live = w > 0.0;
        double f;
        const cplx psi = misfit_sample<KIND>(p, d, s, w, par0, par1, f);
        const cplx t = mf_conjmul(psi, p);
        phi += live ? f : 0.0;
        cx += live ? t.x : 0.0;
        cy += live ? t.y : 0.0;
        PSI[i] = live ? psi : cmake(0.0, 0.0);
    }
    out[3 * (long long)j] = phi;
    out[3 * (long long)j + 1] = cx;
    out[3 * (long long)j + 2] = cy;
}

// V[r][j] = phase[r] (conj(s_j) psi + w2 (e_j d - f_j p)), coef[j] = (Re e_j, Im e_j, f_j) (NULL: a given source, no second term); GN != NULL: the
// Gauss-Newton weight panel.  Elementwise: one thread per sample, and V may be the sample panel itself (a thread reads its p before it writes its v).
template <int KIND>
__global__ __launch_bounds__(256) void k_misfit_adjoint(const cplx *__restrict__ PSI, const cplx *__restrict__ S, const double *__restrict__ coef, const cplx *P,
                                                        const cplx *__restrict__ D, const double *__restrict__ W2, const cplx *__restrict__ phase, long long ld,
                                                        int nrec, int ncol, double par0, cplx *V, double *__restrict__ GN) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nrec * ncol) return;
    const int r = (int)(t / ncol), j = (int)(t % ncol);
    const long long i = (long long)r * ld + j;
    const cplx p = P[i], d = D[i], s = S[j];
    const double w = W2 ? W2[i] : 1.0;
    const bool live = w > 0.0;
    cplx v = mf_conjmul(s, PSI[i]);
    if (coef) {
        const cplx e = cmake(coef[3 * (long long)j], coef[3 * (long long)j + 1]);
        const double f = coef[3 * (long long)j + 2];
        const cplx ed = mf_mul(e, d);
        v = cmake(v.x + w * (ed.x - f * p.x), v.y + w * (ed.y - f * p.y));
    }
    if (phase) v = mf_mul(phase[r], v);
    V[i] = live ? v : cmake(0.0, 0.0);
    if (GN) GN[i] = live ? misfit_gn_weight<KIND>(p, d, s, w, par0) : 0.0;
}

static int misfit_panel_args(helm_op *op, const char *what, int kind, double par0, double par1, long long ld, int nrec, int ncol) {
    if (!op || nrec < 1 || ncol < 1 || ld < ncol) return HELM_ERR_ARG;
    if (kind < MISFIT_L2 || kind > MISFIT_LOG) HELM_FAIL(op, HELM_ERR_ARG, "%s: kind %d is none of l2 (0), huber (1), hybrid (2), logarithmic (3)", what, kind);
    if ((kind == MISFIT_HUBER || kind == MISFIT_HYBRID) && !(par0 > 0.0)) HELM_FAIL(op, HELM_ERR_ARG, "%s: the threshold / epsilon must be positive", what);
    if (kind == MISFIT_LOG && !(par0 >= 0.0 && par1 >= 0.0)) HELM_FAIL(op, HELM_ERR_ARG, "%s: the amplitude and phase weights must not be negative", what);
    return HELM_OK;
}
static inline bool misaligned16(const void *a) { return (((uintptr_t)a) & 15) != 0; }
static inline bool misaligned8(const void *a) { return (((uintptr_t)a) & 7) != 0; }

// dMom[j] = (Re a_j, Im a_j, b_j), j < ncol, from the sample panel dP and the dobs / weight panels dD / dW2 (NULL: ones), all [nrec][ld].  Returns when
// dMom is complete.
extern "C" int helm_misfit_moments_device(helm_op *op, const void *dP, const void *dD, const void *dW2, long long ld, int nrec, int ncol, void *dMom) {
    helm_tuning_refresh();
    if (!op || !dP || !dD || !dMom || nrec < 1 || ncol < 1 || ld < ncol) return HELM_ERR_ARG;
    if (misaligned16(dP) || misaligned16(dD) || misaligned8(dW2) || misaligned8(dMom)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_misfit_moments, dim3((unsigned)((ncol + MISFIT_LANES - 1) / MISFIT_LANES)), dim3(MISFIT_LANES), 0, op->stream, (const cplx *)dP, (const cplx *)dD,
                (const double *)dW2, ld, nrec, ncol, (double *)dMom);
    return launched(op);
}

template <int KIND>
static int misfit_terms_launch(helm_op *op, double par0, double par1, const void *dP, const void *dD, const void *dW2, const void *dS, long long ld, int nrec, int ncol,
                               void *dPsi, void *dOut) {
    HELM_LAUNCH(k_misfit_terms<KIND>, dim3((unsigned)((ncol + MISFIT_LANES - 1) / MISFIT_LANES)), dim3(MISFIT_LANES), 0, op->stream, (const cplx *)dP, (const cplx *)dD,
                (const double *)dW2, (const cplx *)dS, ld, nrec, ncol, par0, par1, (cplx *)dPsi, (double *)dOut);
    return launched(op);
}
// dPsi = psi ([nrec][ld], 0 where w2 = 0; it must not overlap the inputs) and dOut[j] = (phi_j, Re c_j, Im c_j) at the source factors dS[j] (ncol complex128).
// Returns when both are complete.
extern "C" int helm_misfit_terms_device(helm_op *op, int kind, double par0, double par1, const void *dP, const void *dD, const void *dW2, const void *dS, long long ld,
                                        int nrec, int ncol, void *dPsi, void *dOut) {
    helm_tuning_refresh();
    const int rc = misfit_panel_args(op, "helm_misfit_terms_device", kind, par0, par1, ld, nrec, ncol);
    if (rc) return rc;
    if (!dP || !dD || !dS || !dPsi || !dOut || dPsi == dP || dPsi == dD) return HELM_ERR_ARG;
    if (misaligned16(dP) || misaligned16(dD) || misaligned16(dS) || misaligned16(dPsi) || misaligned8(dW2) || misaligned8(dOut)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    switch (kind) {
    case MISFIT_HUBER: return misfit_terms_launch<MISFIT_HUBER>(op, par0, par1, dP, dD, dW2, dS, ld, nrec, ncol, dPsi, dOut);
    case MISFIT_HYBRID: return misfit_terms_launch<MISFIT_HYBRID>(op, par0, par1, dP, dD, dW2, dS, ld, nrec, ncol, dPsi, dOut);
    case MISFIT_LOG: return misfit_terms_launch<MISFIT_LOG>(op, par0, par1, dP, dD, dW2, dS, ld, nrec, ncol, dPsi, dOut);
    default: return misfit_terms_launch<MISFIT_L2>(op, par0, par1, dP, dD, dW2, dS, ld, nrec, ncol, dPsi, dOut);
    }
}

template <int KIND>
static int misfit_adjoint_launch(helm_op *op, double par0, const void *dPsi, const void *dS, const void *dCoef, const void *dP, const void *dD, const void *dW2,
                                 const void *dPhase, long long ld, int nrec, int ncol, void *dV, void *dGn) {
    const long long tot = (long long)nrec * ncol;
    HELM_LAUNCH(k_misfit_adjoint<KIND>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)dPsi, (const cplx *)dS, (const double *)dCoef,
                (const cplx *)dP, (const cplx *)dD, (const double *)dW2, (const cplx *)dPhase, ld, nrec, ncol, par0, (cplx *)dV, (double *)dGn);
    return launched(op);
}
// dV = phase (conj(s) psi + w2 (e d - f p)), [nrec][ld], 0 where w2 = 0.  dCoef[j] = (Re e_j, Im e_j, f_j) or NULL (a given source: the first term alone);
// dPhase: nrec complex128 per-receiver factors or NULL; dGn: NULL, or a [nrec][ld] panel of doubles that receives the Gauss-Newton weights.  dV may be dP (the
// adjoint source replaces the samples); it must not be dPsi or dD.  Returns when dV (and dGn) are complete.
extern "C" int helm_misfit_adjoint_device(helm_op *op, int kind, double par0, double par1, const void *dPsi, const void *dS, const void *dCoef, const void *dP,
                                          const void *dD, const void *dW2, const void *dPhase, long long ld, int nrec, int ncol, void *dV, void *dGn) {
    helm_tuning_refresh();
    const int rc = misfit_panel_args(op, "helm_misfit_adjoint_device", kind, par0, par1, ld, nrec, ncol);
    if (rc) return rc;
    if (!dPsi || !dS || !dP || !dD || !dV || dV == dPsi || dV == dD) return HELM_ERR_ARG;
    if (misaligned16(dPsi) || misaligned16(dS) || misaligned16(dP) || misaligned16(dD) || misaligned16(dV) || misaligned16(dPhase) || misaligned8(dW2) ||
        misaligned8(dCoef) || misaligned8(dGn))
        return HELM_ERR_ARG;
    if (dGn && kind == MISFIT_LOG && par0 != par1)
        HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_misfit_adjoint_device: with amplitude != phase the curvature of the logarithmic misfit is not a real diagonal in the data");
    HIP_TRY(op, hipSetDevice(op->device));
    switch (kind) {
    case MISFIT_HUBER: return misfit_adjoint_launch<MISFIT_HUBER>(op, par0, dPsi, dS, dCoef, dP, dD, dW2, dPhase, ld, nrec, ncol, dV, dGn);
    case MISFIT_HYBRID: return misfit_adjoint_launch<MISFIT_HYBRID>(op, par0, dPsi, dS, dCoef, dP, dD, dW2, dPhase, ld, nrec, ncol, dV, dGn);
    case MISFIT_LOG: return misfit_adjoint_launch<MISFIT_LOG>(op, par0, dPsi, dS, dCoef, dP, dD, dW2, dPhase, ld, nrec, ncol, dV, dGn);
    default: return misfit_adjoint_launch<MISFIT_L2>(op, par0, dPsi, dS, dCoef, dP, dD, dW2, dPhase, ld, nrec, ncol, dV, dGn);
    }
}
