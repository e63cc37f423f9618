// The derivative maps of the Eurus block M1 (eps == delta: the block an N-row right-hand side is solved through) and the boundary-line lag product they need.
//
// A row of M1 is eu_m1_row (eu_row.hpp): linear and homogeneous in the buoyancies b = 1 / rho and the mass terms K = omega_d^2 b / c^2 of the 3 x 3 (clamped)
// cells around it; the PML averages are 1-D functions of cPML and omega, and theta, delta are coefficients.  The velocity enters through K alone.  So along real
// perturbations (dc, db) the nine planes of dM1 are
//     dC = V[dc] + L[db],   L[db] = eu_m1_row(b -> db, K -> omega_d^2 db / c^2),   V[dc] = the mass entries at K -> -2 omega_d^2 b dc / c^3
// (k_eurus_planes).  The entry built from the property neighbour (sz, sx) belongs to the matrix slot (-sz, sx) -- the reference's z-flipped ordering -- and an edge
// row keeps its centre entry EE alone, which depends on the model: its derivative is carried, with the clamped neighbours counted as the assembly counts them.
// k_eurus_adjoint is the plain transpose of both maps as a gather over the rows of the 3 x 3 block around a cell.  The forward and imaging loops over stored
// columns are those of the MiniZephyr derivatives (k_stencil_sources, k_lag_imaging: they read nothing but nine planes); k_lag_imaging leaves the boundary lines
// of P alone, so k_lag_centre_edges adds the one product an edge row needs there, P_4[i] += sum_s UB_s[i] UF_s[i].
#include "survey_internal.hpp"
#include "eu_row.hpp"

namespace {

__device__ __forceinline__ int eu_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// dC[9][N] = V[dc] + L[db], either of dc, db may be null: one lane per cell, the assembly's row on the perturbation
__global__ __launch_bounds__(256) void k_eurus_planes(EuParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ theta,
                                                      const double *__restrict__ delta, const cplx *__restrict__ xix, const cplx *__restrict__ xiz,
                                                      const double *__restrict__ dc, const double *__restrict__ db, cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    const EuPml pml = eu_pml_at(P.dx, P.dz, xix, xiz, iz, ix);
    const cplx om2 = cmul(P.om, P.om);
    double b[9];
    cplx K[9];
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int jz = eu_clamp(iz + sz, 0, P.nz - 1), jx = eu_clamp(ix + sx, 0, P.nx - 1);
            const long long j = (long long)jz * P.nx + jx;
            const cplx cj = c[j];
            const cplx k2 = cdiv(om2, cmul(cj, cj));                 // omega_d^2 / c^2
            const double dbj = db ? db[j] : 0.0;
            cplx k = cscale(k2, dbj);
            if (dc) {
                const cplx kc = cdiv(k2, cj);                        // omega_d^2 / c^3
                const double f = -2.0 * dc[j] / rho[j];
                k.x = fma(kc.x, f, k.x); k.y = fma(kc.y, f, k.y);
            }
            b[mz_slot(sz, sx)] = dbj;
            K[mz_slot(sz, sx)] = k;
        }
    double th = 0, de = 0;
    if (P.aniso) { th = theta ? theta[i] : 0.0; de = delta ? delta[i] : 0.0; }
    const EuEntries out = eu_m1_row(pml, b, K, th, de);
    const bool edge = (ix == 0) || (ix == P.nx - 1) || (iz == 0) || (iz == P.nz - 1);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int p = mz_slot(sz, sx);
            C[(long long)eu_matrix_slot(sz, sx) * N + i] = (edge && p != 4) ? cmake(0.0, 0.0) : eu_entry(out, p);
        }
}

// what the row i = j - (OZ, OX) of the 3 x 3 block around cell j adds to (V^T Pl)[j] and (L^T Pl)[j]: k_eurus_adjoint below.  The lag is a template argument so
// that the unit buoyancy of an interior row is known when the row formulas are compiled.
struct EuAdjointArgs {
    EuParams P;
    const double *__restrict__ theta, *__restrict__ delta;
    const cplx *__restrict__ xix, *__restrict__ xiz, *__restrict__ Pl;
    cplx kL, kV;                // d K_j / d b_j = omega_d^2 / c_j^2 and d K_j / d c_j = -2 omega_d^2 b_j / c_j^3
    int jz, jx;
    bool wantc, wantb;
};
template <int OZ, int OX, bool CONJ>
__device__ __forceinline__ void eu_adjoint_row(const EuAdjointArgs &a, cplx &sumc, cplx &sumb) {
    const EuParams &P = a.P;
    const long long N = (long long)P.nz * P.nx;
    const int iz = a.jz - OZ, ix = a.jx - OX;                      // row i sees cell j as its property neighbour (OZ, OX) -- and, on an edge, wherever clamping leads to j
    if (iz < 0 || iz > P.nz - 1 || ix < 0 || ix > P.nx - 1) return;
    const long long i = (long long)iz * P.nx + ix;
    const bool edge = (ix == 0) || (ix == P.nx - 1) || (iz == 0) || (iz == P.nz - 1);
    double th = 0, de = 0;
    if (P.aniso) { th = a.theta ? a.theta[i] : 0.0; de = a.delta ? a.delta[i] : 0.0; }
    const EuPml pml = eu_pml_at(P.dx, P.dz, a.xix, a.xiz, iz, ix);
    double ub[9];
    cplx K[9];
    if (edge) {
        // EE alone; a cell reached through clamping from several places is counted once per place (every row is visited once: at the lag that is j - i)
        const cplx p4 = a.Pl[4 * N + i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const bool hit = eu_clamp(iz + sz, 0, P.nz - 1) == a.jz && eu_clamp(ix + sx, 0, P.nx - 1) == a.jx;
                ub[mz_slot(sz, sx)] = hit ? 1.0 : 0.0;
                K[mz_slot(sz, sx)] = hit ? a.kL : cmake(0.0, 0.0);
            }
        if (a.wantb) {
            const cplx ee = eu_m1_row(pml, ub, K, th, de).EE;
            cfma(sumb, CONJ ? cconj(ee) : ee, p4);
        }
        if (a.wantc && OZ == 0 && OX == 0) {
            const cplx e = cscale(a.kV, EU_WM1);
            cfma(sumc, CONJ ? cconj(e) : e, p4);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 9; ++p) { ub[p] = p == mz_slot(OZ, OX) ? 1.0 : 0.0; K[p] = p == mz_slot(OZ, OX) ? a.kL : cmake(0.0, 0.0); }
        cplx pk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) pk[k] = a.Pl[(long long)k * N + i];
        if (a.wantb) {
            const EuEntries out = eu_m1_row(pml, ub, K, th, de);
#pragma unroll
            for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    const cplx e = eu_entry(out, mz_slot(sz, sx));
                    cfma(sumb, CONJ ? cconj(e) : e, pk[eu_matrix_slot(sz, sx)]);
                }
        }
        if (a.wantc) {
            const double m = (OZ == 0 && OX == 0) ? EU_WM1 : ((OZ == 0 || OX == 0) ? EU_WM2 : EU_WM3);
            const cplx e = cscale(a.kV, m);
            cfma(sumc, CONJ ? cconj(e) : e, pk[eu_matrix_slot(OZ, OX)]);
        }
    }
}

// Gc[j] += w (V^T Pl)[j] and Gb[j] += w (L^T Pl)[j] (CONJ: the conjugated coefficients), either output may be null: one lane per cell j, a gather over the rows i
// of the 3 x 3 block around it, from one read of the nine planes at each row.  An interior row i = j - o sees cell j in exactly one place, the property neighbour o:
// its coefficients are eu_m1_row on the unit buoyancy there (the compiler drops what the zeros remove).  An edge row keeps EE alone and sees cell j wherever the
// clamped neighbour is j: the unit buoyancies are made at run time.  One writer per cell, a fixed order (the rows in lag order), no atomics, no LDS.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_eurus_adjoint(EuParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ theta,
                                                       const double *__restrict__ delta, const cplx *__restrict__ xix, const cplx *__restrict__ xiz,
                                                       const cplx *__restrict__ Pl, cplx w, cplx *__restrict__ Gc, cplx *__restrict__ Gb) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    EuAdjointArgs a;
    a.P = P; a.theta = theta; a.delta = delta; a.xix = xix; a.xiz = xiz; a.Pl = Pl;
    a.jz = (int)(j / P.nx); a.jx = (int)(j % P.nx);
    a.wantc = Gc != nullptr; a.wantb = Gb != nullptr;
    const cplx cj = c[j];
    a.kL = cdiv(cmul(P.om, P.om), cmul(cj, cj));
    a.kV = cscale(cdiv(a.kL, cj), -2.0 / rho[j]);
    cplx sumc = cmake(0.0, 0.0), sumb = cmake(0.0, 0.0);
    eu_adjoint_row<-1, -1, CONJ>(a, sumc, sumb); eu_adjoint_row<-1, 0, CONJ>(a, sumc, sumb); eu_adjoint_row<-1, 1, CONJ>(a, sumc, sumb);
    eu_adjoint_row<0, -1, CONJ>(a, sumc, sumb); eu_adjoint_row<0, 0, CONJ>(a, sumc, sumb); eu_adjoint_row<0, 1, CONJ>(a, sumc, sumb);
    eu_adjoint_row<1, -1, CONJ>(a, sumc, sumb); eu_adjoint_row<1, 0, CONJ>(a, sumc, sumb); eu_adjoint_row<1, 1, CONJ>(a, sumc, sumb);
    if (Gc) { cplx g = Gc[j]; cfma(g, w, sumc); Gc[j] = g; }
    if (Gb) { cplx g = Gb[j]; cfma(g, w, sumb); Gb[j] = g; }
}

// P_4[i] += sum_s UB[s ldb + i] UF[s ldf + i] on the 2 (nz + nx) - 4 boundary cells i, which k_lag_imaging leaves alone: one lane per boundary cell, the columns
// in order.  The top and bottom lines first (contiguous), then the two side columns row by row.
template <class F>
__global__ __launch_bounds__(256) void k_lag_centre_edges(F UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc, cplx *__restrict__ P, int nz, int nx) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * (nz + nx) - 4) return;
    int z, x;
    if (e < nx) { z = 0; x = e; }
    else if (e < 2 * nx) { z = nz - 1; x = e - nx; }
    else { const int r = e - 2 * nx; z = 1 + (r >> 1); x = (r & 1) ? nx - 1 : 0; }
    const long long N = (long long)nz * nx, i = (long long)z * nx + x;
    cplx acc = cmake(0.0, 0.0);
    for (int s = 0; s < nsrc; ++s) {
        const cplx uf = UF.value(UF.load((long long)s * ldf + i), s);
        cfma(acc, UB[(long long)s * ldb + i], uf);
    }
    cplx *p = P + 4 * N + i;
    *p = cadd(*p, acc);
}

// what the entry points here accept: an assembled 2-D Eurus handle whose model has eps == delta (M1 is then the operator of an N-row right-hand side)
int eu_handle_args(helm_op *op, const char *what) {
    if (op->variant != HELM_EURUS || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the derivative maps of M1 are those of the 2-D Eurus operator", what);
    if (!op->has_model || !op->block_zero[2]) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the model has eps != delta: the derivative of the coupled 2N x 2N system is not built", what);
    return HELM_OK;
}

}  // namespace

// dC[9][N] = V[dc] + L[db] for the operator the handle holds (its c, rho, theta, delta, PML and the frequency of its last assembly; the planes of M1, whether or not
// the handle is transposed): dc, db N float64, either may be NULL (both: dC = 0); dC 9 N complex128, edge rows with the derivative of their centre entry.
extern "C" int helm_eurus_planes_device(helm_op *op, const void *dDc, const void *dDb, void *dC) {
    helm_tuning_refresh();
    if (!op || !dC) return HELM_ERR_ARG;
    if (int rc = eu_handle_args(op, "helm_eurus_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dDc) | ((uintptr_t)dDb)) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    const size_t cbytes = (size_t)op->N * 9 * sizeof(cplx);
    if ((dDc && ranges_overlap(dDc, (size_t)op->N * 8, dC, cbytes)) || (dDb && ranges_overlap(dDb, (size_t)op->N * 8, dC, cbytes))) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "helm_eurus_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    EuParams P;
    const cplx *xix = nullptr, *xiz = nullptr;
    if (int rc = helm_eu_params(op, &P, &xix, &xiz)) HELM_FAIL(op, rc, "helm_eurus_planes_device: the PML profiles of the handle could not be made");
    HELM_LAUNCH(k_eurus_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho,
                (const double *)op->d_theta, (const double *)op->d_delta, xix, xiz, (const double *)dDc, (const double *)dDb, (cplx *)dC);
    return launched(op);
}

// Gc[j] += w sum_(k, i) V_((k, i), j) P_k[i] and Gb[j] += w sum_(k, i) L_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients), V and L the maps of
// helm_eurus_planes_device: P [9][N] complex128 (its edge rows are read at the centre plane), Gc, Gb N complex128, either may be NULL (not both).  An output must
// not overlap P or the other output.  Returns when both are complete.
extern "C" int helm_eurus_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dGc, void *dGb) {
    helm_tuning_refresh();
    if (!op || !dP || (!dGc && !dGb)) return HELM_ERR_ARG;
    if (int rc = eu_handle_args(op, "helm_eurus_adjoint_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dGc) | ((uintptr_t)dGb)) & 15)) return HELM_ERR_ARG;
    const size_t pbytes = (size_t)op->N * 9 * sizeof(cplx), gbytes = (size_t)op->N * sizeof(cplx);
    if ((dGc && ranges_overlap(dP, pbytes, dGc, gbytes)) || (dGb && ranges_overlap(dP, pbytes, dGb, gbytes)) || (dGc && dGb && ranges_overlap(dGc, gbytes, dGb, gbytes)))
        return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "helm_eurus_adjoint_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    EuParams P;
    const cplx *xix = nullptr, *xiz = nullptr;
    if (int rc = helm_eu_params(op, &P, &xix, &xiz)) HELM_FAIL(op, rc, "helm_eurus_adjoint_device: the PML profiles of the handle could not be made");
    const dim3 grid((unsigned)((op->N + 255) / 256));
#define EUADJOINT(CJ) HELM_LAUNCH(k_eurus_adjoint<CJ>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const double *)op->d_theta, \
                                  (const double *)op->d_delta, xix, xiz, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dGc, (cplx *)dGb)
    if (conj) EUADJOINT(true);
    else EUADJOINT(false);
#undef EUADJOINT
    return launched(op);
}

// P[4][i] += sum_s UB[s][i] UF[s][i] on the boundary cells i of the handle's grid, what helm_lag_imaging_accumulate[_c64]_device leaves out and an Eurus edge row
// needs: UF [nsrc][ldf] (either store format), UB [nsrc][ldb] complex128, P [9][N] complex128.  P must not overlap the fields.  Returns when P is complete.
static int lag_centre_edges_launch(helm_op *op, HostField UF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    helm_tuning_refresh();
    if (!op || !UF.u || !dUB || !dP || nsrc < 1 || ldf < op->N || ldb < op->N) return HELM_ERR_ARG;
    if (int rc = eu_handle_args(op, "helm_lag_centre_edges_accumulate_device")) return rc;       // (both entry points refuse under this name)
    if (op->nz < 3 || op->nx < 3) return HELM_ERR_ARG;
    const size_t pbytes = (size_t)op->N * 9 * sizeof(cplx);
    if (ranges_overlap(UF.u, UF.bytes(nsrc, ldf), dP, pbytes) || ranges_overlap(dUB, (size_t)nsrc * ldb * sizeof(cplx), dP, pbytes)) return HELM_ERR_ARG;
    if (!UF.ok() || ((((uintptr_t)dUB) | ((uintptr_t)dP)) & 15)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const int cells = 2 * (op->nz + op->nx) - 4;
    return UF.with([&](auto F) {
        HELM_LAUNCH(k_lag_centre_edges<decltype(F)>, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, op->stream, F, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP,
                    op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_lag_centre_edges_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    return lag_centre_edges_launch(op, HostField::c128(dUF), ldf, dUB, ldb, nsrc, dP);
}
extern "C" int helm_lag_centre_edges_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc,
                                                           void *dP) {
    return lag_centre_edges_launch(op, HostField::packed(dUF32, dExp), ldf, dUB, ldb, nsrc, dP);
}
