// The row factors of the 2-D MiniZephyr operator, shared by its assembly (assemble.hip k_assemble_mz) and by the buoyancy derivative (survey_frechet.hip
// k_buoyancy_planes / k_buoyancy_adjoint): what a row takes from the velocity of its own cell and from the PML alone.  Their derivatives with respect to that
// velocity (mz_row_factors_dc, mz_kappa_dc) serve the total velocity derivative (survey_frechet.hip k_velocity_planes / k_velocity_adjoint), the second
// derivatives (mz_row_factors_d2c, mz_kappa_d2c) the residual part of the Newton Hessian (survey_newton.hip k_velocity_curvature).
#pragma once
#include "helm_internal.hpp"

struct MzParams {
    int nz, nx;
    double dx, dz, aky;
    cplx om;          // damped angular frequency
    double fx, fz;    // PML factors 3 ln(1/1e-3) / (2 L^3)
    int fs0, fs1, fs2, fs3;
    int npml;         // (the profiles made in place by mz_profile_at; k_assemble_mz reads the uploaded ones)
};

// the weights of the 9-point star (minizephyr.py:205-209): stiffness a, b; mass centre c, edge d, corner e
constexpr double MZ_WA = 0.5461, MZ_WB = 0.4539, MZ_WC = 0.6248, MZ_WD = 0.09381, MZ_WE = 0.000001297;

// PML stretch factors of a row from the local (unpadded) velocity c0 and the profiles at its cell (minizephyr.py:98-133)
struct MzRow { cplx X, Z, px, pz; };
__device__ __forceinline__ MzRow mz_row_factors(const MzParams &P, cplx c0, double dX, double sX, double dZ, double sZ) {
    const cplx iom = cmake(-P.om.y, P.om.x);          // 1j * om
    MzRow r;
    cplx denx = cadd(cscale(cscale(c0, P.fx), dX * dX), iom);
    cplx r1x = cdiv(iom, denx);
    r.X = cmul(r1x, r1x);
    r.px = cdiv(cmul(cscale(r.X, sX), cscale(cscale(c0, 2.0 * P.fx), dX)), denx);
    cplx denz = cadd(cscale(cscale(c0, P.fz), dZ * dZ), iom);
    cplx r1z = cdiv(iom, denz);
    r.Z = cmul(r1z, r1z);
    r.pz = cdiv(cmul(cscale(r.Z, sZ), cscale(cscale(c0, 2.0 * P.fz), dZ)), denz);
    return r;
}

// d (X, px) / dc along one axis (f the PML factor, d the profile distance, s its sign), from the same inputs: with den = f c d^2 + i om, X = (i om / den)^2 and
// p = s X 2 f c d / den,   dX/dc = -2 X f d^2 / den,   dp/dc = s 2 f d (dX/dc c + X - X c f d^2 / den) / den.  Outside the layers d = 0 and both are zero.
__device__ __forceinline__ void mz_axis_factors_dc(cplx iom, double f, cplx c0, double d, double s, cplx &dS, cplx &dp) {
    const double fdd = f * d * d;
    const cplx den = cadd(cscale(c0, fdd), iom);
    const cplx r1 = cdiv(iom, den);
    const cplx S = cmul(r1, r1);
    dS = cdiv(cscale(S, -2.0 * fdd), den);
    const cplx Sc = cmul(S, c0);
    const cplx inner = csub(cadd(cmul(dS, c0), S), cdiv(cscale(Sc, fdd), den));
    dp = cdiv(cscale(inner, s * 2.0 * f * d), den);
}
// d (X, Z, px, pz) / dc of mz_row_factors: the derivative of a row's stretch factors with respect to the velocity of its own cell
__device__ __forceinline__ MzRow mz_row_factors_dc(const MzParams &P, cplx c0, double dX, double sX, double dZ, double sZ) {
    const cplx iom = cmake(-P.om.y, P.om.x);          // 1j * om
    MzRow r;
    mz_axis_factors_dc(iom, P.fx, c0, dX, sX, r.X, r.px);
    mz_axis_factors_dc(iom, P.fz, c0, dZ, sZ, r.Z, r.pz);
    return r;
}

// d^2 (X, px) / dc^2 along one axis, from the same inputs: with a = f d^2, X = (i om)^2 / den^2 and p = s 2 f d (i om)^2 c / den^3,
//   d2X/dc2 = 6 X a^2 / den^2,   d2p/dc2 = s 2 f d (2 d2X/dc2 c - 6 X a / den) / den.  Outside the layers d = 0 and both are zero.
__device__ __forceinline__ void mz_axis_factors_d2c(cplx iom, double f, cplx c0, double d, double s, cplx &d2S, cplx &d2p) {
    const double fdd = f * d * d;
    const cplx den = cadd(cscale(c0, fdd), iom);
    const cplx r1 = cdiv(iom, den);
    const cplx S = cmul(r1, r1);
    const cplx Sa = cdiv(cscale(S, fdd), den);
    d2S = cdiv(cscale(Sa, 6.0 * fdd), den);
    const cplx inner = csub(cscale(cmul(d2S, c0), 2.0), cscale(Sa, 6.0));
    d2p = cdiv(cscale(inner, s * 2.0 * f * d), den);
}
// d^2 (X, Z, px, pz) / dc^2 of mz_row_factors: what the second derivative of a row with respect to the velocity of its own cell is made of
__device__ __forceinline__ MzRow mz_row_factors_d2c(const MzParams &P, cplx c0, double dX, double sX, double dZ, double sZ) {
    const cplx iom = cmake(-P.om.y, P.om.x);          // 1j * om
    MzRow r;
    mz_axis_factors_d2c(iom, P.fx, c0, dX, sX, r.X, r.px);
    mz_axis_factors_d2c(iom, P.fz, c0, dZ, sZ, r.Z, r.pz);
    return r;
}

// kappa = omega_d^2 / c^2 - ky^2 of a cell: K = kappa / rho
__device__ __forceinline__ cplx mz_kappa(const MzParams &P, cplx cj) {
    cplx k = cdiv(cmul(P.om, P.om), cmul(cj, cj));
    k.x -= P.aky * P.aky;
    return k;
}
// d kappa / dc = -2 omega_d^2 / c^3 of a cell
__device__ __forceinline__ cplx mz_kappa_dc(const MzParams &P, cplx cj) {
    return cdiv(cscale(cmul(P.om, P.om), -2.0), cmul(cmul(cj, cj), cj));
}

// d^2 kappa / dc^2 = 6 omega_d^2 / c^4 of a cell
__device__ __forceinline__ cplx mz_kappa_d2c(const MzParams &P, cplx cj) {
    const cplx c2 = cmul(cj, cj);
    return cdiv(cscale(cmul(P.om, P.om), 6.0), cmul(c2, c2));
}

__host__ __device__ inline int mz_slot(int dz, int dx) { return 3 * (dz + 1) + (dx + 1); }

// The nine coefficients of a row (minizephyr.py:219-243) from its factors, the averaged buoyancies bn[k] = (b_i + b_(i+k)) / 2 and the mass terms
// Kn[k] = kappa b of the neighbouring cells: linear and homogeneous in (bn, Kn), hence in the buoyancy field.  The assembly calls it with b = 1 / rho, the
// buoyancy derivative with a perturbation of b.
__device__ __forceinline__ void mz_star(const MzParams &P, const MzRow &row, const double (&bn)[9], const cplx (&Kn)[9], cplx (&out)[9]) {
    const double ac = MZ_WA, bc = MZ_WB, cc = MZ_WC, dc = MZ_WD, ec = MZ_WE;
    const double dxx = P.dx * P.dx, dzz = P.dz * P.dz, dxz = (dxx + dzz) / 2.0, dd = sqrt(dxz);
    const cplx X = row.X, Z = row.Z, px = row.px, pz = row.pz;
    const cplx ZpX = cadd(Z, X), ZmX = csub(Z, X), XmZ = csub(X, Z);
    // corners
#pragma unroll
    for (int sz = -1; sz <= 1; sz += 2)
#pragma unroll
        for (int sx = -1; sx <= 1; sx += 2) {
            const int k = mz_slot(sz, sx);
            cplx t = cadd(cscale(ZpX, 1.0 / (4 * dxz)),
                          cscale(cadd(cscale(pz, (double)sz), cscale(px, (double)sx)), 1.0 / (4 * dd)));
            out[k] = cadd(cscale(Kn[k], ec), cscale(t, bc * bn[k]));
        }
    // vertical neighbours
#pragma unroll
    for (int sz = -1; sz <= 1; sz += 2) {
        const int k = mz_slot(sz, 0);
        cplx t1 = cscale(cadd(cscale(Z, 1.0 / P.dz), cscale(pz, sz / 2.0)), ac * bn[k] / P.dz);
        cplx t2 = cscale(ZmX, bc * (bn[mz_slot(sz, 1)] + bn[mz_slot(sz, -1)]) / (4 * dxz));
        out[k] = cadd(cscale(Kn[k], dc), cadd(t1, t2));
    }
    // horizontal neighbours
#pragma unroll
    for (int sx = -1; sx <= 1; sx += 2) {
        const int k = mz_slot(0, sx);
        cplx t1 = cscale(cadd(cscale(X, 1.0 / P.dx), cscale(px, sx / 2.0)), ac * bn[k] / P.dx);
        cplx t2 = cscale(XmZ, bc * (bn[mz_slot(1, sx)] + bn[mz_slot(-1, sx)]) / (4 * dxz));
        out[k] = cadd(cscale(Kn[k], dc), cadd(t1, t2));
    }
    // centre
    {
        const double bW = bn[mz_slot(0, -1)], bE = bn[mz_slot(0, 1)], bS = bn[mz_slot(-1, 0)], bNn = bn[mz_slot(1, 0)];
        const double bSW = bn[mz_slot(-1, -1)], bNE = bn[mz_slot(1, 1)], bSE = bn[mz_slot(-1, 1)], bNW = bn[mz_slot(1, -1)];
        cplx a1 = cscale(px, (bW - bE) / (2 * P.dx));
        cplx a2 = cscale(pz, (bS - bNn) / (2 * P.dz));
        cplx a3 = cscale(X, (bW + bE) / dxx);
        cplx a4 = cscale(Z, (bS + bNn) / dzz);
        cplx aterm = csub(csub(cadd(a1, a2), a3), a4);
        cplx b1 = cscale(cadd(cscale(cadd(px, pz), (bSW - bNE)), cscale(csub(pz, px), (bSE - bNW))), 1.0 / (4 * dd));
        cplx b2 = cscale(cadd(X, Z), (bSW + bNE + bNW + bSE) / (4 * dxz));
        cplx bterm = csub(b1, b2);
        out[4] = cadd(cscale(Kn[4], cc), cadd(cscale(aterm, ac), cscale(bterm, bc)));
    }
}

// entry k of the 1-D PML distance and sign profiles along an axis of n cells: what mz_profiles (assemble.hip) tabulates, the same products
__device__ __forceinline__ void mz_profile_at(int n, int npml, double h, int fs_low, int fs_high, int k, double &dist, double &sgn) {
    const int hi = n - npml > 0 ? n - npml : 0;
    dist = k >= hi ? (double)(k - (n - npml) + 1) * h : (k < npml ? (double)(npml - k) * h : 0.0);
    sgn = (k < npml && !fs_low) ? 1.0 : ((k >= hi && !fs_high) ? -1.0 : 0.0);
}

// the parameters of the operator a handle holds, from what its last assembly recorded (assemble.hip)
int helm_mz_params(const helm_op *op, MzParams *P);
