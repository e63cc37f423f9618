// One row of an Eurus block (Operto 2009 mixed-grid TTI, C-PML), shared by its assembly (assemble.hip k_assemble_eurus) and by the derivative maps of M1
// (survey_eurus.hip k_eurus_planes / k_eurus_adjoint): what turns the 3 x 3 buoyancies b, the mass terms K = omega_d^2 b / c^2 of the same (clamped) cells, the
// PML averages of the row and its anisotropy coefficients into the nine entries.  Every entry is linear and homogeneous in (b, K) for fixed PML and
// coefficients -- the PML profiles are 1-D functions of cPML and omega and do not depend on the model -- so the derivative kernels evaluate the same statements
// at (db, dK).  Entries go by the PROPERTY neighbour: eu_entry(e, 3 (sz + 1) + (sx + 1)) is built from the cell (iz + sz, ix + sx) and, with the reference's z-flipped ordering
// mord = (-nx, +1), belongs to the matrix slot (-sz, sx): eu_matrix_slot.
#pragma once
#include "helm_internal.hpp"

struct EuParams {
    int nz, nx;
    double dx, dz;
    cplx om;
    int aniso;
    int nblk_out;     // 4, or 1 to build only M1
};

// EuParams and the device PML profiles of the operator an assembled 2-D Eurus handle holds (assemble.hip)
int helm_eu_params(helm_op *op, EuParams *P, const cplx **xix, const cplx **xiz);

// mass weights (centre, edge, corner; eurus.py:229-269) and the blend of the rotated and the plain stiffness star
constexpr double EU_WM1 = 0.6287326, EU_WM2R = 0.3712667, EU_W1 = 0.4382634;
constexpr double EU_WM2 = 0.25 * EU_WM2R, EU_WM3 = 0.25 * (1.0 - EU_WM1 - EU_WM2R), EU_W1C = 1.0 - 0.4382634;

// matrix slot of the entry built from the property neighbour (sz, sx): the plane multiplies u(iz - sz, ix + sx)
__host__ __device__ inline int eu_matrix_slot(int sz, int sx) { return 3 * (-sz + 1) + (sx + 1); }

// PML averages of a row from the padded 1-D profiles (index p = i + 1): eurus.py:140-168
struct EuPml { cplx xM, xP, zM, zP, xc, zc, Lx4, Lx, Lz4, Lz; };
__device__ __forceinline__ EuPml eu_pml_of(double dx, double dz, cplx xl, cplx xc, cplx xr, cplx zl, cplx zc, cplx zr) {
    const double dxx = dx * dx, dzz = dz * dz;
    EuPml q;
    q.xc = xc; q.zc = zc;
    q.xM = cscale(cadd(xl, xc), 0.5); q.xP = cscale(cadd(xc, xr), 0.5);
    q.zM = cscale(cadd(zl, zc), 0.5); q.zP = cscale(cadd(zc, zr), 0.5);
    q.Lx4 = crecip(cscale(xc, 4 * dxx)); q.Lx = crecip(cscale(xc, dxx));
    q.Lz4 = crecip(cscale(zc, 4 * dzz)); q.Lz = crecip(cscale(zc, dzz));
    return q;
}
__device__ __forceinline__ EuPml eu_pml_at(double dx, double dz, const cplx *__restrict__ xix, const cplx *__restrict__ xiz, int iz, int ix) {
    return eu_pml_of(dx, dz, xix[ix], xix[ix + 1], xix[ix + 2], xiz[iz], xiz[iz + 1], xiz[iz + 2]);
}

// buoyancy squares and lines over the PML averages (eurus.py:170-226), from b in property order: m = index - 1, p = index + 1; first letter z, second x
struct EuStiff { cplx s1x, s2x, s3x, s4x, s1z, s2z, s3z, s4z, ln1, ln2, ln3, ln4, ln1c, ln2c, ln3c, ln4c; };
__device__ __forceinline__ EuStiff eu_stiffness(const EuPml &q, const double (&b)[9]) {
    const double bmm = b[0], bm0 = b[1], bmp = b[2], b0m = b[3], b00 = b[4], b0p = b[5], bpm = b[6], bp0 = b[7], bpp = b[8];
    const double sq1 = (bpm + bp0 + b0m + b00) / 4, sq2 = (bp0 + bpp + b00 + b0p) / 4;
    const double sq3 = (b0m + b00 + bmm + bm0) / 4, sq4 = (b00 + b0p + bm0 + bmp) / 4;
    EuStiff s;
    // NB: the reference divides (b / xi); multiply by the reciprocal differs by <= 1 ulp-level rounding
    s.s1x = cdiv(cmake(sq1, 0), q.xM); s.s2x = cdiv(cmake(sq2, 0), q.xP); s.s3x = cdiv(cmake(sq3, 0), q.xM); s.s4x = cdiv(cmake(sq4, 0), q.xP);
    s.s1z = cdiv(cmake(sq1, 0), q.zM); s.s2z = cdiv(cmake(sq2, 0), q.zM); s.s3z = cdiv(cmake(sq3, 0), q.zP); s.s4z = cdiv(cmake(sq4, 0), q.zP);
    s.ln1 = cdiv(cmake((bp0 + b00) / 2, 0), q.zM); s.ln2 = cdiv(cmake((b0m + b00) / 2, 0), q.xM);
    s.ln3 = cdiv(cmake((b00 + b0p) / 2, 0), q.xP); s.ln4 = cdiv(cmake((b00 + bm0) / 2, 0), q.zP);
    s.ln1c = cdiv(cmake((bp0 + b00) / 2, 0), q.xc); s.ln2c = cdiv(cmake((b0m + b00) / 2, 0), q.zc);
    s.ln3c = cdiv(cmake((b00 + b0p) / 2, 0), q.zc); s.ln4c = cdiv(cmake((b00 + bm0) / 2, 0), q.xc);
    return s;
}

// the TTI coefficient fields of a row (eurus.py:279-295): M1 takes (Ax, Bx, Bx, Bz)
struct EuTti { double Ax, Bx, Cx, Dx, Ex, Fx, Bz, Dz, Fz; };
__device__ __forceinline__ EuTti eu_tti(double th, double ep, double de) {
    const double ct = cos(th), st = sin(th), s2t = sin(2.0 * th);
    const double ct2 = ct * ct, st2 = st * st;
    EuTti t;
    t.Ax = 1.0 + (2.0 * de) * ct2; t.Bx = (-1.0 * de) * s2t; t.Cx = (1.0 + (2.0 * de)) * ct2;
    t.Dx = (-0.5 * (1.0 + (2.0 * de))) * s2t; t.Ex = (2.0 * (ep - de)) * ct2; t.Fx = (-1.0 * (ep - de)) * s2t;
    t.Bz = 1.0 + (2.0 * de) * st2; t.Dz = (1.0 + (2.0 * de)) * st2; t.Fz = (2.0 * (ep - de)) * st2;
    return t;
}

// the mass terms of the nine cells with their weights, property order
__device__ __forceinline__ void eu_mass_weighted(const cplx (&K)[9], cplx (&Kw)[9]) {
    Kw[0] = cscale(K[0], EU_WM3); Kw[1] = cscale(K[1], EU_WM2); Kw[2] = cscale(K[2], EU_WM3);
    Kw[3] = cscale(K[3], EU_WM2); Kw[4] = cscale(K[4], EU_WM1); Kw[5] = cscale(K[5], EU_WM2);
    Kw[6] = cscale(K[6], EU_WM3); Kw[7] = cscale(K[7], EU_WM2); Kw[8] = cscale(K[8], EU_WM3);
}

// the nine entries of a row, named as the reference names them; eu_entry(e, p) is the one built from the property neighbour p = 3 (sz + 1) + (sx + 1)
struct EuEntries { cplx GG, HH, II, DD, EE, FF, AA, BB, CC; };
__device__ __forceinline__ cplx eu_entry(const EuEntries &e, int p) {
    return p == 0 ? e.GG : p == 1 ? e.HH : p == 2 ? e.II : p == 3 ? e.DD : p == 4 ? e.EE : p == 5 ? e.FF : p == 6 ? e.AA : p == 7 ? e.BB : e.CC;
}

// the nine entries of a row of one block (eurus.py:300-427) from the weighted mass terms, the stiffness terms and the block's coefficients
// (mass, c1x, c1z, c2x, c2z)
__device__ __forceinline__ EuEntries eu_row_entries(const EuPml &q, const EuStiff &s, const cplx (&Kw)[9], double mass, double c1x, double c1z, double c2x, double c2z) {
    EuEntries out;
    const cplx Kmm = Kw[0], Km0 = Kw[1], Kmp = Kw[2], K0m = Kw[3], K00 = Kw[4], K0p = Kw[5], Kpm = Kw[6], Kp0 = Kw[7], Kpp = Kw[8];
    const cplx s1x = s.s1x, s2x = s.s2x, s3x = s.s3x, s4x = s.s4x, s1z = s.s1z, s2z = s.s2z, s3z = s.s3z, s4z = s.s4z;
    const cplx ln1 = s.ln1, ln2 = s.ln2, ln3 = s.ln3, ln4 = s.ln4, ln1c = s.ln1c, ln2c = s.ln2c, ln3c = s.ln3c, ln4c = s.ln4c;
    const double w1 = EU_W1, w1c = EU_W1C;
    const cplx ax = cscale(q.Lx4, c1x), bx = cscale(q.Lx4, c2x), az = cscale(q.Lz4, c1z), bz = cscale(q.Lz4, c2z);
    const cplx axf = cscale(q.Lx, c1x), bzf = cscale(q.Lz, c2z);
    cplx t, u;
    // GG
    t = csub(csub(cmul(ax, s3x), cmul(bx, s3z)), cmul(az, s3x)); t = cadd(t, cmul(bz, s3z));
    u = cneg(cadd(cmul(bx, ln2c), cmul(az, ln4c)));
    out.GG = cadd(cscale(Kmm, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // HH
    t = cadd(cadd(cmul(ax, cneg(cadd(s3x, s4x))), cmul(bx, csub(s4z, s3z))),
             cadd(cmul(az, csub(s3x, s4x)), cmul(bz, cadd(s3z, s4z))));
    u = cadd(cmul(bx, csub(ln3c, ln2c)), cmul(bzf, ln4));
    out.HH = cadd(cscale(Km0, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // II
    t = cadd(cadd(cmul(ax, s4x), cmul(bx, s4z)), cadd(cmul(az, s4x), cmul(bz, s4z)));
    u = cadd(cmul(bx, ln3c), cmul(az, ln4c));
    out.II = cadd(cscale(Kmp, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // DD
    t = cadd(cadd(cmul(ax, cadd(s3x, s1x)), cmul(bx, csub(s3z, s1z))),
             cadd(cmul(az, csub(s1x, s3x)), cmul(bz, cneg(cadd(s3z, s1z)))));
    u = cadd(cmul(axf, ln2), cmul(az, csub(ln1c, ln4c)));
    out.DD = cadd(cscale(K0m, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // EE
    t = cadd(cadd(cmul(cneg(ax), cadd(cadd(s1x, s2x), cadd(s3x, s4x))),
                  cmul(bx, csub(cadd(s2z, s3z), cadd(s1z, s4z)))),
             cadd(cmul(az, csub(cadd(s2x, s3x), cadd(s1x, s4x))),
                  cmul(cneg(bz), cadd(cadd(s1z, s2z), cadd(s3z, s4z)))));
    u = cadd(cmul(axf, cneg(cadd(ln2, ln3))), cmul(bzf, cneg(cadd(ln1, ln4))));
    out.EE = cadd(cscale(K00, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // FF
    t = cadd(cadd(cmul(ax, cadd(s2x, s4x)), cmul(bx, csub(s2z, s4z))),
             cadd(cmul(az, csub(s4x, s2x)), cmul(bz, cneg(cadd(s2z, s4z)))));
    u = cadd(cmul(axf, ln3), cmul(az, csub(ln4c, ln1c)));
    out.FF = cadd(cscale(K0p, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // AA
    t = cadd(cadd(cmul(ax, s1x), cmul(bx, s1z)), cadd(cmul(az, s1x), cmul(bz, s1z)));
    u = cadd(cmul(bx, ln2c), cmul(az, ln1c));
    out.AA = cadd(cscale(Kpm, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // BB
    t = cadd(cadd(cmul(ax, cneg(cadd(s2x, s1x))), cmul(bx, csub(s1z, s2z))),
             cadd(cmul(az, csub(s2x, s1x)), cmul(bz, cadd(s2z, s1z))));
    u = cadd(cmul(bx, csub(ln2c, ln3c)), cmul(bzf, ln1));
    out.BB = cadd(cscale(Kp0, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    // CC
    t = csub(csub(cmul(ax, s2x), cmul(bx, s2z)), cmul(az, s2x)); t = cadd(t, cmul(bz, s2z));
    u = cneg(cadd(cmul(bx, ln3c), cmul(az, ln1c)));
    out.CC = cadd(cscale(Kpp, mass), cadd(cscale(t, w1), cscale(u, w1c)));
    return out;
}

// a row of M1: the nine entries from the buoyancies and the UNWEIGHTED mass terms of the 3 x 3 cells, the row's PML averages and its theta, delta
__device__ __forceinline__ EuEntries eu_m1_row(const EuPml &q, const double (&b)[9], const cplx (&K)[9], double th, double de) {
    const EuTti t = eu_tti(th, de, de);
    cplx Kw[9];
    eu_mass_weighted(K, Kw);
    return eu_row_entries(q, eu_stiffness(q, b), Kw, 1.0, t.Ax, t.Bx, t.Bx, t.Bz);
}
