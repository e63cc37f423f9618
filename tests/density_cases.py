"""Shared by tests/test_density_host.py (CPU) and tests/test_gpu_density.py (GPU): the density derivative (parameter='rho' of JvecBorn / Jtvec / Hvec) on the
37 x 53 survey of tests/frechet_cases.py, and the 80-bit evaluations of the four device kernels with the componentwise bounds they are held to.

The bounds.  u = 2^-53.  Every bound is c u m per component (real or imaginary part), m the sum of the moduli of the terms the component is a sum of
(the `magnitude` evaluations below and in zephyr_amd.frechet), c a count of roundings read off the code, generously:

  k_stencil_sources   a component of the nine-term sum is a chain of 18 FMAs (two per complex product), each rounding once: relative 18 u of the running
                      sum of moduli at most; the product with coef is two products and a sum per component (3).                       C_STENCIL = 18 + 3
  k_lag_imaging       per column and lag one complex FMA, two roundings per component; the sum over nsrc columns is in LAG_WAVES = 4 register chains
                      that are then added in wave order (4 more), and one addition into P.                                         c_lag = 2 nsrc + 4 + 1
  k_buoyancy_planes   the row factors: a denominator (two products, a sum: 3), a Smith division (6), a square (3) for X or Z -- 12 -- and for px / pz the
                      scaled product with c and a second division on top (10 more): 22.  kappa: a square (3), a Smith division (6), the subtraction, the
                      product with b and with the mass weight: 12.  The star then multiplies a factor by at most three constants and an average (a sum
                      and a halving: 2) and joins at most nine terms (9): 14.                                                     C_PLANES = 22 + 14 + 12
  k_buoyancy_adjoint  the same factors (22) and kappa (12); per term a difference of planes (1), a product (3), the halving is exact; a cell gathers
                      at most 8 + 8 terms of the averages and 9 of the mass in running sums (25); the product with w (3) and the addition
                      into G (1).                                                                                       C_ADJOINT = 22 + 12 + 4 + 25 + 4

A complex64 store adds 2^-24 m: every stored component is within 2^-24 relative of the packed one and enters every term linearly.
"""
import numpy as np

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
LAGS = fr.LAGS
TAYLOR_H = fc.TAYLOR_H

C_STENCIL = 18 + 3
C_PLANES = 22 + 14 + 12
C_ADJOINT = 22 + 12 + 4 + 25 + 4


def c_lag(nsrc):
    return 2 * nsrc + 4 + 1


# ---- the 37 x 53 case ---------------------------------------------------------------------------------------------------------------------------
def perturbation(seed=21, amplitude=50.):
    'a density perturbation uniform in +-50, non-zero everywhere: boundary lines and absorbing layers included'
    rng = np.random.default_rng(seed)
    return amplitude * rng.uniform(-1., 1., fc.NZ * fc.NX)


def dpred_of_rho(sv):
    'rho -> dpred at the velocity of the config'
    return lambda rho: sv.dpred({'rho': np.array(rho, dtype=np.float64)})


def taylor_remainders(sv, Jv, rho0, v, hs=TAYLOR_H):
    '||d(rho0 + h v) - d(rho0) - h Jv|| for h in hs; the model is put back'
    dpred = dpred_of_rho(sv)
    d0 = dpred(rho0)
    out = [fc.norm(dpred(rho0 + h * v.reshape(rho0.shape)) - d0 - h * Jv) for h in hs]
    sv.prob.updateModel({'rho': np.array(rho0, dtype=np.float64)})
    return out


def born_with_planes(prob, sv, uF, planes):
    """the host route of JvecBorn(linearisation='operator') with the planes of delta A given: planes(op) -> (9, nz, nx).  What a deliberately wrong derivative is
    run through."""
    st = complex(prob.system.scaleTerm)
    subs = prob.system.subProblems
    data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
    qv = [fr.applyPlanes(planes(subs[i]), np.conj(np.asarray(uF[i]) / st), subs[i].nz, subs[i].nx) / -complex(subs[i].premul) for i in range(sv.nfreq)]
    for ifreq, uB in prob._solveOwned(qv):
        uB = np.asarray(uB)
        for isrc in range(sv.nsrc):
            data[:, isrc, ifreq] = sv.rVec(isrc if sv.mode != 'fixed' else 0, ifreq) * uB[:, isrc]
    return data.ravel()


def mass_only_planes(op, db):
    'L[db] with the stiffness averages left out: the mass terms m_k kappa db of the neighbouring cell alone (a wrong derivative)'
    nz, nx = int(op.nz), int(op.nx)
    kb = fr.rowFactors(op)[4] * np.asarray(db).reshape((nz, nx))
    mc, md, me = fr.MZ_MASS
    C = np.zeros((9, nz, nx), dtype=np.complex128)
    for k, (sz, sx) in enumerate(LAGS):
        C[k] = (mc if (sz, sx) == (0, 0) else (me if sz and sx else md)) * fr._at(kb, sz, sx)
    C[:, ~fr._interiorMask(nz, nx)] = 0
    return C


# ---- the four kernels in 80-bit arithmetic ------------------------------------------------------------------------------------------------------------
def _shift(a, sz, sx):
    return fr._at(a, sz, sx)


def stencil_sources_reference(U, C, coef, nz, nx, conj, dtype=CLD, lags=LAGS):
    """R[s] = coef sum_k C_k (.) conj-or-not(U[s])(i + off_k), cells outside the grid contributing nothing, and the magnitude |coef| sum_k |C_k||u| the bound
    scales.  U (nsrc, N), C (9, N).  lags: the offsets the planes are paired with (the kernel's: LAGS; a mis-shifted list makes a wrong evaluation)."""
    real = LD if dtype is CLD else np.float64
    Ux = np.asarray(U).astype(dtype)
    if conj:
        Ux = np.conj(Ux)
    Cx = np.asarray(C).astype(dtype).reshape((9, nz, nx))
    cf = dtype(coef)
    acoef = abs(cf.real) + abs(cf.imag)
    out = np.zeros(Ux.shape, dtype=dtype)
    mag = np.zeros(Ux.shape, dtype=real)
    for s in range(Ux.shape[0]):
        u = Ux[s].reshape((nz, nx))
        r = np.zeros((nz, nx), dtype=dtype)
        m = np.zeros((nz, nx), dtype=real)
        for k, (sz, sx) in enumerate(lags):
            us = _shift(u, sz, sx)
            r = r + Cx[k] * us
            m = m + fc._absprod(Cx[k], us).astype(real)
        out[s], mag[s] = (cf * r).ravel(), (acoef * m).ravel()
    return out, mag


def lag_imaging_reference(P0, UF, UB, nz, nx, dtype=CLD, lags=LAGS, mask=True):
    """P_k = P0_k + sum_s UB[s] (.) UF[s](i + off_k) on the interior cells, P0 elsewhere, and the magnitude |P0| + sum_s |UB||UF| the bound scales.  (9, N)."""
    real = LD if dtype is CLD else np.float64
    F = np.asarray(UF).astype(dtype)
    B = np.asarray(UB).astype(dtype)
    inside = fr._interiorMask(nz, nx) if mask else np.ones((nz, nx), dtype=bool)
    out = np.asarray(P0).astype(dtype).reshape((9, nz, nx)).copy()
    mag = (np.abs(out.real) + np.abs(out.imag)).astype(real)
    for s in range(F.shape[0]):
        f, b = F[s].reshape((nz, nx)), B[s].reshape((nz, nx))
        for k, (sz, sx) in enumerate(lags):
            fs = _shift(f, sz, sx)
            out[k] = out[k] + np.where(inside, b * fs, 0)
            mag[k] = mag[k] + np.where(inside, fc._absprod(b, fs).astype(real), 0)
    return out.reshape((9, nz * nx)), mag.reshape((9, nz * nx))


def planes_reference(op, db):
    'L[db] in 80-bit arithmetic and the magnitude (every term of the star by its modulus) the bound scales: (9, N) each'
    N = int(op.nz) * int(op.nx)
    return fr.buoyancyPlanes(op, db, dtype=CLD).reshape((9, N)), fr.buoyancyPlanes(op, db, dtype=CLD, magnitude=True).reshape((9, N))


def adjoint_reference(op, G0, P, w, conj):
    'G0 + w (conj-or-not L)^T P in 80-bit arithmetic and the magnitude |G0| + |w| |L|^T |P|'
    wx = CLD(w)
    g0 = np.asarray(G0).astype(CLD)
    ref = g0 + wx * fr.buoyancyAdjoint(op, P, dtype=CLD, conj=conj)
    mag = np.abs(g0.real) + np.abs(g0.imag) + (abs(wx.real) + abs(wx.imag)) * fr.buoyancyAdjoint(op, P, dtype=CLD, magnitude=True).real
    return ref, mag


worst_ratio = fc.worst_ratio


# ---- inputs of the kernel tests --------------------------------------------------------------------------------------------------------------------
# (nz, nx, nsrc).  nx: 3 and 4 (one or two interior cells), 61 .. 64 either side of the tile edge OP_TILE_X = 62, 125 a third tile by one cell.  nz: 3 and 4,
# LAG_ROWS - 1 = 3 and LAG_ROWS + 1 = 5 (k_lag_imaging), 33 = OP_ROWS + 1 (a second chunk of the rolling window).  nsrc: 1, 4 (one full group of OP_UNROLL), 5 (a
# partial group; a second round over the LAG_WAVES waves), 33 (more groups than waves).
KERNEL_CASES = [(3, 3, 1), (4, 4, 4), (5, 61, 5), (3, 62, 33), (4, 63, 1), (5, 64, 5), (33, 125, 4), (33, 64, 33), (33, 3, 5)]


def kernel_inputs(nz, nx, nsrc, seed=0):
    'U with columns of very different size, B, nine random planes C and a non-zero P0'
    rng = np.random.default_rng(seed)
    N = nz * nx
    U = ac.randc(rng, (nsrc, N)) * 10.0 ** rng.uniform(-3, 3, (nsrc, 1))
    B = ac.randc(rng, (nsrc, N))
    C = ac.randc(rng, (9, N))
    P0 = ac.randc(rng, (9, N))
    return U, B, C, P0


# handles the planes / adjoint kernels are run on: free-surface flags on and off, dx != dz, ky != 0, a damped frequency; nPML 2 so that 3 x 3 is legal
OPERATOR_CASES = {
    'tiny': dict(nz=3, nx=3, dx=10., dz=10., nPML=2, freq=6., freeSurf=(False, False, False, False)),
    'even': dict(nz=4, nx=4, dx=10., dz=7., nPML=2, freq=6., freeSurf=(True, False, False, True)),
    'tile': dict(nz=5, nx=63, dx=10., dz=10., nPML=3, freq=8. - 0.4j, freeSurf=(True, False, False, False), ky=0.004),
    'wide': dict(nz=33, nx=125, dx=12.5, dz=9., nPML=6, freq=7., tau=0.4, freeSurf=(False, True, True, False)),
}


def operator_config(name, seed=5):
    sc = dict(OPERATOR_CASES[name])
    rng = np.random.default_rng(seed)
    sc.update(c=rng.uniform(2000., 2600., (sc['nz'], sc['nx'])), rho=rng.uniform(1800., 2300., (sc['nz'], sc['nx'])))
    return sc


def operator_inputs(sc, seed=6):
    'db of the size of b0 and positive, random complex planes P, a non-zero G0'
    rng = np.random.default_rng(seed)
    N = sc['nz'] * sc['nx']
    db = (1.0 / sc['rho']).ravel() * rng.uniform(0.5, 1.5, N)
    return db, ac.randc(rng, (9, N)), ac.randc(rng, N)
