"""Shared by tests/test_newton_host.py (CPU) and tests/test_gpu_newton.py (GPU): the full Newton Hessian-vector product (Hvec with resid=) on the 37 x 53 survey of
tests/frechet_cases.py, and the 80-bit evaluations of the two device kernels with the componentwise bounds they are held to.

The bounds, in the style of tests/full_cases.py: c u m per component, u = 2^-53, m the `magnitude` evaluation of zephyr_amd.frechet (every term by its modulus), c a
count of roundings read off the code, generously:

  k_velocity_curvature  a twice-differentiated row factor: the denominator (3), a Smith division (6) and a square (3) for X -- 12 -- a scaling and a second
                        division for X a / den (7): 19, a scaling and a third division for d2X / dc2 (7): 26.  For d2p / dc2 the product with c (3: 29), the
                        scaling of X a / den by 6 (1 on 19), the join (1: 30), the constant 2 f d s and its product (4: 34), the last division (6): 40.  Through
                        the constants of mz_stiffness (4); per term a difference of planes, a product and for a corner one more multiply-add (6); the average of
                        two 1 / rho and its product (4); d2 kappa / dc2 b: omega_d^2 (3), c^2 and c^4 (6), the scaling (1), a Smith division (6), 1 / rho and the
                        product (2): 18; running sums of 8 stretch terms and of 9 mass terms of a product and an addition each (26); the join of the two parts
                        (4), the product with p (1), the product with w and the addition into G (4).
                                                                                                     C_CURVATURE = 40 + 4 + 6 + 4 + 18 + 26 + 4 + 1 + 4
  k_stencil_sources_t   the nine-term sum is the chain of 18 FMAs of k_stencil_sources (conjugating a plane is exact), the product with coef 3.
                                                                                                                             C_STENCIL_T = 18 + 3
                        With accumulate the conjugate (exact) is added to R: one more rounding, and |R0| joins the magnitude.
  k_mass_planes         d kappa / dc: omega_d^2 (3), c^3 (6), a Smith division (6): 15; dc / rho (1), the mass weight (1), the product (1).      C_MPLANES = 15 + 3
  k_velocity_adjoint    without its stretch part (helm_mass_adjoint_device): full_cases.C_VADJOINT bounds it, the magnitude that of the mass term alone.
A complex64 store adds 2^-24 m, as in tests/density_cases.py.
"""
import numpy as np

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
C_CURVATURE = 40 + 4 + 6 + 4 + 18 + 26 + 4 + 1 + 4
C_STENCIL_T = 18 + 3
C_MPLANES = 15 + 3
C_VADJOINT = xc.C_VADJOINT
SECOND = 3.5                    # the window of the Taylor tests of test_frechet_host.py / test_full_host.py: factors >= 3.5 are second order
STALL = 1.2                     # ... and a remainder that does not converge keeps its size: factors below this

pair = xc.pair
everywhere = xc.perturbation            # uniform in +-50, non-zero in every cell: boundary lines and absorbing layers included
outside_layers = fc.perturbation        # the same amplitude, zero in the absorbing layers and on the boundary
OFFSET = 40.0                           # dobs is the data of the model shifted by this much (m/s): ||H p - J^T J p|| / ||H p|| = 0.72 on the fixed MiniZephyr case


def observed(prob, sv, c0):
    'dobs: the data of c0 + OFFSET, a model far enough for the residual part of the Hessian to show; the model is put back'
    dobs = sv.dpred(np.array(c0) + OFFSET)
    prob.updateModel(np.array(c0))
    return dobs


def gradient_of(prob, sv, dobs, **kw):
    'c -> g(c) = Jtvec(c, dpred(c) - dobs, adjoint=\'transpose\') at fixed dobs; with parameter=\'rho\' the argument is the density and c stays the config\'s'
    if kw.get('parameter', 'c') == 'rho':
        def g(rho):
            m = {'rho': np.array(rho, dtype=np.float64)}
            return prob.Jtvec(m, sv.dpred(m) - dobs, adjoint='transpose', **kw)
        return g
    return lambda c: prob.Jtvec(c, sv.dpred(c) - dobs, adjoint='transpose', **kw)


def central_remainders(g, m0, p, Hp, keep=None, hs=fc.TAYLOR_H):
    '||(g(m0 + h p) - g(m0 - h p)) / 2h - Hp|| for h in hs, over the cells `keep` (default all)'
    keep = slice(None) if keep is None else keep
    return [fc.norm((fc.central(g, m0, p, h) - Hp)[keep]) for h in hs]


# ---- the two kernels in 80-bit arithmetic -----------------------------------------------------------------------------------------------------------
def curvature_reference(op, G0, P, p, w, conj, stretch):
    'G0 + w p (.) (conj-or-not d2A)^T P in 80-bit arithmetic and the magnitude |G0| + |w| |p| |d2A|^T |P|'
    wx = CLD(w)
    g0 = np.asarray(G0).astype(CLD)
    ref = g0 + wx * fr.velocityCurvature(op, P, p, conj=conj, stretch=stretch, dtype=CLD)
    mag = np.abs(g0.real) + np.abs(g0.imag) + (abs(wx.real) + abs(wx.imag)) * fr.velocityCurvature(op, P, p, stretch=stretch, dtype=CLD, magnitude=True).real
    return ref, mag


def stencil_t_reference(U, C, coef, nz, nx, conj, dtype=CLD):
    """R[s] = coef (conj-or-not C)^T U[s] through frechet.applyPlanesTransposed and the magnitude |coef| |C|^T |U| the bound scales.  U (nsrc, N), C (9, N)."""
    real = LD if dtype is CLD else np.float64
    Ux = np.asarray(U).astype(dtype).T
    Cx = np.asarray(C).astype(dtype)
    if conj:
        Cx = np.conj(Cx)
    cf = dtype(coef)
    out = cf * fr.applyPlanesTransposed(Cx, Ux, nz, nx)
    parts = lambda a: (np.abs(a.real) + np.abs(a.imag)).astype(real)
    mag = (abs(cf.real) + abs(cf.imag)) * fr.applyPlanesTransposed(parts(Cx), parts(Ux), nz, nx)
    return out.T, mag.T


def mass_planes_reference(op, v):
    'the planes of the mass term alone in 80-bit arithmetic and their magnitude: (9, N) each'
    N = int(op.nz) * int(op.nx)
    return fr.massPlanes(op, v, dtype=CLD).reshape((9, N)), fr.massPlanes(op, v, dtype=CLD, magnitude=True).reshape((9, N))


def mass_adjoint_reference(op, G0, P, w, conj):
    'G0 + w (conj-or-not M)^T P in 80-bit arithmetic, M the mass term alone, and the magnitude |G0| + |w| |M|^T |P|'
    wx = CLD(w)
    g0 = np.asarray(G0).astype(CLD)
    ref = g0 + wx * fr.velocityAdjoint(op, P, dtype=CLD, conj=conj, stretch=False)
    mag = np.abs(g0.real) + np.abs(g0.imag) + (abs(wx.real) + abs(wx.imag)) * fr.velocityAdjoint(op, P, dtype=CLD, magnitude=True, stretch=False).real
    return ref, mag


def stencil_t_accumulated(R0, ref, mag):
    'R0 + conj(ref) and the magnitude |R0| + mag: what the accumulate mode of the transposed stencil leaves in R'
    r0 = np.asarray(R0).astype(CLD)
    return r0 + np.conj(ref), np.abs(r0.real) + np.abs(r0.imag) + mag


def stencil_t_without_a_lag(U, C, coef, nz, nx, conj, skip=5):
    'the plain fp64 evaluation with one of the nine terms left out: a wrong one'
    Cx = np.array(C, dtype=np.complex128)
    Cx[skip] = 0
    return stencil_t_reference(U, Cx, coef, nz, nx, conj, dtype=np.complex128)[0]


def curvature_inputs(sc, seed=9):
    'p uniform in +-50 and non-zero everywhere, random complex planes P and a non-zero G0 of the size of what is added to it: 6 |omega|^2 / (c^4 rho) |p| m_c'
    rng = np.random.default_rng(seed)
    N = sc['nz'] * sc['nx']
    p = 50. * rng.uniform(-1., 1., N)
    p[np.abs(p) < 1.] = 1.
    cm = float(np.mean(sc['c']))
    size = 6. * abs(2. * np.pi * complex(sc['freq'])) ** 2 / (cm ** 4 * float(np.mean(sc['rho']))) * 50.
    return p, ac.randc(rng, (9, N)), size * ac.randc(rng, N)


worst_ratio = fc.worst_ratio
KERNEL_CASES = dc.KERNEL_CASES
kernel_inputs = dc.kernel_inputs
