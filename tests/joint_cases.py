"""Shared by tests/test_joint_host.py (CPU) and tests/test_gpu_joint.py (GPU): the stacked (c, rho) routes, parameter='joint', on the 37 x 53 survey of
tests/frechet_cases.py, and the 80-bit evaluations of the two device kernels of the mixed second derivative with the componentwise bounds they are held to.

The bounds, in the style of tests/full_cases.py and tests/newton_cases.py: c u m per component, u = 2^-53, m the `magnitude` evaluation of zephyr_amd.frechet (every
term by its modulus), c a count of roundings read off the code, generously:

  k_velocity_adjoint_b  k_velocity_adjoint (full_cases.C_VADJOINT = 33 + 4 + 6 + 4 + 17 + 26 + 4 + 4) with the buoyancy read from an array and never inverted: the
                        average of two entries and its product are 2 roundings, not 4, and (d kappa / dc) B one less than with 1 / rho.
                                                                                                  C_VADJOINT_B = 33 + 4 + 6 + 2 + 16 + 26 + 4 + 4
  k_mixed_adjoint       per row the differentiated factors (33) through the constants of mz_stiffness (4); per term a difference of planes, a product and for a
                        corner one more multiply-add (6); the running sum of the centre row's eight terms (8); the product with p of the row (1); the running sum
                        over the nine rows (9; the halving is exact).  d kappa / dc: omega_d^2 (3), c^3 (6), a Smith division (6), then its product with p (1):
                        16; the mass gather of nine terms, a product and an addition each (18); the join of the two parts (4: a complex multiply-add), the product
                        with w and the addition into G (4).                              C_MIXED = 33 + 4 + 6 + 8 + 1 + 9 + 16 + 18 + 4 + 4
"""
import numpy as np

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import newton_cases as nc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
C_VADJOINT_B = 33 + 4 + 6 + 2 + 16 + 26 + 4 + 4
C_MIXED = 33 + 4 + 6 + 8 + 1 + 9 + 16 + 18 + 4 + 4
SECOND, STALL = nc.SECOND, nc.STALL

pair = xc.pair
OFFSET = nc.OFFSET              # dobs is the data of the model with c + 40 m/s ...
DENSITY_FACTOR = 1.03           # ... and rho x 1.03: far enough for the residual part and for the mixed terms of the Hessian to show


def model():
    'c0, rho0 of the 37 x 53 case, float64 (nz, nx) each'
    c, rho = fc.model()
    return np.array(c, dtype=np.float64), np.array(rho, dtype=np.float64)


def both(c, rho):
    return {'c': np.array(c, dtype=np.float64), 'rho': np.array(rho, dtype=np.float64)}


def restore(prob):
    prob.updateModel(both(*model()))


def observed(prob, sv):
    'dobs: the data of (c0 + OFFSET, rho0 DENSITY_FACTOR); the model is put back'
    c0, rho0 = model()
    dobs = sv.dpred(both(c0 + OFFSET, rho0 * DENSITY_FACTOR))
    restore(prob)
    return dobs


def stack(vc, vrho):
    return np.concatenate((np.asarray(vc, dtype=np.float64).ravel(), np.asarray(vrho, dtype=np.float64).ravel()))


def directions(layers=False):
    '(v_c, v_rho), (N,) each: uniform in +-50; v_c non-zero in every cell, or (layers) zero in the absorbing layers and on the boundary'
    return (nc.outside_layers() if layers else nc.everywhere()).ravel(), dc.perturbation().ravel()


def gradient_of(prob, sv, dobs, **kw):
    'h -> g(c0 + h v_c, rho0 + h v_rho) along a stacked direction v: the joint gradient at fixed dobs, float64 (2N,)'
    c0, rho0 = model()
    N = c0.size

    def g(v, h):
        m = both(c0 + h * v[:N].reshape(c0.shape), rho0 + h * v[N:].reshape(rho0.shape))
        return prob.Jtvec(m, sv.dpred(m) - dobs, adjoint='transpose', parameter='joint', **kw)
    return g


def central_remainders(g, v, Hv, N, keep=None, hs=fc.TAYLOR_H):
    '[(||.|| over the c half, ||.|| over the rho half) of (g(+h) - g(-h)) / 2h - Hv for h in hs]; keep: the cells of the c half that are compared (default all)'
    keep = slice(None) if keep is None else keep
    out = []
    for h in hs:
        d = (g(v, h) - g(v, -h)) / (2 * h) - Hv
        out.append((fc.norm(d[:N][keep]), fc.norm(d[N:])))
    return out


# ---- the two kernels in 80-bit arithmetic -----------------------------------------------------------------------------------------------------------
def mixed_inputs(sc, seed=14):
    """p uniform in +-50 with zeros and both signs, a buoyancy perturbation B of the size of 1 / rho with zeros and both signs, random complex planes P and a
    non-zero G0 of the size of what either kernel adds to it: |d kappa / dc| |B| |p| m_c at the mean model"""
    rng = np.random.default_rng(seed)
    N = sc['nz'] * sc['nx']
    p = 50. * rng.uniform(-1., 1., N)
    B = rng.uniform(-1., 1., N) / float(np.mean(sc['rho']))
    if N > 9:                   # (the 3 x 3 grid has one interior row: its p and B stay non-zero, so that the kernels have something to add)
        p[rng.integers(0, N, max(1, N // 16))] = 0.
        B[rng.integers(0, N, max(1, N // 16))] = 0.
    cm = float(np.mean(sc['c']))
    size = 2. * abs(2. * np.pi * complex(sc['freq'])) ** 2 / (cm ** 3 * float(np.mean(sc['rho']))) * 50.
    return p, B, ac.randc(rng, (9, N)), size * ac.randc(rng, N)


def _with_magnitude(fn, G0, w):
    wx = CLD(w)
    g0 = np.asarray(G0).astype(CLD)
    return g0 + wx * fn(False), np.abs(g0.real) + np.abs(g0.imag) + (abs(wx.real) + abs(wx.imag)) * fn(True).real


def mixed_b_reference(op, G0, P, p, w, conj, stretch):
    'G0 + w (conj-or-not M_b[p])^T P in 80-bit arithmetic (k_mixed_adjoint) and the magnitude |G0| + |w| |M_b[p]|^T |P|'
    return _with_magnitude(lambda mag: fr.mixedAdjointB(op, P, p, conj=conj and not mag, stretch=stretch, dtype=CLD, magnitude=mag), G0, w)


def mixed_c_reference(op, G0, P, B, w, conj, stretch):
    'G0 + w (conj-or-not M_c[B])^T P in 80-bit arithmetic (k_velocity_adjoint_b) and the magnitude |G0| + |w| |M_c[B]|^T |P|'
    return _with_magnitude(lambda mag: fr.mixedAdjointC(op, P, B, conj=conj and not mag, stretch=stretch, dtype=CLD, magnitude=mag), G0, w)


def _row_terms(op, P, p, conj):
    '{lag o: Q_o (nz, nx)} of mixedAdjointB: the coefficient of the average of lag o in row i, with the stiffness factors p_i d row_i / dc; and the shape'
    nz, nx = int(op.nz), int(op.nx)
    v = np.asarray(p, dtype=np.float64).reshape((nz, nx))
    drow = [x * v for x in fr.rowFactorsDc(op)]
    if conj:
        drow = [np.conj(x) for x in drow]
    t, tzx = fr._stiffness(op, drow)
    Pl = np.asarray(P).astype(np.complex128).reshape((9, nz, nx)).copy()
    Pl[:, ~fr._interiorMask(nz, nx)] = 0
    slot = {o: k for k, o in enumerate(fr.LAGS)}
    q = {}
    for o in fr.LAGS:
        if o == (0, 0):
            continue
        sz, sx = o
        q[o] = t[o] * (Pl[slot[o]] - Pl[4])
        if sz and sx:
            q[o] = q[o] + tzx * (Pl[slot[(sz, 0)]] - Pl[slot[(0, sx)]])
    return q


def mixed_b_without_the_centre_row(op, P, p, conj):
    'frechet.mixedAdjointB in plain fp64 with the eight averages of the row of the cell itself left out: a wrong transpose'
    q = _row_terms(op, P, p, conj)
    return fr.mixedAdjointB(op, P, p, conj=conj) - sum(q[o] for o in q).ravel() / 2


def mixed_b_with_p_of_the_cell(op, P, p, conj):
    'frechet.mixedAdjointB in plain fp64 with p_j, the perturbation at the cell that gathers, in the place of p_i of the row in the stiffness part: a wrong transpose'
    one = np.ones(np.size(p))
    stiff = fr.mixedAdjointB(op, P, one, conj=conj) - fr.mixedAdjointB(op, P, one, conj=conj, stretch=False)
    return np.asarray(p, dtype=np.float64).ravel() * stiff + fr.mixedAdjointB(op, P, p, conj=conj, stretch=False)


worst_ratio = fc.worst_ratio
