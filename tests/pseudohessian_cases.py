"""Shared by tests/test_pseudohessian_host.py (CPU) and tests/test_gpu_pseudohessian.py (GPU): the pseudo-Hessian diagonal of the exact derivatives
(illumination(linearisation='operator' | 'full', parameter='c' | 'rho')), its one-cell-at-a-time brute force, its 80-bit evaluation and the componentwise bound
the fp64 evaluations (numpy's and k_pseudo_hessian's) are held to.

The quantity, per cell i:   H[i] = H0[i] + alpha W[i] sum_s sum_j |r_sj|^2,   r_sj = sum_n E_i[j][n] u_s[n],   j and n in the 3 x 3 block around i.

The bound is  c_ph(nsrc) u (|H0| + alpha W M),  u = 2^-53,  M = sum_s sum_j rho_sj^2,  rho_sj = sum_n |E_i[j][n]|_mag |u_s[n]|  with |E|_mag the `magnitude`
evaluation of the planes (every term of the star by its modulus: zephyr_amd.frechet) and |u| the modulus.  The count, read off the operation tree:

  a coefficient      each component within C_COEF u |E|_mag: the velocity planes with the buoyancy planes joined are C_VPLANES_DB = 69 (tests/full_cases.py;
                     the buoyancy planes alone 48, tests/density_cases.py); the kernel scales the buoyancy star by the chain (1) and joins the two stars or
                     the mass weight of the velocity part (1) itself.                                                                   C_COEF = 69 + 2
  a row sum          at most nine complex FMAs: a component is a chain of 18 FMAs, each rounding once, relative to the running sum of moduli.    C_ROW = 18
                     So each component of r is within (C_COEF + C_ROW) u rho and |dr| <= sqrt(2) (C_COEF + C_ROW) u rho.
  its squared modulus ||r + dr|^2 - |r|^2| <= 2 |r||dr| + |dr|^2 <= 2 sqrt(2) (C_COEF + C_ROW) u rho^2 (|r| <= rho; the second-order term is 1e-28 rho^2),
                     and two squares and a sum round three times more.                                            ceil(2 sqrt(2) (C_COEF + C_ROW)) + 3 = 255
  the sums           non-negative terms: each addition is relative to the total.  Nine rows per column (9), the columns of a wave in order (at most nsrc),
                     the four waves (4).  The real weight S_i |u[i]|^2 that stands for the eight mass-only rows of the velocity star is within the same count.
                                                                                                                                          9 + nsrc + 4
  the end            alpha W (1), its product with the sum (1), the addition to H0 (1).                                                              3

A complex64 store adds C64 2^-24 alpha W M: every stored component is within 2^-24 relative of the packed one, so |du| <= 2^-24 |u|, |dr| <= 2^-24 rho and
||r + dr|^2 - |r|^2| <= (2 + 2^-24) 2^-24 rho^2.
"""
import math

import numpy as np

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
C_COEF = xc.C_VPLANES_DB + 2
C_ROW = 18
C64 = 2.0 + 2.0 ** -24


def c_ph(nsrc):
    return math.ceil(2 * math.sqrt(2) * (C_COEF + C_ROW)) + 3 + (9 + int(nsrc) + 4) + 3


# mode -> (the config has `rho`, the parameter of frechet.pseudoHessianDiagonal in the kernel's units, the mode of pseudoHessianAccumulateDevice)
MODES = {'explicit': (True, 'c', 'velocity'), 'gardner': (False, 'c', 'gardner'), 'rho': (True, 'b', 'buoyancy')}
HANDLES = ('tiny', 'even', 'tile', 'wide')


def operator(name, mode, **extra):
    "(config, operator, chain) of a handle of density_cases.OPERATOR_CASES in a mode: chain the Gardner d b / d c, or None"
    import zephyr_amd as za
    sc = xc.operator_config(name, MODES[mode][0])
    op = za.MiniZephyr(dict(sc, **extra))
    return sc, op, (fr.gardnerChain(sc['c']) if mode == 'gardner' else None)


def columns(N, nsrc, seed=0):
    "u^ (N, nsrc): random complex columns of magnitudes 1e-3 .. 1e3, as the kernel inputs of density_cases"
    rng = np.random.default_rng(seed)
    return ac.randc(rng, (N, nsrc)) * 10.0 ** rng.uniform(-3, 3, (1, nsrc))


def unit_planes(op, i, parameter, chain, dtype=np.complex128):
    "the planes of d A / d p_i: frechet.velocityPlanes(op, e_i, chain e_i), or frechet.buoyancyPlanes(op, e_i) ('b') / (op, -e_i / rho_i^2) ('rho')"
    N = int(op.nz) * int(op.nx)
    e = np.zeros(N)
    e[i] = 1.0
    if parameter == 'c':
        return fr.velocityPlanes(op, e, None if chain is None else chain * e, dtype)
    if parameter == 'rho':
        e[i] = -1.0 / float(np.ravel(op.rho)[i]) ** 2
    return fr.buoyancyPlanes(op, e, dtype)


def brute_force(op, u, parameter, chain, cells):
    "H[i] = sum_s ||(d A / d p_i) u_s||^2 for the cells given, one cell at a time"
    nz, nx = int(op.nz), int(op.nx)
    out = np.zeros(len(cells))
    for k, i in enumerate(cells):
        r = fr.applyPlanes(unit_planes(op, i, parameter, chain), u, nz, nx)
        out[k] = (np.square(r.real) + np.square(r.imag)).sum()
    return out


def sample_cells(nz, nx, npml, seed=3, extra=12):
    "every cell of a small grid; else the corners, cells on the four boundary lines and beside them, the PML edge inside and outside, the centre and a few more"
    N = nz * nx
    if N <= 64:
        return list(range(N))
    zs = sorted({0, 1, npml - 1, npml, nz // 2, nz - npml - 1, nz - npml, nz - 2, nz - 1} & set(range(nz)))
    xs = sorted({0, 1, npml - 1, npml, 61, 62, 63, nx // 2, nx - npml - 1, nx - npml, nx - 2, nx - 1} & set(range(nx)))
    cells = {z * nx + x for z in zs for x in xs}
    cells |= set(np.random.default_rng(seed).integers(0, N, extra).tolist())
    return sorted(cells)


def exact(op, u, parameter, chain):
    "(H, M), longdouble (N,): the sum in 80-bit arithmetic from the fp64 columns u^ given, and the magnitude M of the module docstring"
    return (fr.pseudoHessianDiagonal(op, u, parameter, chain, dtype=CLD), fr.pseudoHessianDiagonal(op, u, parameter, chain, dtype=CLD, magnitude=True))


def combine(HM, alpha=1.0, W=None, H0=None):
    "(ref, mag, added) from `exact`: H0 + alpha W H, |H0| + alpha W M that the bound scales, and alpha W M alone (what a store format term scales)"
    w = LD(alpha) * (LD(1) if W is None else np.asarray(W).astype(LD))
    h0 = LD(0) if H0 is None else np.asarray(H0).astype(LD)
    return h0 + w * HM[0], np.abs(h0) + w * HM[1], w * HM[1]


def reference(op, u, parameter, chain, alpha=1.0, W=None, H0=None):
    "combine(exact(...), ...)"
    return combine(exact(op, u, parameter, chain), alpha, W, H0)


def worst_ratio(got, ref, bound):
    "max over cells of |got - ref| / bound (0 / 0 counts as 0), non-finite results infinite"
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float('inf')
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max())


# ---- deliberately wrong evaluations -------------------------------------------------------------------------------------------------------------------
def wrong(op, u, parameter, chain, how):
    """plain fp64 with one thing wrong.  'no_stretch': the PML stretch left out of the velocity planes (the mass term alone; for the buoyancy the stiffness
    averages left out: density_cases.mass_only_planes).  'own_row': only row i kept, the eight rows around it dropped.  'transposed': the lags transposed,
    plane k paired with the offset of 8 - k."""
    nz, nx = int(op.nz), int(op.nx)
    ua = np.asarray(u).reshape((nz * nx, -1))
    ch = chain
    if parameter == 'c':
        planes = lambda v: fr.velocityPlanes(op, v, None if ch is None else ch * v)
    else:
        planes = lambda v: fr.buoyancyPlanes(op, v)
    if how == 'no_stretch':
        if parameter == 'c':
            base = lambda v: xc.mass_only_planes(op, v) + (0 if ch is None else fr.buoyancyPlanes(op, ch * v))
        else:
            base = lambda v: dc.mass_only_planes(op, v)
        return fr.colourSum(nz, nx, base, ua)
    if how == 'own_row':
        return fr.colourSum(nz, nx, planes, ua, box=False)
    if how == 'transposed':
        return fr.colourSum(nz, nx, lambda v: planes(v)[::-1], ua)
    raise ValueError(how)


def layer_cells(sc):
    "bool (N,): the cells whose 3 x 3 block touches an absorbing layer (where the stretch factors depend on c)"
    nz, nx, n = sc['nz'], sc['nx'], sc['nPML']
    z, x = np.divmod(np.arange(nz * nx), nx)
    return (z - 1 < n) | (z + 1 >= nz - n) | (x - 1 < n) | (x + 1 >= nx - n)
