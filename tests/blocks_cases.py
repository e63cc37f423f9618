"""Shared by tests/test_blocks_host.py (CPU) and tests/test_gpu_blocks.py (GPU): the per-cell 2 x 2 blocks of the joint (c, rho) Hessian (hessianBlocks), the
cross entries of Hvec(parameter='joint') they are checked against, their brute forces, the 80-bit evaluations of the two device kernels and the componentwise
bounds those are held to.

The bounds.  u = 2^-53; every row of a block has its own magnitude evaluation M (frechet.*Blocks(magnitude=True): every factor by its modulus, the cross term
with +1 / rho^2), and the bound of a row is C u (|H0| + alpha M) of that row.

  k_gauss_newton_blocks    the operation tree of k_gauss_newton_diagonal (gaussnewton_cases.C_GN: three coefficient errors of C_COEF, T = E Phi 18, S = Gamma T 18, the
                           sum of conj(E) S over at most 33 coefficients 66) for each of the three sums -- the cross sum pairs conj(E^c) with the S of E^b and has the
                           17 velocity terms only.  The end takes five roundings where the diagonal takes three: rho^2 (1), rho^4 (1), alpha over it (1), the product
                           (1), the addition to H0 (1).                                                     C_GNB = 3 C_COEF + 18 + 18 + 66 + 5
  k_pseudo_hessian_blocks  pseudohessian_cases counts a row sum within (C_COEF + C_ROW) u rho per component.  The weighted sum of the eight buoyancy rows that the
                           cross term of the neighbouring velocity rows uses adds four edge rows (4), scales (1), four corner rows (4), scales (1) and joins (1):
                           within (C_COEF + C_ROW + 11) u sum_j m_o rho_j; the other factor, conj(w) v[4], is within less.  A product Re conj(a) b of two such
                           sums is within 2 sqrt(2) (C_COEF + C_ROW + 11) u rho_a rho_b, and its two products and one sum round three times more -- the squared
                           moduli of rows 0 and 2 are the case a = b.  The sums: at most nine terms per column (9), the columns of a wave in order (at most nsrc),
                           the four waves (4), each relative to the running sum of moduli, which M bounds.  The end: five, as above.
                                                                     c_phb(nsrc) = ceil(2 sqrt(2) (C_COEF + C_ROW + 11)) + 3 + (9 + nsrc + 4) + 5
                           A complex64 store adds C64 2^-24 alpha M: |dr| <= 2^-24 rho for both factors of every product (pseudohessian_cases.C64).
"""
import math

import numpy as np

from tests import gaussnewton_cases as gc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

LD, CLD, U64 = gc.LD, gc.CLD, gc.U64
C64 = pc.C64
C_GNB = 3 * pc.C_COEF + 18 + 18 + 66 + 5
LINS = {'full': True, 'operator': False}          # linearisation -> the `stretch` of the kernels


def c_phb(nsrc):
    return math.ceil(2 * math.sqrt(2) * (pc.C_COEF + pc.C_ROW + 11)) + 3 + (9 + int(nsrc) + 4) + 5


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------------
def hvec_cross(prob, uF, cells, linearisation):
    "(Hvec([0; e_i])[i], Hvec([e_i; 0])[N + i]) of parameter='joint' for the cells given: the two places the cross entry of a block appears in the operator"
    N = prob.nrow
    a, b = np.zeros(len(cells)), np.zeros(len(cells))
    for k, i in enumerate(cells):
        e = np.zeros(2 * N)
        e[N + i] = 1.0
        a[k] = prob.Hvec(None, e, u=uF, linearisation=linearisation, parameter='joint')[i]
        e = np.zeros(2 * N)
        e[i] = 1.0
        b[k] = prob.Hvec(None, e, u=uF, linearisation=linearisation, parameter='joint')[N + i]
    return a, b


def cross_error(got, want, scale):
    "max over cells of |got - want| / scale, scale = sqrt(B0 B2) of the cell; where want is exactly 0 got must be exactly 0"
    got, want, scale = (np.asarray(x, dtype=np.float64) for x in (got, want, scale))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(want != 0, np.abs(got - want) / np.where(scale > 0, scale, 1), np.where(got != 0, np.inf, 0))
        r = np.where((want != 0) & (scale <= 0), np.inf, r)
    return float(r.max())


def coherence(B):
    "B1 / sqrt(B0 B2) where both diagonals are positive, 0 elsewhere"
    s = np.sqrt(B[0] * B[2])
    return np.where(s > 0, B[1] / np.where(s > 0, s, 1), 0.0)


def gram_properties(B, slack=1e-10):
    "every block is a Gram matrix: non-negative diagonals, B1^2 <= B0 B2 (1 + slack), and B1 exactly 0 where a diagonal is exactly 0"
    B = np.asarray(B)
    zero = (B[0] == 0) | (B[2] == 0)
    return bool(np.all(B[0] >= 0) and np.all(B[2] >= 0) and np.all(B[1] * B[1] <= B[0] * B[2] * (1 + slack)) and np.all(B[1][zero] == 0))


def brute_force(prob, sv, uF, cells, linearisation):
    """(3, len(cells)): |scaleTerm|^2 sum_f sum_s sum_r Re conj(g_r^T E^a_i u^_s) (g_r^T E^b_i u^_s) for (a, b) = (c, c), (c, rho), (rho, rho): gaussnewton_cases.brute_force
    extended to the cross product, g_r from a sparse LU of the transposed oracle matrix and E_i u^ by applyPlanes on the planes along e_i"""
    st = complex(prob.system.scaleTerm)
    out = np.zeros((3, len(cells)))
    for ifreq, sub in enumerate(prob.system.subProblems):
        g = gc.transposed_greens(prob, sv, ifreq)
        uh = np.conj(np.asarray(uF[ifreq]) / st)
        for k, i in enumerate(cells):
            dc = g.T @ fr.applyPlanes(gc.unit_planes(prob, sub, i, linearisation, 'c'), uh, sub.nz, sub.nx)
            dr = g.T @ fr.applyPlanes(gc.unit_planes(prob, sub, i, 'operator', 'rho'), uh, sub.nz, sub.nx)
            out[:, k] += abs(st) ** 2 * np.array([float((np.abs(dc) ** 2).sum()), float((np.conj(dc) * dr).real.sum()), float((np.abs(dr) ** 2).sum())])
    return out


def ph_brute_force(op, u, linearisation, cells):
    "(3, len(cells)): sum_s Re <E^a_i u_s, E^b_i u_s> one cell at a time, the planes of pseudohessian_cases.unit_planes (frechet.massPlanes for 'operator')"
    nz, nx = int(op.nz), int(op.nx)
    out = np.zeros((3, len(cells)))
    for k, i in enumerate(cells):
        if linearisation == 'operator':
            e = np.zeros(nz * nx)
            e[i] = 1.0
            Pc = fr.massPlanes(op, e)
        else:
            Pc = pc.unit_planes(op, i, 'c', None)
        rc = fr.applyPlanes(Pc, u, nz, nx)
        rr = fr.applyPlanes(pc.unit_planes(op, i, 'rho', None), u, nz, nx)
        out[:, k] = [(np.abs(rc) ** 2).sum(), (np.conj(rc) * rr).real.sum(), (np.abs(rr) ** 2).sum()]
    return out


def unit_blocks(op, B):
    "(cc, cb, bb) in buoyancy units from the rows of a block in density units: cb = -B1 rho^2, bb = B2 rho^4"
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64), (int(op.nz), int(op.nx))).ravel()
    return B[0], -B[1] * rho ** 2, B[2] * rho ** 4


# ---- the kernels in 80-bit arithmetic ---------------------------------------------------------------------------------------------------------------------
def _rows(alpha, H, H0, real):
    return np.asarray(H0).astype(real) + real(alpha) * H


def gn_reference(op, Cu, Cg, linearisation, alpha, H0, dtype=CLD):
    """(ref, mag), (3, N) each: H0 + alpha B and |H0| + alpha M with B = frechet.gaussNewtonBlocks on the planes Cu, Cg of the UNCONJUGATED solves (the kernel is fed
    their conjugates and conjugates its coefficients, which leaves the real traces as they are) and M its magnitude evaluation"""
    real = LD if dtype is CLD else np.float64
    B = fr.gaussNewtonBlocks(op, Cu, Cg, linearisation, dtype=dtype)
    M = fr.gaussNewtonBlocks(op, Cu, Cg, linearisation, dtype=dtype, magnitude=True)
    return _rows(alpha, B, H0, real), _rows(alpha, M, np.abs(H0), real)


def ph_reference(op, u, linearisation, alpha, H0, dtype=CLD):
    "(ref, mag, added), (3, N) each: H0 + alpha B, |H0| + alpha M and alpha M alone (what the store format term scales) with B = frechet.pseudoHessianBlocks"
    real = LD if dtype is CLD else np.float64
    B = fr.pseudoHessianBlocks(op, u, linearisation, dtype=dtype)
    M = fr.pseudoHessianBlocks(op, u, linearisation, dtype=dtype, magnitude=True)
    return _rows(alpha, B, H0, real), _rows(alpha, M, np.abs(H0), real), real(alpha) * M


def worst_rows(got, ref, bound):
    "pseudohessian_cases.worst_ratio per row of a block: [cc, crho, rhorho]"
    return [pc.worst_ratio(np.asarray(got)[a], ref[a], bound[a]) for a in range(3)]


# ---- deliberately wrong evaluations -----------------------------------------------------------------------------------------------------------------------
def _velocity_planes(op, linearisation):
    return (lambda v: fr.massPlanes(op, v)) if linearisation == 'operator' else (lambda v: fr.velocityPlanes(op, v))


def _density_rows(op, cc, cb, bb, sign=-1.0):
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64), (int(op.nz), int(op.nx))).ravel()
    return np.stack([cc, sign * cb / rho ** 2, bb / rho ** 4])


def gn_wrong(op, Cu, Cg, linearisation, how):
    """frechet.gaussNewtonBlocks in plain fp64 with one thing wrong.  'conjugate': the conjugate on the wrong factor of the cross term.  'own_row': the cross term
    without the neighbouring rows of the velocity coefficients.  'sign': +1 / rho^2 for -1 / rho^2.  'gamma_transposed': Gamma^T for Gamma.  None: nothing wrong."""
    nz, nx = int(op.nz), int(op.nx)
    Ec = fr.blockCoefficients(nz, nx, _velocity_planes(op, linearisation))
    Eb = fr.blockCoefficients(nz, nx, lambda v: fr.buoyancyPlanes(op, v))
    Gamma, Phi = fr._gramBlocks(Cg, nz, nx), fr._gramBlocks(Cu, nz, nx)
    if how == 'gamma_transposed':
        Gamma = np.swapaxes(Gamma, 1, 2)
    cc = fr.gaussNewtonCrossTrace(Ec, Gamma, Ec, Phi)
    bb = fr.gaussNewtonCrossTrace(Eb, Gamma, Eb, Phi)
    Ex = Ec
    if how == 'conjugate':
        Ex = np.conj(Ec)
    elif how == 'own_row':
        Ex = np.zeros_like(Ec)
        Ex[:, 4, :] = Ec[:, 4, :]
    cb = fr.gaussNewtonCrossTrace(Ex, Gamma, Eb, Phi)
    return _density_rows(op, cc, cb, bb, 1.0 if how == 'sign' else -1.0)


def ph_wrong(op, u, linearisation, how):
    "frechet.pseudoHessianBlocks in plain fp64 with one thing wrong: 'conjugate', 'own_row', 'sign' as for `gn_wrong`; None: nothing wrong"
    nz, nx = int(op.nz), int(op.nx)
    N = nz * nx
    ua = np.asarray(u).reshape((N, -1))
    planesC = _velocity_planes(op, linearisation)
    iz, ix = np.divmod(np.arange(N), nx)
    out = np.zeros((3, N))
    for a in range(3):
        for b in range(3):
            mine = (iz % 3 == a) & (ix % 3 == b)
            if not mine.any():
                continue
            ind = mine.astype(np.float64)
            rc = fr.applyPlanes(planesC(ind), ua, nz, nx)
            rb = fr.applyPlanes(fr.buoyancyPlanes(op, ind), ua, nz, nx)
            cross = ((rc if how == 'conjugate' else np.conj(rc)) * rb).real.sum(axis=1).reshape((nz, nx))
            terms = ((np.abs(rc) ** 2).sum(axis=1).reshape((nz, nx)), cross, (np.abs(rb) ** 2).sum(axis=1).reshape((nz, nx)))
            for k, e in enumerate(terms):
                out[k, mine] = (e if (k == 1 and how == 'own_row') else fr._boxSum(e, nz, nx)).ravel()[mine]
    return _density_rows(op, out[0], out[1], out[2], 1.0 if how == 'sign' else -1.0)
