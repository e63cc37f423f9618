"""Shared by tests/test_hessian3d_host.py (CPU) and tests/test_gpu_hessian3d.py (GPU): the problem / survey pairs with hessian3D=True, one-cell brute force
through the derivative maps of frechet3d.py, and the extended-precision references of the two kernels of csrc/survey3d_hessian.hip with their rounding
bounds -- all counted here, before anything ran on a GPU."""
import numpy as np

from zephyr_amd import frechet3d
from tests import survey3d_cases as s3
from tests import survey3d_density_cases as d3c

U53 = s3.U53

# ---- the rounded operations of the two kernels -------------------------------------------------------------------------------------------------------------
# Every bound is c u (majorant); the majorant is the same sum with every term by |Re| + |Im| (frechet3d's magnitude=True), which bounds each COMPONENT of the
# complex terms, so the counts below are componentwise.  Already counted in tests/survey3d_density_cases.py: 36 u for the two evaluations of the stretch tables
# (handle against numpy), 19 u for the operations of lap3_sum, 14 u for kappa (both relative to their own majorants).
#
# k_ph3_coefficients, per cell:
#   lap_{-d}(i + d): the tables (36), the rounded constants m m / h^2 (4), a product and two additions (3): 43 u of its majorant
#   a_p = 1/2 lap + kappa mu: kappa (14), mu (3), the product (1): 18 u of |kappa|_1 mu; the addition (1; the halving is exact): 44 u               -> 48 u of am
#   chi = -2 kappa b / c: kappa (14), b (1), the product (1), the division through conj(c) / |c|^2 (8): 24 u of |chi|_1
#   g = -b / (4 Re c): 2 u.  Gardner row: chi mu (24 + 4), g a_p (48 + 2 + 1), their addition (1): 52 u                                             -> 56 u of qm
#   A0 is a_i or the Gardner row of the centre: 56 u of its majorant; h = 1/2 (exact) or g / 2 (2 u)                                                -> 4 u of |h|
#   S' = sum_{d != 0} |q_d|^2: a component off by 56 u qm moves its square by 2 * 56 u qm^2, two components 224 u qm^2; the squares and their addition
#   3 u of 2 qm^2; 26 additions: 224 + 6 + 26 = 256 u                                                                                              -> 272 u of S'm
#   C' = sum_{d != 0} mu a_p: 48 + 3 + 1 + 26 = 78 u                                                                                                -> 96 u of C'm
#   Smu = sum mu^2: mu^2 (7), 27 additions: 34 u                                                                                                    -> 48 u of Smu
COEF_ULPS = dict(A0=56, h=4, S=272, C=96, Smu=48)
# k_ph3_moments, per cell and column:
#   T = (L u^)_i: 36 + 19 = 55 u of its majorant Tm; r = A0 u + h T: the product A0 u (56 + 3 u of A0m |u|_1), h T (55 + 2 + 1 u of |h| Tm), the addition (1):
#   61 u of rm = A0m |u|_1 + |h| Tm                                                                                                                   -> 64 u of rm
#   |r|^2: 4 * 64 u rm^2 from r, 3 u of 2 rm^2 from the squares and their addition; the running sum over k columns k u of 2 Dm: (262 + 2 k) u of Dm = sum rm^2
#   E = sum |u|^2: (3 + k) u of Em = sum |u|_1^2.   S' E: 272 + 3 + k + 1.   H = S' E + D: max(276 + k, 262 + 2 k) + 1; alpha W (2); the addition into H0 (1):
#   at most (280 + 2 k) u of |H0| + alpha W (S'm Em + Dm)
#   blocks, H_cc = |chi|^2 Smu E: |chi|^2 (4 * 24 + 6), Smu (48), E (3 + k), two products (2), alpha W (2), H0 (1): (158 + k) u
#   blocks, H_crho: C' E (96 + 3 + k + 1); Y = sum conj(u) r (64 + 3 + k u of Ym = sum |u|_1 rm), mu_0 Y (4): their addition (1): (101 + k) u; Re conj(chi) x
#   (24 + 3), b^2 (3), alpha W (2), the products (2), H0 (1): (136 + k) u of |H0| + alpha W b^2 |chi|_1 (C'm Em + mu_0 Ym)
#   blocks, H_rhorho = b^4 (S' E + D): (277 + 2 k) + b^4 (7) + the product (1) + alpha W (2) + H0 (1)                                               -> (288 + 2 k) u
# One figure for every row and mode:
def moments_ulps(k):
    return 288 + 2 * k


# Two fp64 evaluations of the same quantity on the host (the moments route, the 27-colour evaluation, one-cell brute force) each stay inside that count -- the
# sparse products of the derivative maps form plain sums of at most 27 terms per row, fewer rounded operations than counted above, and there the tables are
# the same numpy arrays on both sides --, so two of them differ by at most twice the bound.
def host_bound(k, majorant):
    return 2 * moments_ulps(k) * U53 * majorant


def host_pair(grid, mode='fixed', gardner=False, **extra):
    'survey3d_density_cases.host_pair (derivatives3D=True) with hessian3D=True'
    return d3c.host_pair(grid, mode, gardner, **dict(dict(hessian3D=True), **extra))


def fields_of(prob):
    '[u^ (N, nsrc) per frequency] and the host list of fields() of a host pair'
    st = complex(prob.system.scaleTerm)
    F = prob.fields(None)
    return [np.conj(np.asarray(f) / st) for f in F], F


def brute_force(op, uh, cells, chain=None):
    """{'cc', 'cb', 'bb' (, 'total')}: sum_s ||.||^2 and Re <., .> of the columns of the derivative maps along the unit vector of each cell in `cells` -- velocity
    at fixed density, buoyancy, and (chain = d b / d c given) their Gardner combination"""
    N = int(np.prod(op.modelDims))
    L, M = frechet3d.lapStencil3(op), frechet3d.massStencil3(op.modelDims)
    out = {n: np.zeros(len(cells)) for n in ('cc', 'cb', 'bb', 'total')}
    for j, i in enumerate(cells):
        e = np.zeros(N)
        e[i] = 1.0
        vc, vb = frechet3d.bornSources3(op, e, uh, M), frechet3d.buoyancySources3(op, e, uh, L, M)
        out['cc'][j], out['bb'][j], out['cb'][j] = (abs(vc) ** 2).sum(), (abs(vb) ** 2).sum(), (np.conj(vc) * vb).real.sum()
        if chain is not None:
            out['total'][j] = (abs(vc + chain[i] * vb) ** 2).sum()
    return out


def _ldr(a):
    return np.asarray(a).astype(np.longdouble)


def gardner_chain_of_handle(op):
    'd b / d c = -(1 / rho) / (4 Re c) with the density of the handle, 80 bits: what k_ph3_coefficients<gardner> forms from op.rho'
    N = int(op.nrow)
    rho = _ldr(np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (N,)))
    cr = _ldr(np.broadcast_to(np.asarray(op.c).ravel().real, (N,)))
    return -(np.longdouble(1) / rho) / (np.longdouble(4) * cr)


def coefficient_reference(op, mode):
    '{plane: (reference, bound)} of k_ph3_coefficients in 80-bit arithmetic, each plane held to COEF_ULPS u of its own majorant'
    chain = gardner_chain_of_handle(op) if mode == 'gardner' else None
    ref = frechet3d.pseudoHessianCoefficients3(op, mode, chain, dtype=np.clongdouble)
    maj = frechet3d.pseudoHessianCoefficients3(op, mode, chain, dtype=np.clongdouble, magnitude=True)
    names = ('A0', 'h', 'S') + (('C', 'Smu') if mode == 'blocks' else ())
    return {n: (ref[n], COEF_ULPS[n] * U53 * maj[n]) for n in names}


def moments_terms(op, X, mode):
    """(value, majorant) of what k_ph3_moments adds per unit alpha W, in 80-bit arithmetic: S' E + D (N,), or for mode 'blocks' the rows H_cc, H_crho, H_rhorho
    (3, N) with the density factors; X (k, N) the columns as the kernel sums them (conjugated already where it conjugates).  The majorant is the same
    evaluation with every term by |Re| + |Im|."""
    uh = X.T
    if mode == 'blocks':
        return frechet3d.pseudoHessianBlocks3(op, uh, dtype=np.clongdouble), frechet3d.pseudoHessianBlocks3(op, uh, dtype=np.clongdouble, magnitude=True)
    chain = gardner_chain_of_handle(op) if mode == 'gardner' else None
    out = []
    for mag in (False, True):
        c = frechet3d.pseudoHessianCoefficients3(op, mode, chain, dtype=np.clongdouble, magnitude=mag)
        E, D, _ = frechet3d.pseudoHessianMoments3(op, uh, c['A0'], c['h'], np.clongdouble, mag)
        out.append(c['S'] * E + D)
    return tuple(out)


def moments_reference(terms, k, alpha, W, H0):
    """(H, bound) of k_ph3_moments fed the planes of k_ph3_coefficients: H = H0 + alpha W value, bound = moments_ulps(k) u (|H0| + alpha W majorant); terms those
    of moments_terms, W (N,) or None, H0 (N,) -- (3, N) for the blocks"""
    val, maj = terms
    w = np.longdouble(alpha) * (np.longdouble(1) if W is None else _ldr(W))
    H0 = _ldr(H0)
    return H0 + w * val, moments_ulps(k) * U53 * (np.abs(H0) + w * maj)


def worst(err, bound):
    'the largest error in units of its bound; where the bound is zero the error must be'
    err, bound = np.asarray(err), np.asarray(bound)
    ok = bound > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
