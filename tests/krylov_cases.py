"""Shared by tests/test_krylov_reference_host.py (CPU) and tests/test_gpu_krylov.py (GPU): the cases (grid, model, right-hand sides) on which the Krylov
drivers of zephyr_amd/csrc/krylov.hip are held to their recurrences, and plain-numpy restatements of those recurrences.  Nothing here touches a GPU.

With `method = bicgstab | cgnr` and `maxit = k` the drivers perform exactly k iterations and hand back the iterate (status 1, the true relative residual): a
deterministic function of the coefficient planes and the right-hand side.  The references below compute the same iterate

    exact    everything in numpy.clongdouble (x87: 64-bit significand)
    double   the same statements in complex128: every stored vector, scaled plane and scalar rounded to double, sums in numpy's order

and d_k = ||x_k^double - x_k^exact|| / ||x_k^exact|| measures what one realisation of double rounding does to the k-th iterate.  The device is another
realisation of the same size (wave butterfly, one partial per workgroup, a fixed-order k_fin, contracted multiply-adds); the recurrence amplifies both alike,
so the device iterate is asked to lie within MARGIN max(d_k, 64 u) of x_k^exact, MARGIN = 16.

Orders, as the drivers have them:

    run_bicgstab   x = 0, r = r0 = bbar = D^-1 (premul q), rho = (bbar, bbar);  p = r + beta (p - omega v) [beta = 0 first];  v = Abar p;  sigma = (r0, v);
                   alpha = rho / sigma;  s = r - alpha v;  t = Abar s;  omega = (t, s) / (t, t);  x += alpha p + omega s;  r = s - omega t;  rho' = (r0, r);
                   beta = (rho' / rho)(alpha / omega).  (a, b) = sum conj(a) b.
    run_cgnr       x = 0, r = bbar [FIN_CG_RR counts ONE iteration here];  z = Abar^H r;  gamma = (z, z);  p = z;  then per step  w = Abar p;
                   alpha = gamma / (w, w);  x += alpha p;  r -= alpha w [count + 1];  z = Abar^H r;  gamma' = (z, z);  beta = gamma' / gamma;  p = z + beta p.
                   Hence after j steps the driver reports j + 1 iterations, and `maxit = j + 1` returns the iterate of j steps (maxit = 1: x = 0).
                   On the Jacobi-scaled block Abar = D^-1 A, bbar = D^-1 q'; on the coupled system Abar = diag(rs) [[M1, M2], [M3, M4]], rs = 1 / ||row||_2 over
                   both blocks of a row, bbar = rs q', vectors of 2N.

Stencil sweeps are by slicing, as oracle.helm_oracle.stencil_apply does: entries that point outside the grid are dropped."""
import functools

import numpy as np

CLD, LD = np.clongdouble, np.longdouble
U = 2.0 ** -53
MARGIN = 16.0
KS = (1, 2, 3, 5, 8)
NCOLS = (1, 5, 17)
PREMULS = (1.0 + 0j, 0.3 - 1.7j)
HELM_BICGSTAB, HELM_CGNR, HELM_AUTO, HELM_MG = 0, 1, 2, 3


def have_x87():
    return np.finfo(np.longdouble).nmant >= 63


def cgnr_reported(steps):
    "what helm_solve_info.iterations holds after `steps` CGNR steps: the residual evaluation that starts run_cgnr (FIN_CG_RR) already counts one"
    return steps + 1


def floor_tol(d):
    "the bound of an iterate whose double reference sits d from the exact one"
    return MARGIN * max(float(d), 64 * U)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
#   kind: 'mz' MiniZephyr, 'eu' Eurus block 0 (eps == delta, N-row right-hand side), 'tti' the coupled Eurus system (2N-row right-hand side), '3d' Helm3D
CASES = {
    'S':    dict(kind='mz', dims=(12, 70), h=(10., 10.), nPML=4, freq=20., seed=11),
    'M':    dict(kind='mz', dims=(41, 150), h=(8., 10.), nPML=4, freq=20., tau=0.4, freeSurf=(True, False, False, False), seed=12),
    'L':    dict(kind='mz', dims=(450, 600), h=(10., 10.), nPML=10, freq=20., seed=13, ks=(1, 2), ncols=(1, 2)),
    'E0':   dict(kind='eu', dims=(41, 150), h=(10., 10.), nPML=4, freq=20., seed=14),
    'TTI':  dict(kind='tti', dims=(44, 52), h=(10., 10.), nPML=4, freq=10., tau=0.02, seed=15),
    '3S':   dict(kind='3d', dims=(10, 9, 70), h=(8., 12., 10.), nPML=4, freq=12., tau=0.5, seed=16),
    '3L':   dict(kind='3d', dims=(64, 64, 65), h=(10., 10., 10.), nPML=10, freq=8., seed=17, ks=(1, 2), ncols=(1,)),
    # the refinement round (restart_columns below): at 40 Hz the mass term nearly cancels the Laplacian on the diagonal of the slowest cells (k h ~ 1.4 along x,
    # dz = 6: |centre| from 1.5e-6 to a median of 2.4e-5), so that rows weigh very differently in the scaled and in the unscaled residual
    'R':    dict(kind='mz', dims=(12, 70), h=(6., 10.), nPML=4, freq=40., tau=0.4, freeSurf=(True, False, False, False), seed=12),
}
# h = (dz, dx) or (dz, dy, dx)
ITERATE_CASES = ('S', 'M', 'L', 'E0', 'TTI', '3S', '3L')          # those of the iterate tests; 'R' serves the restart path alone


def case_ks(name):
    return CASES[name].get('ks', KS)


def case_ncols(name):
    return CASES[name].get('ncols', NCOLS)


def case_methods(name):
    "the Krylov methods the driver serves for this case (3-D has no adjoint apply, the coupled system is CGNR only)"
    return {'mz': ('bicgstab', 'cgnr'), 'eu': ('bicgstab', 'cgnr'), 'tti': ('cgnr',), '3d': ('bicgstab',)}[CASES[name]['kind']]


def rows_of(name):
    n = int(np.prod(CASES[name]['dims']))
    return 2 * n if CASES[name]['kind'] == 'tti' else n


@functools.lru_cache(maxsize=None)
def model(name):
    "c = (1800 + 2200 rand)(1 + 0.01j), rho = 1000 + 600 rand; the coupled case adds theta, eps != delta"
    cs = CASES[name]
    rng = np.random.default_rng(cs['seed'])
    dims = cs['dims']
    m = dict(c=(1800. + 2200. * rng.random(dims)) * (1 + 0.01j), rho=1000. + 600. * rng.random(dims))
    if cs['kind'] == 'tti':
        m.update(theta=0.6 * rng.random(dims), eps=0.2 + 0.1 * rng.random(dims), delta=0.05 + 0.1 * rng.random(dims))
    elif cs['kind'] == 'eu':
        e = 0.1 + 0.1 * rng.random(dims)
        m.update(theta=0.6 * rng.random(dims), eps=e, delta=e.copy())
    return m


def config(name, **kw):
    "systemConfig of the zephyr_amd class of this case (MiniZephyr, Eurus, Helm3D)"
    cs, m = CASES[name], model(name)
    dims, h = cs['dims'], cs['h']
    cfg = dict(nz=dims[0], nx=dims[-1], dz=h[0], dx=h[-1], freq=cs['freq'], nPML=cs['nPML'], c=m['c'], rho=m['rho'])
    if len(dims) == 3:
        cfg.update(ny=dims[1], dy=h[1])
    for key in ('tau', 'freeSurf'):
        if key in cs:
            cfg[key] = cs[key]
    for key in ('theta', 'eps', 'delta'):
        if key in m:
            cfg[key] = m[key]
    cfg.update(kw)
    return cfg


def oracle_planes(name):
    "the planes of the case from the CPU oracle: (9, nz, nx), (4, 9, nz, nx) for the Eurus kinds, (27, nz, ny, nx)"
    from oracle import helm_oracle as ho
    from oracle import helm3d_oracle as h3
    cs, m = CASES[name], model(name)
    dims, h = cs['dims'], cs['h']
    tau = cs.get('tau', np.inf)
    if cs['kind'] == 'mz':
        return ho.minizephyr_coefficients(dims[0], dims[1], m['c'], m['rho'], cs['freq'], dx=h[1], dz=h[0], tau=tau, nPML=cs['nPML'],
                                          freeSurf=cs.get('freeSurf', (False,) * 4))
    if cs['kind'] in ('eu', 'tti'):
        return ho.eurus_coefficients(dims[0], dims[1], m['c'], m['rho'], cs['freq'], dx=h[1], dz=h[0], tau=tau, nPML=cs['nPML'],
                                     theta=m['theta'], eps=m['eps'], delta=m['delta'])
    return h3.helm3d_coefficients(dims[0], dims[1], dims[2], m['c'], m['rho'], cs['freq'], dx=h[2], dy=h[1], dz=h[0], tau=tau, nPML=cs['nPML'])


def system_planes(name, C):
    "what the references take: the planes of the one block that is iterated ((P, *dims)), or for the coupled system all four ((4, 9, nz, nx))"
    kind = CASES[name]['kind']
    if kind == 'eu':
        return C[0] if C.ndim == 4 else C
    return C


def rhs_columns(name, ncol):
    """(ncol, rows) complex128: complex normal fields, with one point source next to an absorbing layer (column 1) and one all-zero column (column 2) where there
    is room for them; returns (Q, kinds), kinds[j] in 'normal', 'point', 'zero'"""
    cs = CASES[name]
    dims = cs['dims']
    rows = rows_of(name)
    rng = np.random.default_rng(1000 + cs['seed'])
    Q = rng.standard_normal((17, rows)) + 1j * rng.standard_normal((17, rows))
    Q = Q[:ncol].copy()
    kinds = ['normal'] * ncol
    if ncol >= 3:
        at = tuple(min(cs['nPML'] + 1, d - 2) for d in dims)              # the first cell inside the layers, in every direction
        Q[1] = 0
        Q[1, int(np.ravel_multi_index(at, dims))] = 2.0 - 1.5j
        if rows == 2 * int(np.prod(dims)):
            Q[1, int(np.prod(dims)) + int(np.ravel_multi_index(at, dims))] = -0.5 + 1.0j
        Q[2] = 0
        kinds[1], kinds[2] = 'point', 'zero'
    return Q, kinds


# ---- sweeps ------------------------------------------------------------------------------------------------------------------------------------
def _offsets(ndim):
    r = (-1, 0, 1)
    return [(a, b) for a in r for b in r] if ndim == 2 else [(a, b, c) for a in r for b in r for c in r]


def sweep(C, X, adjoint=False):
    """Y = A X (adjoint: A^H X) for one block.  C: (P, *dims); X: (ncol, *dims) of C's dtype.  (A x)[i] = sum_k C[k][i] x[i + off_k], cells outside dropped."""
    dims = C.shape[1:]
    Y = np.zeros_like(X)
    for k, off in enumerate(_offsets(len(dims))):
        here = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, dims))
        there = tuple(slice(max(0, -o) + o, n - max(0, o) + o) for o, n in zip(off, dims))
        if adjoint:
            Y[(slice(None),) + there] += np.conj(C[k][here]) * X[(slice(None),) + here]
        else:
            Y[(slice(None),) + here] += C[k][here] * X[(slice(None),) + there]
    return Y


def sweep_sys2(C4, X, adjoint=False):
    "the coupled system [[M1, M2], [M3, M4]] on (ncol, 2, nz, nx): launch_sys2_apply"
    Y = np.empty_like(X)
    for half in range(2):
        a, b = ((0 * 2 + half), (1 * 2 + half)) if adjoint else ((half * 2 + 0), (half * 2 + 1))
        Y[:, half] = sweep(C4[a], X[:, 0], adjoint) + sweep(C4[b], X[:, 1], adjoint)
    return Y


def dot(a, b):
    "(a, b) = sum conj(a) b per column"
    n = a.shape[0]
    return (np.conj(a) * b).reshape(n, -1).sum(axis=1)


def _col(s, X):
    return s.reshape((-1,) + (1,) * (X.ndim - 1))


class System(object):
    """the scaled system the driver iterates on, in one precision: Abar, bbar = scale (premul q) and the raw operator for true residuals.
    planes: what system_planes returned (complex128, upcast exactly); dtype: CLD ('exact') or complex128 ('double')"""

    def __init__(self, name, planes, dtype):
        kind = CASES[name]['kind']
        self.dtype, self.sys2 = dtype, kind == 'tti'
        self.dims = CASES[name]['dims']
        self.raw = np.asarray(planes).astype(dtype)
        rdt = LD if dtype == CLD else np.float64
        if self.sys2:
            a2 = (self.raw.real.astype(rdt) ** 2 + self.raw.imag.astype(rdt) ** 2)               # (4, 9, nz, nx)
            n2 = np.stack([a2[0].sum(axis=0) + a2[1].sum(axis=0), a2[2].sum(axis=0) + a2[3].sum(axis=0)])      # (2, nz, nx)
            self.scale = (1 / np.sqrt(n2)).astype(rdt)                               # rs
            self.Abar = (self.raw.reshape((2, 2) + self.raw.shape[1:]) * self.scale[:, None, None]).reshape(self.raw.shape).astype(dtype)
            self.vshape = (2,) + tuple(self.dims)
        else:
            centre = self.raw.shape[0] // 2
            self.scale = (1 / self.raw[centre]).astype(dtype)                        # dinv
            self.Abar = (self.raw / self.raw[centre][None]).astype(dtype)
            self.Abar[centre] = 1
            self.vshape = tuple(self.dims)

    def apply(self, X, adjoint=False, raw=False):
        P = self.raw if raw else self.Abar
        return sweep_sys2(P, X, adjoint) if self.sys2 else sweep(P, X, adjoint)

    def qprime(self, Q, premul):
        return (self.dtype(premul) * np.asarray(Q).astype(self.dtype)).astype(self.dtype).reshape((-1,) + self.vshape)

    def bbar(self, Q, premul):
        return (self.scale[None] * self.qprime(Q, premul)).astype(self.dtype)


BICG_MUTANTS = ('omega_st', 'beta_no_ratio', 'p_no_omega_v', 'r0_refreshed')
CGNR_MUTANTS = ('beta_inverted', 'z_forward')


def bicgstab_iterates(S, Q, premul, kmax, mutant=None, rtol=None):
    """x_1 .. x_kmax of run_bicgstab for the non-zero columns Q (ncol, rows): list of (ncol, rows) arrays.  rtol given: go on until every column has
    ||r|| <= rtol ||bbar|| (at most kmax) and return (x, iterations) instead."""
    b = S.bbar(Q, premul)
    x, r, r0 = np.zeros_like(b), b.copy(), b.copy()
    p, v = np.zeros_like(b), np.zeros_like(b)
    rho = dot(b, b)
    bb = rho.real.copy()
    one = np.ones(b.shape[0], dtype=S.dtype)
    alpha, omega, beta = one.copy(), one.copy(), 0 * one
    out = []
    for k in range(1, kmax + 1):
        if mutant == 'r0_refreshed':
            r0 = r.copy()
            rho = dot(r0, r)
        p = r + _col(beta, p) * (p - (0 if mutant == 'p_no_omega_v' else _col(omega, v) * v))
        v = S.apply(p)
        alpha = rho / dot(r0, v)
        s = r - _col(alpha, v) * v
        t = S.apply(s)
        omega = (dot(s, t) if mutant == 'omega_st' else dot(t, s)) / dot(t, t).real
        x = x + _col(alpha, p) * p + _col(omega, s) * s
        r = s - _col(omega, t) * t
        rhon = dot(r0, r)
        beta = (rhon / rho) * (1 if mutant == 'beta_no_ratio' else alpha / omega)
        rho = rhon
        if rtol is None:
            out.append(x.reshape(x.shape[0], -1).copy())
        elif np.all(dot(r, r).real <= (rtol * rtol) * bb):
            return x.reshape(x.shape[0], -1), k
    return out if rtol is None else (x.reshape(x.shape[0], -1), kmax)


def cgnr_iterates(S, Q, premul, kmax, mutant=None, rtol=None):
    "x after 1 .. kmax CGNR steps of run_cgnr (the driver reports cgnr_reported(steps) iterations); rtol as in bicgstab_iterates"
    b = S.bbar(Q, premul)
    x, r = np.zeros_like(b), b.copy()
    bb = dot(b, b).real
    z = S.apply(r, adjoint=(mutant != 'z_forward'))
    gamma = dot(z, z).real
    p = z.copy()
    out = []
    for k in range(1, kmax + 1):
        w = S.apply(p)
        alpha = gamma / dot(w, w).real
        x = x + _col(alpha, p) * p
        r = r - _col(alpha, w) * w
        z = S.apply(r, adjoint=(mutant != 'z_forward'))
        gn = dot(z, z).real
        beta = gamma / gn if mutant == 'beta_inverted' else gn / gamma
        gamma = gn
        p = z + _col(beta, p) * p
        if rtol is None:
            out.append(x.reshape(x.shape[0], -1).copy())
        elif np.all(dot(r, r).real <= (rtol * rtol) * bb):
            return x.reshape(x.shape[0], -1), k
    return out if rtol is None else (x.reshape(x.shape[0], -1), kmax)


ITERATES = {'bicgstab': bicgstab_iterates, 'cgnr': cgnr_iterates}
MUTANTS = {'bicgstab': BICG_MUTANTS, 'cgnr': CGNR_MUTANTS}


def relnorm(a, b):
    "||a - b|| / ||b|| per column, in extended precision"
    a, b = np.asarray(a).astype(CLD), np.asarray(b).astype(CLD)
    num = np.sqrt((np.abs(a - b) ** 2).sum(axis=1))
    den = np.sqrt((np.abs(b) ** 2).sum(axis=1))
    return (num / den).astype(np.float64)


def sensitivity(name, planes, Q, premul, method, kmax):
    "(exact iterates, d): d[k - 1][col] = ||x_k^double - x_k^exact|| / ||x_k^exact|| for the non-zero columns Q"
    ex = ITERATES[method](System(name, planes, CLD), Q, premul, kmax)
    db = ITERATES[method](System(name, planes, np.complex128), Q, premul, kmax)
    return ex, np.array([relnorm(b, e) for b, e in zip(db, ex)])


# ---- the refinement round ------------------------------------------------------------------------------------------------------------------------------
RESTART_RTOL = 1e-3


def restart_columns(C):
    """five columns on case 'R' (C: its nine planes): 0, 4 complex normal fields, 1 a point source in the middle of the grid, 2 zeros, 3 a point source on the
    interior cell whose diagonal entry is the smallest"""
    dims = CASES['R']['dims']
    Q, kinds = rhs_columns('R', 5)
    Q[1] = 0
    Q[1, (dims[0] // 2) * dims[1] + dims[1] // 2] = 2.0 - 1.5j
    D = np.abs(np.asarray(C)[4]).astype(np.float64).copy()
    D[0], D[-1], D[:, 0], D[:, -1] = np.inf, np.inf, np.inf, np.inf
    Q[3] = 0
    Q[3, int(np.argmin(D))] = 1.0 + 1.0j
    kinds[3] = 'point'
    return Q, kinds


def refinement_ratio(name, C, q, rtol):
    """what solve_block_krylov looks at after its first round, from the double reference: BiCGSTAB until ||r|| <= rtol / 2 ||bbar|| on the scaled system, then
    ||q - A x|| / ||q|| of the unscaled one over rtol.  Above 1 the column takes the refinement round.  Returns (ratio, iterations)."""
    x, its = bicgstab_iterates(System(name, C, np.complex128), q[None], 1.0, 20000, rtol=0.5 * rtol)
    rr, _ = relres_reference(name, C, q[None], 1.0, x)
    return float(rr[0] / rtol), its


# ---- the true relative residual the driver reports ---------------------------------------------------------------------------------------------------
def relres_reference(name, planes, Q, premul, X):
    """||q' - A x|| / ||q'|| per column in extended precision, q' = premul q, and the bound on what the device's figure may differ from it by.

    The device forms every component of r = q' - A x as a real sum of 2 P + 1 terms (P planes per row: 9, 27, or 18 on the coupled system), every product rounded
    at most twice, q' = premul q itself a rounded complex product: |r - r_ref| <= (2 P + 10) u S, S = |q'| + sum |c_k| |x_k| in moduli, whatever the order.  The
    sums of n squares behind rr and qq carry a relative error of at most (2 n + 8) u each (order-independent), so sqrt(rr / qq) with its division and root lies
    within  (2 P + 10) u ||S|| / ||q'||  +  (2 n + 12) u relres  of the reference."""
    S = System(name, planes, CLD)
    q = S.qprime(Q, premul)
    x = np.asarray(X).astype(CLD).reshape(q.shape)
    r = q - S.apply(x, raw=True)
    mod = System.__new__(System)
    mod.__dict__.update(S.__dict__)
    mod.raw = np.abs(S.raw).astype(CLD)
    Smod = np.abs(q) + mod.apply(np.abs(x).astype(CLD), raw=True).real
    nrm = lambda a: np.sqrt((np.abs(a.reshape(a.shape[0], -1)) ** 2).sum(axis=1))
    qn = nrm(q)
    relres = nrm(r) / qn
    P = 18 if S.sys2 else S.raw.shape[0]
    n = int(np.prod(q.shape[1:]))
    bound = (2 * P + 10) * U * nrm(Smod) / qn + (2 * n + 12) * U * relres
    return relres.astype(np.float64), bound.astype(np.float64)
