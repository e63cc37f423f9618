"""Host maps of the exact velocity and buoyancy derivatives of the 3-D 27-point operator (numpy / scipy): what `Helm3DProblem` runs when the device routes do not serve
(hostGradient, host lists of fields, no GPU), and the reference the device kernels of csrc/survey3d.hip are tested against.

With an explicit density the derivative of `Helm3D.A` along the velocity is its mass term alone (oracle/helm3d_oracle.py: the C-PML profiles do not depend on
the model, bbar on rho only):

    dA[dc] = M~ diag(dK),   dK_j = chi_j dc_j,   chi = -2 K / c,   K = om~^2 / (rho c^2),   om~ = 2 pi f - i / tau

M~ the constant 27-point stencil mu_o = a [o == 0] + (1 - a) m(ox) m(oy) m(oz) (a = 1/2, m(0) = 2/3, m(+-1) = 1/6) with the rows on the box boundary zeroed:
those are identity rows and do not move.  An interior row never reads outside the grid; a boundary NODE is a column of interior rows, so dc there counts.

Everything here reads nothing of an operator but `c`, `rho`, `freq`, `tau` and its grid (`modelDims`): any object with those serves, whatever its `* q` does.
"""
import numpy as np
import scipy.sparse as sp

MASS_BLEND = 0.5


def _m(o):
    return 2.0 / 3.0 if o == 0 else 1.0 / 6.0


def massWeight3(oz, oy, ox):
    'mu_o of the 27-point mass stencil'
    return (MASS_BLEND if (oz, oy, ox) == (0, 0, 0) else 0.0) + (1.0 - MASS_BLEND) * _m(ox) * _m(oy) * _m(oz)


def interiorMask3(dims):
    '(N,) bool: True on the cells that are not on the boundary of the (nz, ny, nx) box -- the rows of A that are not identity rows'
    nz, ny, nx = (int(d) for d in dims)
    m = np.zeros((nz, ny, nx), dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m.ravel()


def massStencil3(dims):
    'M~ as CSR (N, N), float64: row p = mu_o at the columns p + o for an interior p, an empty row for a boundary p'
    nz, ny, nx = (int(d) for d in dims)
    N = nz * ny * nx
    iz, iy, ix = (a[1:-1, 1:-1, 1:-1].ravel() for a in np.mgrid[0:nz, 0:ny, 0:nx])
    row = (iz * ny + iy) * nx + ix
    rows, cols, vals = [], [], []
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                rows.append(row)
                cols.append(((iz + oz) * ny + (iy + oy)) * nx + (ix + ox))
                vals.append(np.full(row.size, massWeight3(oz, oy, ox)))
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()


def dampedOmega3(op):
    'om~ = 2 pi f - i / tau of an operator (f may be complex; no `tau`: no damping)'
    return 2.0 * np.pi * complex(op.freq) - 1j / float(getattr(op, 'tau', np.inf))


def massField3(op):
    'K = om~^2 / (rho c^2) per cell, (N,) complex128'
    N = int(np.prod(op.modelDims))
    c = np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel(), (N,))
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (N,))
    om = dampedOmega3(op)
    return om * om / (rho * c * c)


def velocityChain3(op):
    'chi = d K / d c = -2 K / c per cell, (N,) complex128'
    N = int(np.prod(op.modelDims))
    c = np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel(), (N,))
    return -2.0 * massField3(op) / c


def bornSources3(op, dc, uh, M=None):
    """(dA[dc]) u^_s = M~(chi dc (.) u^_s) for the columns of uh (N, nsrc) -- the unconjugated, unscaled forward solves u^ = A^-1 premul q; dc (N,) real.
    M: massStencil3(op.modelDims) if the caller keeps one."""
    M = massStencil3(op.modelDims) if M is None else M
    w = velocityChain3(op) * np.asarray(dc, dtype=np.float64).ravel()
    return M @ (w[:, None] * np.asarray(uh))


def imagingSum3(op, uh, lam, M=None):
    'P_j = sum_s u^_{s,j} (M~^T lam_s)_j, (N,) complex128: uh, lam (N, nsrc); the boundary rows of lam drop out through the empty rows of M~'
    M = massStencil3(op.modelDims) if M is None else M
    return (np.asarray(uh) * (M.T @ np.asarray(lam))).sum(axis=1)


# ---- the derivative along the buoyancy b = 1 / rho ------------------------------------------------------------------------------------------------------
# An interior row of the operator is C_o(p) = (b_p + b_{p+o}) / 2 lap_o(p) + b_{p+o} kappa_{p+o} mu_o, kappa = om~^2 / c^2,
#     lap_o(p) = Lx[ox](ix) m(oy) m(oz) / dx^2 + m(ox) Ly[oy](iy) m(oz) / dy^2 + m(ox) m(oy) Lz[oz](iz) / dz^2,
# the stretch tables read at the ROW p: linear and homogeneous in b, so with L the matrix of lap_o(p) on interior rows (boundary rows empty)
#     dA[db] = 1/2 diag(db) L + 1/2 L diag(db) + M~ diag(kappa db).
# L is not symmetric (the stretch factors sit at the row): the adjoint needs L^T.
GARDNER_FACTOR, GARDNER_POWER = 310., 0.25


def stretchTables3(op):
    """((Lx(-1), Lx(0), Lx(+1)), (Ly...), (Lz...)): the Laplacian factors of the C-PML per axis, complex128 arrays of nx, ny, nz entries -- the tables the
    assembly reads (gamma = cPML cos(pi/2 dist / L) over nPML nodes at each end, xi = 1 - i gamma / om~, L(+-1) = 1 / (xi_i (xi_i + xi_{i+-1}) / 2))"""
    nz, ny, nx = (int(d) for d in op.modelDims)
    om = dampedOmega3(op)
    npml, cpml = int(getattr(op, 'nPML', 10)), float(getattr(op, 'cPML', 300.))

    def axis(n, h):
        g = np.zeros(n)
        k = np.arange(npml)
        ell = h * (npml - 1)
        g[:npml] = cpml * np.cos((np.pi / 2) * (k * h / ell))
        g[n - npml:] = cpml * np.cos((np.pi / 2) * ((npml - 1 - k) * h / ell))
        xi = 1 - (1j * np.pad(g, 1, mode='edge')) / om
        c = xi[1:-1]
        lm, lp = 1.0 / (c * (c + xi[:-2]) / 2), 1.0 / (c * (c + xi[2:]) / 2)
        return lm, -(lm + lp), lp
    return axis(nx, float(op.dx)), axis(ny, float(getattr(op, 'dy', op.dx))), axis(nz, float(op.dz))


def lapStencil3(op):
    'L as CSR (N, N), complex128: row p = lap_o(p) at the columns p + o for an interior p, an empty row for a boundary p'
    nz, ny, nx = (int(d) for d in op.modelDims)
    N = nz * ny * nx
    Lx, Ly, Lz = stretchTables3(op)
    dx, dy, dz = float(op.dx), float(getattr(op, 'dy', op.dx)), float(op.dz)
    iz, iy, ix = (a[1:-1, 1:-1, 1:-1].ravel() for a in np.mgrid[0:nz, 0:ny, 0:nx])
    row = (iz * ny + iy) * nx + ix
    rows, cols, vals = [], [], []
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                rows.append(row)
                cols.append(((iz + oz) * ny + (iy + oy)) * nx + (ix + ox))
                vals.append(Lx[ox + 1][ix] * (_m(oy) * _m(oz) / dx ** 2) + Ly[oy + 1][iy] * (_m(ox) * _m(oz) / dy ** 2) + Lz[oz + 1][iz] * (_m(ox) * _m(oy) / dz ** 2))
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()


def kappa3(op):
    'kappa = om~^2 / c^2 per cell, (N,) complex128: K = b kappa'
    N = int(np.prod(op.modelDims))
    c = np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel(), (N,))
    om = dampedOmega3(op)
    return om * om / (c * c)


def buoyancySources3(op, db, uh, L=None, M=None):
    """(dA[db]) u^_s = 1/2 db (.) (L u^_s) + 1/2 L(db (.) u^_s) + M~(kappa db (.) u^_s) for the columns of uh (N, nsrc); db (N,) real.  The boundary rows are
    exact zeros.  L, M: lapStencil3(op), massStencil3(op.modelDims) if the caller keeps them."""
    L = lapStencil3(op) if L is None else L
    M = massStencil3(op.modelDims) if M is None else M
    db = np.asarray(db, dtype=np.float64).ravel()[:, None]
    uh = np.asarray(uh)
    return 0.5 * db * (L @ uh) + 0.5 * (L @ (db * uh)) + M @ ((kappa3(op)[:, None] * db) * uh)


def buoyancyImaging3(op, uh, lam, L=None, M=None, LT=None):
    """(N,) complex128: sum_s [ 1/2 lam0_s (.) (L u^_s) + 1/2 u^_s (.) (L^T lam0_s) + kappa (.) u^_s (.) (M~^T lam0_s) ], the transpose of buoyancySources3 in db
    contracted with lam; lam0 = lam with its boundary rows masked (they drop out through the empty rows of L and M~: every cell receives a value, boundary
    nodes included).  LT: what stands in the place of L^T (tests put L there to show that it is not the transpose)."""
    L = lapStencil3(op) if L is None else L
    M = massStencil3(op.modelDims) if M is None else M
    LT = sp.csr_matrix(L.T) if LT is None else LT
    uh = np.asarray(uh)
    lam0 = np.asarray(lam) * interiorMask3(op.modelDims)[:, None]
    return (0.5 * lam0 * (L @ uh) + 0.5 * uh * (LT @ lam0) + kappa3(op)[:, None] * uh * (M.T @ lam0)).sum(axis=1)


def densityChain3(op):
    'd b / d rho = -1 / rho^2 per cell, (N,) float64'
    N = int(np.prod(op.modelDims))
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (N,))
    return -1.0 / (rho * rho)


def gardnerChain3(op):
    'd b / d c = -b / (4 Re c) per cell of the default density rho = 310 Re(c)^0.25 (b = Re(c)^-0.25 / 310), (N,) float64'
    N = int(np.prod(op.modelDims))
    cr = np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel(), (N,)).real
    return -(cr ** -GARDNER_POWER / GARDNER_FACTOR) / (4.0 * cr)


# ---- the pseudo-Hessian diagonal and the (c, rho) blocks ------------------------------------------------------------------------------------------------
# H_p[i] = sum_s ||(dA / dp_i) u^_s||^2.  The column of a unit perturbation of cell i touches the 27 rows p = i + d around it:
#     velocity (explicit rho):  v^c_p = chi_i mu_d [p interior] u^_i                                        (mu is even: mu_{i-p} = mu_d)
#     buoyancy:                 v^b_p = a_p(i) u^_i + [p == i] 1/2 (L u^)_i,   a_p(i) = [p interior] (1/2 lap_{-d}(i + d) + kappa_i mu_d)
# lap_{-d}(i + d) reads the stretch tables at the NEIGHBOUR's row: the entry L[p, i] of the column, not L[i, p] of the row.  Per cell and column only u^_i and
# T_i = (L u^)_i are needed; with r_s = A0_i u^_{s,i} + h_i T_{s,i} and the moments E = sum_s |u^_i|^2, D = sum_s |r_s|^2, Y = sum_s conj(u^_i) r_s
#     H_bb = S' E + D,   H_cc = |chi|^2 Smu E,   H_cb = Re conj(chi) (C' E + mu_0 [i interior] Y)
# S' = sum_{p != i} |a_p(i)|^2, C' = sum_{p != i} mu_d a_p(i), Smu = sum_{p interior} mu_d^2, A0 = a_i(i), h = 1/2.  The Gardner total derivative is the column
# v^c + g v^b, g = d b / d c: A0 = chi mu_0 [i interior] + g a_i(i), h = g / 2, S' = sum_{p != i} |chi mu_d [p interior] + g a_p(i)|^2, H = S' E + D.
# D is never expanded: |a|^2 E + Re(conj(a) X) + 1/4 sum |T|^2 cancels wherever L u^ ~ -kappa u^, which is everywhere away from a source.
OFFSETS27 = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _realType(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def _mag(a):
    '|Re a| + |Im a|: what stands for a complex number when every term is taken by its modulus (it majorises both |a| and the componentwise products)'
    a = np.asarray(a)
    return np.abs(a.real) + np.abs(a.imag) if np.iscomplexobj(a) else np.abs(a)


def _shift3(T, o):
    'T[p + o] on a (nz, ny, nx, ...) array, zero (False) where p + o lies outside the grid'
    nz, ny, nx = T.shape[:3]
    Tp = np.zeros((nz + 2, ny + 2, nx + 2) + T.shape[3:], dtype=T.dtype)
    Tp[1:-1, 1:-1, 1:-1] = T
    oz, oy, ox = o
    return Tp[1 + oz:1 + oz + nz, 1 + oy:1 + oy + ny, 1 + ox:1 + ox + nx]


def _lapGeometry3(op, dtype, magnitude):
    """(lap, m, rt): lap(d, at) the (nz, ny, nx) array of lap_d read at the row i (at == 0) or of lap_{-d} read at the row i + d (at == 1: the column entry
    L[i + d, i], zero where i + d lies outside the grid), from the fp64 tables of stretchTables3 widened exactly, the constants m and 1 / h^2 in the real type
    of `dtype`; magnitude: every table value by |Re| + |Im|"""
    rt = _realType(dtype)
    nz, ny, nx = (int(d) for d in op.modelDims)
    tabs = [tuple(np.asarray(t).astype(dtype) for t in axis) for axis in stretchTables3(op)]
    if magnitude:
        tabs = [tuple(_mag(t) for t in axis) for axis in tabs]
    third, sixth = rt(2) / rt(3), rt(1) / rt(6)
    m = lambda o: third if o == 0 else sixth
    ih2 = [rt(1) / (rt(float(h)) * rt(float(h))) for h in (op.dx, getattr(op, 'dy', op.dx), op.dz)]

    def table(axis, o, at):
        if not at:
            return tabs[axis][o + 1]
        t = tabs[axis][1 - o]                       # L[-o] at the neighbour i + o
        out = np.zeros_like(t)
        if o == 0:
            out[:] = t
        elif o > 0:
            out[:-1] = t[1:]
        else:
            out[1:] = t[:-1]
        return out

    def lap(d, at):
        dz, dy, dx = d
        tx, ty, tz = table(0, dx, at)[None, None, :], table(1, dy, at)[None, :, None], table(2, dz, at)[:, None, None]
        return np.broadcast_to(tx * (m(dy) * m(dz) * ih2[0]) + ty * (m(dx) * m(dz) * ih2[1]) + tz * (m(dx) * m(dy) * ih2[2]), (nz, ny, nx))
    return lap, m, rt


def pseudoHessianCoefficients3(op, mode, chain=None, dtype=np.complex128, magnitude=False, tables='transposed', rows='all', mask=True):
    """The per-cell coefficients of the pseudo-Hessian, each (N,): {'A0' (complex), 'h', 'S' (S'), and for mode 'blocks' 'C' (C', complex), 'Smu', 'chi' (complex),
    'rho'}.  mode 'buoyancy' (the derivative along b), 'gardner' (the total velocity derivative, chain = d b / d c per cell, default gardnerChain3(op)) or
    'blocks' (the buoyancy coefficients and what the velocity and cross entries need).  dtype complex128 or clongdouble (the model and the fp64 stretch tables
    widened exactly).  magnitude: every term by |Re| + |Im|, all outputs real and non-negative -- the majorants of the rounding bounds.
    tables='row', rows='centre', mask=False: what the tests put in the place of the column of L, of the 27 rows and of the interior mask of the neighbour
    rows to show that each matters."""
    if mode not in ('buoyancy', 'gardner', 'blocks'):
        raise ValueError('mode is %r: \'buoyancy\', \'gardner\' or \'blocks\'' % (mode,))
    dims = tuple(int(d) for d in op.modelDims)
    N = int(np.prod(dims))
    lap, m, rt = _lapGeometry3(op, dtype, magnitude)
    c = np.broadcast_to(np.asarray(op.c).ravel(), (N,)).astype(dtype).reshape(dims)
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (N,)).astype(rt).reshape(dims)
    om = np.dtype(dtype).type(dampedOmega3(op))
    kap = om * om / (c * c)
    b = rt(1) / rho
    chi = rt(-2) * kap * b / c
    if mode == 'gardner':
        g = (gardnerChain3(op) if chain is None else np.broadcast_to(np.asarray(chain).ravel(), (N,))).astype(rt).reshape(dims)
    if magnitude:
        kap, chi = _mag(kap), _mag(chi)
        g = np.abs(g) if mode == 'gardner' else None
    inside = interiorMask3(dims).reshape(dims)
    ingrid = np.ones(dims, dtype=bool)
    half, mu0 = rt(1) / rt(2), None
    A0 = np.zeros(dims, dtype=kap.dtype)
    S, Smu, C = np.zeros(dims, dtype=rt), np.zeros(dims, dtype=rt), np.zeros(dims, dtype=kap.dtype)
    for d in OFFSETS27:
        mu = half * m(d[0]) * m(d[1]) * m(d[2]) + (half if d == (0, 0, 0) else rt(0))
        pin = _shift3(inside if mask else ingrid, d)
        a = np.where(pin, half * lap(d, 0 if tables == 'row' else 1) + kap * mu, 0)
        q = np.where(pin, chi * mu, 0) + g * a if mode == 'gardner' else a
        if d == (0, 0, 0):
            A0, mu0 = q, mu
            Smu = Smu + np.where(pin, mu * mu, 0)
        elif rows == 'all':
            S = S + (q * q if magnitude else q.real * q.real + q.imag * q.imag)
            C = C + mu * a
            Smu = Smu + np.where(pin, mu * mu, 0)
    out = dict(A0=A0.ravel(), h=(half * g if mode == 'gardner' else np.full(dims, half, dtype=rt)).ravel(), S=S.ravel())
    if mode == 'blocks':
        out.update(C=C.ravel(), Smu=Smu.ravel(), chi=chi.ravel(), rho=rho.ravel(), mu0=mu0, inside=inside.ravel())
    return out


def pseudoHessianMoments3(op, uh, A0, h, dtype=np.complex128, magnitude=False):
    """(E, D, Y), each (N,): E = sum_s |u^_i|^2, D = sum_s |r_s|^2, Y = sum_s conj(u^_i) r_s with r_s = A0_i u^_{s,i} + h_i (L u^_s)_i, (L u^)_i the row sum with
    the tables at i on an interior i and zero on a boundary one; uh (N, k).  magnitude: u^ by |Re| + |Im|, the tables by theirs (A0, h those of
    pseudoHessianCoefficients3(magnitude=True)): the majorants."""
    dims = tuple(int(d) for d in op.modelDims)
    uh = np.asarray(uh)
    k = uh.shape[1]
    u = uh.astype(dtype).reshape(dims + (k,))
    if magnitude:
        u = _mag(u)
    lap, _, rt = _lapGeometry3(op, dtype, magnitude)
    T = np.zeros_like(u)
    for d in OFFSETS27:
        T = T + lap(d, 0)[..., None] * _shift3(u, d)
    T = np.where(interiorMask3(dims).reshape(dims + (1,)), T, 0)
    r = np.asarray(A0).reshape(dims + (1,)) * u + np.asarray(h).reshape(dims + (1,)) * T
    N = int(np.prod(dims))
    if magnitude:
        return (u * u).sum(axis=3).ravel(), (r * r).sum(axis=3).ravel(), (u * r).sum(axis=3).ravel()
    E = (u.real * u.real + u.imag * u.imag).sum(axis=3)
    D = (r.real * r.real + r.imag * r.imag).sum(axis=3)
    return E.reshape(N), D.reshape(N), (np.conj(u) * r).sum(axis=3).reshape(N)


def massWeightSquares3(dims):
    """Smu_i = sum_{p interior} mu_{i-p}^2 per cell, (N,) float64.  The interior is a product of three index ranges and mu_d^2 = 1/4 (1 + 2 m0^3) [d == 0] +
    1/4 (m(dx) m(dy) m(dz))^2, so the sum separates: 1/4 (1 + 2 m0^3) [i interior] + 1/4 sz(iz) sy(iy) sx(ix), s(i) = sum_o m(o)^2 [i + o interior]."""
    nz, ny, nx = (int(d) for d in dims)

    def axis(n):
        inside = np.zeros(n + 2)
        inside[2:n] = 1.0                            # (padded by one: the cells 1 .. n - 2)
        return _m(0) ** 2 * inside[1:-1] + _m(1) ** 2 * (inside[:-2] + inside[2:])
    sz, sy, sx = axis(nz), axis(ny), axis(nx)
    b2 = (1.0 - MASS_BLEND) ** 2
    centre = (MASS_BLEND ** 2 + 2.0 * MASS_BLEND * (1.0 - MASS_BLEND) * _m(0) ** 3) * interiorMask3(dims).reshape((nz, ny, nx))
    return (centre + b2 * sz[:, None, None] * sy[None, :, None] * sx[None, None, :]).ravel()


def velocityPseudoHessianWeight3(op):
    '|chi_i|^2 Smu_i per cell, (N,) float64: the closed form of the velocity pseudo-Hessian with an explicit density, H_cc = weight (.) sum_s |u^_i|^2'
    chi = velocityChain3(op)
    return (chi.real * chi.real + chi.imag * chi.imag) * massWeightSquares3(op.modelDims)


def pseudoHessianDiagonal3(op, uh, parameter, chain=None, dtype=np.complex128, magnitude=False, **variant):
    """sum_s ||(dA / dp_i) u^_s||^2 per cell i, (N,) real, for the columns of uh (N, k): parameter 'rho' (density units: H_bb / rho^4), 'c' with chain None (an
    explicit density: the closed form |chi|^2 Smu E) or 'c' with chain = d b / d c per cell (the Gardner total derivative)."""
    if parameter not in ('c', 'rho'):
        raise ValueError('parameter is %r: \'c\' or \'rho\'' % (parameter,))
    if parameter == 'c' and chain is None:
        k = pseudoHessianCoefficients3(op, 'blocks', dtype=dtype, magnitude=magnitude, **variant)
        u = np.asarray(uh).astype(dtype)
        E = (_mag(u) ** 2 if magnitude else u.real * u.real + u.imag * u.imag).sum(axis=1)
        chi2 = k['chi'] * k['chi'] if magnitude else k['chi'].real * k['chi'].real + k['chi'].imag * k['chi'].imag
        return chi2 * k['Smu'] * E
    mode = 'gardner' if parameter == 'c' else 'buoyancy'
    k = pseudoHessianCoefficients3(op, mode, chain, dtype=dtype, magnitude=magnitude, **variant)
    E, D, _ = pseudoHessianMoments3(op, uh, k['A0'], k['h'], dtype, magnitude)
    H = k['S'] * E + D
    if parameter == 'rho':
        rt = _realType(dtype)
        rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), H.shape).astype(rt)
        H = H / (rho * rho * rho * rho)
    return H


def pseudoHessianBlocks3(op, uh, dtype=np.complex128, magnitude=False, **variant):
    """(3, N) real: the rows H_cc, H_crho, H_rhorho of the per-cell 2 x 2 blocks, B_ab[i] = sum_s Re <(dA / da_i) u^_s, (dA / db_i) u^_s>, from the moments:
    H_cc = |chi|^2 Smu E, H_crho = -Re conj(chi) (C' E + mu_0 [i interior] Y) / rho^2, H_rhorho = (S' E + D) / rho^4.  magnitude: the same sums with every term
    by its modulus (the cross entry then is its majorant, not its Cauchy-Schwarz bound)."""
    k = pseudoHessianCoefficients3(op, 'blocks', dtype=dtype, magnitude=magnitude, **variant)
    E, D, Y = pseudoHessianMoments3(op, uh, k['A0'], k['h'], dtype, magnitude)
    chi, rho = k['chi'], k['rho']
    cross = k['C'] * E + np.where(k['inside'], k['mu0'] * Y, 0)
    if magnitude:
        Hcc, Hcb = chi * chi * k['Smu'] * E, chi * cross
    else:
        Hcc, Hcb = (chi.real * chi.real + chi.imag * chi.imag) * k['Smu'] * E, (np.conj(chi) * cross).real
    r2 = rho * rho
    return np.stack([Hcc, (Hcb if magnitude else -Hcb) / r2, (k['S'] * E + D) / (r2 * r2)])


def _boxSum3(e, dims):
    'sum over the 27 rows p = i + d of e[p], (N,) -> (N,)'
    e = np.asarray(e).reshape(dims)
    out = np.zeros_like(e)
    for d in OFFSETS27:
        out = out + _shift3(e, d)
    return out.ravel()


def pseudoHessianColours3(op, uh, parameter, chain=None, L=None, M=None):
    """The same quantities by an independent evaluation: cells with equal (iz, iy, ix) mod 3 have disjoint column supports, so bornSources3 / buoyancySources3 on
    the indicator of a colour, |.|^2 summed over the columns and a 3 x 3 x 3 box sum give H on the cells of that colour exactly -- 27 applications of the
    derivative maps.  parameter 'c' (chain None: explicit density; chain given: the Gardner total), 'rho', or 'blocks' ((3, N))."""
    dims = tuple(int(d) for d in op.modelDims)
    N = int(np.prod(dims))
    L = lapStencil3(op) if L is None else L
    M = massStencil3(dims) if M is None else M
    uh = np.asarray(uh)
    iz, iy, ix = (a.ravel() for a in np.mgrid[0:dims[0], 0:dims[1], 0:dims[2]])
    out = np.zeros((3, N) if parameter == 'blocks' else N)
    for col in OFFSETS27:
        ind = ((iz % 3 == col[0] + 1) & (iy % 3 == col[1] + 1) & (ix % 3 == col[2] + 1))
        if not ind.any():
            continue
        v = ind.astype(np.float64)
        vc = vb = None
        if parameter in ('c', 'blocks'):
            vc = bornSources3(op, v, uh, M)
            if chain is not None:
                vc = vc + buoyancySources3(op, np.asarray(chain) * v, uh, L, M)
        if parameter in ('rho', 'blocks'):
            vb = buoyancySources3(op, densityChain3(op) * v, uh, L, M)
        n2 = lambda a, b_: _boxSum3((np.conj(a) * b_).real.sum(axis=1), dims)
        if parameter == 'blocks':
            for row, (a, b_) in enumerate(((vc, vc), (vc, vb), (vb, vb))):
                out[row, ind] = n2(a, b_)[ind]
        else:
            x = vc if parameter == 'c' else vb
            out[ind] = n2(x, x)[ind]
    return out
