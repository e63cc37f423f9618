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
