"""Host maps of the exact velocity derivative of the 3-D 27-point operator (numpy / scipy): what `Helm3DProblem` runs when the device routes do not serve
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
