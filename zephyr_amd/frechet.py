"""What the exact Frechet derivative of MiniZephyr (linearisation='operator' of HelmBaseProblem.JvecBorn / Jtvec / Hvec) is made of, in numpy: the mass
term of the 9-point operator.  MiniZephyr carries the velocity as K = (omega_d^2 / c^2 - ky^2) / rho of the NEIGHBOURING cell, spread over the nine slots of a
row by the mass weights, and overwrites its boundary rows by +-identity, so

    (dA) u = mask_int (.) M0(dK (.) u),      dK = -2 omega_d^2 v / (c^3 rho)

The host routes of problem.py evaluate this here; the device routes (device_survey.py) take the scalars from here and run the stencil in
k_virtual_sources_op / k_imaging_op (csrc/survey.hip)."""
import numpy as np


MZ_MASS = (0.6248, 0.09381, 0.000001297)      # centre, edge and corner weights of the lumped/consistent mass average (minizephyr.py:207-209)


def maskInterior(u, nz, nx):
    "a copy of u ((N,) or (N, k), N = nz nx, z-major) with the four boundary lines zeroed: mask_int (.) u"
    a = np.array(u).reshape((int(nz), int(nx)) + np.shape(u)[1:])
    a[0], a[-1], a[:, 0], a[:, -1] = 0, 0, 0, 0
    return a.reshape(np.shape(u))


def massStencil(u, nz, nx, mask=False):
    """M0 u: the constant 9-point stencil of the mass weights on the nz x nx grid (neighbours outside the grid contribute nothing), column by column of
    u ((N,) or (N, k)).  The sum runs centre, then the four edges (up, down, left, right), then the four corners -- the order of the device kernels.
    mask: mask_int (.) M0 u."""
    nz, nx = int(nz), int(nx)
    a = np.asarray(u).reshape((nz, nx) + np.shape(u)[1:])
    p = np.zeros((nz + 2, nx + 2) + a.shape[2:], dtype=a.dtype)
    p[1:-1, 1:-1] = a
    mc, md, me = MZ_MASS
    sh = lambda dz, dx: p[1 + dz:1 + dz + nz, 1 + dx:1 + dx + nx]
    out = mc * a + md * (((sh(-1, 0) + sh(1, 0)) + sh(0, -1)) + sh(0, 1)) + me * (((sh(-1, -1) + sh(-1, 1)) + sh(1, -1)) + sh(1, 1))
    out = out.reshape(np.shape(u))
    return maskInterior(out, nz, nx) if mask else out


def dampedOmega(op):
    "omega_d = 2 pi f - i / tau of an operator (f may be complex)"
    return 2.0 * np.pi * complex(op.freq) - 1j / float(op.tau)


def operatorWeight(op):
    "d K / d c of a MiniZephyr operator per cell, (N,) complex: K = (omega_d^2 / c^2 - (2 pi ky)^2) / rho, so -2 omega_d^2 / (c^3 rho), omega_d = 2 pi f - i / tau"
    om = dampedOmega(op)
    c = np.asarray(op.c, dtype=np.complex128).ravel()
    return -2.0 * om * om / (c * c * c * np.asarray(op.rho, dtype=np.float64).ravel())
