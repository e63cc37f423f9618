"""Shared by tests/test_survey3d_host.py (CPU) and tests/test_gpu_survey3d.py (GPU): an splu-backed stand-in for Helm3D on the oracle's matrix (and its
transposed class), the plane formula of the transposed 27-point operator in numpy, the surveys the 3-D routes are tested on, and the
extended-precision references of the two mass-stencil kernels with their rounding bounds."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import helm3d_oracle as h3
import zephyr_amd as za

U53 = 2.0 ** -53


def oracle_matrix(op):
    "the oracle's CSR matrix of a Helm3D-like object (untransposed)"
    nz, ny, nx = (int(d) for d in op.modelDims)
    C = h3.helm3d_coefficients(nz, ny, nx, op.c, op.rho, complex(op.freq), dx=float(op.dx), dy=float(op.dy), dz=float(op.dz), tau=float(op.tau),
                               nPML=int(op.nPML), cPML=float(op.cPML))
    return h3.coefficients_to_csr3(C)


class OracleHelm3D(za.Helm3D):
    """Helm3D whose matrix is the oracle's and whose `* q` is a sparse LU of it: conj(A^-1 premul q); its class `Transposed` (OracleHelm3DT): conj(A^-T premul q).  No GPU."""

    @property
    def A(self):
        if getattr(self, '_A', None) is None:
            A = oracle_matrix(self)
            self._A = sp.csr_matrix(A.T) if self.transposed else A
        return self._A

    def __mul__(self, rhs):
        if sp.issparse(rhs):
            rhs = rhs.toarray()
        if getattr(self, '_lu', None) is None:
            self._lu = spla.splu(sp.csc_matrix(self.A))
        return np.conj(self._lu.solve(complex(self.premul) * np.asarray(rhs, dtype=np.complex128)))

    def __getstate__(self):
        state = za.Helm3D.__getstate__(self)
        state.pop('_lu', None)
        return state


class OracleHelm3DT(OracleHelm3D, za.Helm3DTransposed):
    'the stand-in of Helm3DTransposed: the LU of the transposed oracle matrix'


OracleHelm3D.Transposed = OracleHelm3DT


def transpose_planes3(C):
    """the planes of A^T from the planes C (27, nz, ny, nx) of A: CT[k(o)][p] = C[26 - k(o)][p + o], zero where p + o is outside the grid (per axis)"""
    C = np.asarray(C)
    _, nz, ny, nx = C.shape
    CT = np.zeros_like(C)
    for k, (oz, oy, ox) in enumerate(h3.OFFSETS3):
        z0, z1 = max(0, -oz), nz - max(0, oz)
        y0, y1 = max(0, -oy), ny - max(0, oy)
        x0, x1 = max(0, -ox), nx - max(0, ox)
        CT[k, z0:z1, y0:y1, x0:x1] = C[26 - k, z0 + oz:z1 + oz, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return CT


def randc(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def inner(a, b):
    '<a, b> = Re sum conj(a) b'
    return float(np.real(np.vdot(np.asarray(a).ravel(), np.asarray(b).ravel())))


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def survey_config(dims, nPML, freqs, mode, nsrc=3, nrec=10, spacing=(10., 9., 11.), seed=1, rec_patch=None):
    """random c of 1900-2300 m/s and rho of 1000-1100 on a (nz, ny, nx) grid with dx != dy != dz, `nsrc` sources off the nodes -- the last one inside the
    absorbing layer --, `nrec` receivers on a slanted line that starts next to the layer (offsets around the source when the array moves with it; rec_patch
    (ny_r, nx_r): a patch of receivers instead), complex source, receiver and frequency terms."""
    nz, ny, nx = dims
    dx, dy, dz = spacing
    rng = np.random.default_rng(seed)
    c = 1900. + 400. * rng.random(dims)
    rho = 1000. + 100. * rng.random(dims)
    X, Y, Z = dx * (nx - 1), dy * (ny - 1), dz * (nz - 1)
    lo = nPML + 1
    src = np.stack([np.linspace(dx * (lo + 0.3), X - dx * (lo + 0.6), nsrc), np.linspace(dy * (lo + 0.7), Y - dy * (lo + 0.2), nsrc),
                    np.full(nsrc, dz * (lo + 0.4))], axis=1)
    src[-1] = (dx * 1.4, dy * (ny - 2.7), dz * 1.6)                    # inside the layer
    if rec_patch is not None:
        gy, gx = np.meshgrid(np.linspace(-1.6 * dy, 1.7 * dy, rec_patch[0]), np.linspace(-2.3 * dx, 2.1 * dx, rec_patch[1]), indexing='ij')
        if mode == 'fixed':
            rec = np.stack([X / 2 + gx.ravel(), Y / 2 + gy.ravel(), np.full(gx.size, Z - dz * (lo + 0.7))], axis=1)
        else:
            rec = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, dz * 2.2)], axis=1)
    elif mode == 'fixed':
        rec = np.stack([np.linspace(dx * (nPML + 0.1), X - dx * (nPML + 0.2), nrec), np.linspace(dy * (nPML + 0.3), Y - dy * (nPML + 0.1), nrec),
                        np.linspace(Z - dz * (lo + 1.7), Z - dz * (nPML + 0.2), nrec)], axis=1)
    else:
        rec = np.stack([np.linspace(-2.3 * dx, 2.1 * dx, nrec), np.linspace(-1.2 * dy, 1.9 * dy, nrec), np.full(nrec, dz * 2.2)], axis=1)
    geom = dict(src=src, rec=rec, mode=mode, sterms=randc(rng, nsrc), rterms=randc(rng, len(rec)))
    return dict(nx=nx, ny=ny, nz=nz, dx=dx, dy=dy, dz=dz, c=c, rho=rho, nPML=nPML, cPML=250., freqs=list(freqs), sterms=randc(rng, len(freqs)), geom=geom,
                parallel=False)


HOST_GRIDS = {'12x11x13': ((12, 11, 13), 3, (5., 6.)), '18x16x20': ((18, 16, 20), 4, (6.,))}


def host_pair(grid, mode='fixed', **extra):
    """(prob, survey) of a CPU case on OracleHelm3D: three sources, ten receivers, a complex scaleTerm and a complex premul (they tell the conjugations
    apart); the numpy routes are forced (hostGradient), so that the cases mean the same on a machine with a GPU."""
    dims, npml, freqs = HOST_GRIDS[grid]
    sc = survey_config(dims, npml, freqs, mode)
    sc.update(Disc=OracleHelm3D, hostGradient=True, scaleTerm=0.7 - 0.2j, premul=1.1 + 0.3j, tau=1.5)
    sc.update(extra)
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    return prob, sv


# ---- extended-precision references of the mass-stencil kernels ---------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a).astype(np.clongdouble)


def _mu_sum(T, weights=None):
    'sum_o mu_o T[p + o] on a (nz, ny, nx, k) array, cells outside the grid contributing nothing; longdouble weights'
    nz, ny, nx = T.shape[:3]
    Tp = np.zeros((nz + 2, ny + 2, nx + 2) + T.shape[3:], dtype=T.dtype)
    Tp[1:-1, 1:-1, 1:-1] = T
    out = np.zeros_like(T)
    third, sixth = np.longdouble(2) / np.longdouble(3), np.longdouble(1) / np.longdouble(6)
    for (oz, oy, ox) in h3.OFFSETS3:
        m = np.longdouble(0.5) * (third if ox == 0 else sixth) * (third if oy == 0 else sixth) * (third if oz == 0 else sixth)
        if (oz, oy, ox) == (0, 0, 0):
            m = m + np.longdouble(0.5)
        out += m * Tp[1 + oz:1 + oz + nz, 1 + oy:1 + oy + ny, 1 + ox:1 + ox + nx]
    return out


def _interior(dims):
    m = np.zeros(dims, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def _l1(a):
    'the componentwise majorant |Re a| + |Im a|, longdouble'
    return np.abs(a.real).astype(np.longdouble) + np.abs(a.imag).astype(np.longdouble)


def mass_sources_reference(dims, U, W, coef, conj):
    """(R, bound): R[s] = coef M~(W (.) X_s) in 80-bit arithmetic for the columns U (k, N), and the componentwise bound on the error of the fp64 kernel.
    Rounded operations per output component, relative to the majorant (|Re coef| + |Im coef|) sum_o mu_o a_{p+o}, a = (|Re W| + |Im W|)(|Re X| + |Im X|):
    2 for the product W X (two multiplications and an addition, one of the products entering the sum exactly or not at all), 4 per level of the separable sum
    (the rounded constant, the multiplication, the neighbour addition, the final addition) times 3 levels, 1 for the blend, 2 for the product with coef: 17,
    taken as 20 u.  Fused multiply-adds only remove roundings."""
    k, N = U.shape
    X = _ld(np.conj(U) if conj else U).T.reshape(dims + (k,))
    Wl = _ld(W).reshape(dims + (1,))
    S = _mu_sum(Wl * X)
    inside = _interior(dims)[..., None]
    R = np.where(inside, np.clongdouble(coef) * S, 0)
    maj = _mu_sum((_l1(Wl) * _l1(X)).astype(np.clongdouble)).real
    bound = np.where(inside, 20 * U53 * (abs(coef.real) + abs(coef.imag)) * maj, 0)
    return R.reshape((N, k)).T, bound.reshape((N, k)).T


def mass_imaging_reference(dims, UF, UB, P0):
    """(P, bound): P = P0 + sum_s UF_s (.) (M~^T UB_s) in 80-bit arithmetic, the boundary rows of UB masked, and the componentwise bound on the fp64 kernel:
    13 roundings in the mu sum, 2 in each product with UF, one addition per source into the running sum and one into P0 -- (16 + k) u relative to
    |P0| + sum_s (|Re UF| + |Im UF|) sum_o mu_o (|Re UB| + |Im UB|), taken as (20 + 2 k) u."""
    k, N = UF.shape
    inside = _interior(dims)[..., None]
    L = np.where(inside, _ld(UB).T.reshape(dims + (k,)), 0)
    F = _ld(UF).T.reshape(dims + (k,))
    P = _ld(P0).reshape(dims) + (F * _mu_sum(L)).sum(axis=3)
    maj = _l1(_ld(P0).reshape(dims)) + (_l1(F) * _mu_sum(_l1(L).astype(np.clongdouble)).real).sum(axis=3)
    return P.ravel(), ((20 + 2 * k) * U53 * maj).ravel()
