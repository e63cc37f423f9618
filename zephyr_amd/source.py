"""Right-hand-side generators (interface of zephyr/backend/source.py:17-351).

Host-side input producers of the hot path: a unit delta at the nearest node, the stacked
(2N) variant used with Eurus, and Hicks' Kaiser-windowed-sinc point sources returned as a
scipy sparse (N, nsrc) matrix.  Locations are physical (x, z) pairs; with `ny` in the config (a 3-D grid, which the reference
refuses: source.py:43-44) they are (x, y, z) triples and the Kaiser patch is the separable product of the same 1-D responses.
"""
import warnings
import numpy as np
import scipy.sparse as sp
from scipy.special import i0

from .base import BaseModelDependent, BaseAnisotropic


class BaseSource(BaseModelDependent):
    pass


class FakeSource(BaseSource):
    'Pass-through used with analytical systems (source.py:23-28)'

    def __call__(self, loc):
        return loc


class SimpleSource(BaseSource):
    """Unit delta at the grid node nearest to each location (source.py:31-107)."""

    def __init__(self, systemConfig):
        BaseSource.__init__(self, systemConfig)
        if hasattr(self, 'ny'):
            if not self.SERVES_3D:
                raise NotImplementedError('%s has no 3-D form (`ny` is in the config): SimpleSource, SparseKaiserSource and KaiserSource serve (x, y, z) '
                                          'locations' % (type(self).__name__,))
            return                  # (3-D: the nearest node is found per axis, no (nsrc, nz, ny, nx) distance field is built)
        nz, nx = int(self.nz), int(self.nx)
        # node coordinates exactly as np.mgrid[orig : orig + d*n : d] produces them (source.py:51-54)
        self._z, self._x = np.mgrid[self.zorig:self.zorig + self.dz * nz:self.dz,
                                    self.xorig:self.xorig + self.dx * nx:self.dx]

    SERVES_3D = True         # (classes that have no 3-D form refuse `ny` in their constructor)

    def _axes3(self):
        '(origin, spacing, nodes) of the x, y and z axes of a 3-D grid, in the order of a location triple'
        return ((self.xorig, self.dx, int(self.nx)), (self.yorig, self.dy, int(self.ny)), (self.zorig, self.dz, int(self.nz)))

    def _nearest3(self, loc):
        """(ix, iy, iz) of the node nearest to each (x, y, z) location, int64 (nsrc,) each.  The squared distance is a sum over the axes, so its first
        minimum in linear-index order -- what np.argmin of the full distance field returns -- is the first minimum of every axis."""
        loc = np.asarray(loc, dtype=np.float64)
        if loc.ndim != 2 or loc.shape[1] != 3:
            raise ValueError('with `ny` in the config locations are (x, y, z) triples: an array of shape (n, 3), not %s' % (loc.shape,))
        return tuple(np.argmin(np.abs((o + d * np.arange(n))[None, :] - loc[:, a:a + 1]), axis=1) for a, (o, d, n) in enumerate(self._axes3()))

    def dist(self, loc):
        'distance of every node from every location, shape (nsrc, nz, nx) (source.py:56-77)'
        if hasattr(self, 'ny'):
            raise NotImplementedError('dist() builds the 2-D distance field: a 3-D grid finds its nearest nodes per axis (linIndexOf)')
        loc = np.asarray(loc)
        n = len(loc)
        ddx = self._x[None, :, :] - loc[:, 0].reshape((n, 1, 1))
        ddz = self._z[None, :, :] - loc[:, 1].reshape((n, 1, 1))
        return np.sqrt(ddx ** 2 + ddz ** 2)

    def linIndexOf(self, loc):
        'linear index of the nearest node (first minimum, as np.argmin) (source.py:83-88)'
        if hasattr(self, 'ny'):
            ix, iy, iz = self._nearest3(loc)
            return (iz * int(self.ny) + iy) * int(self.nx) + ix
        n = np.asarray(loc).shape[0]
        return np.argmin(self.dist(loc).reshape((n, -1)), axis=1)

    def vecIndexOf(self, loc):
        return self.toVecIndex(self.linIndexOf(loc))

    def __call__(self, loc):
        'dense (N, nsrc) complex right-hand sides (source.py:90-107)'
        idx = self.linIndexOf(loc)
        q = np.zeros((self.nrow, len(idx)), dtype=np.complex128)
        q[idx, np.arange(len(idx))] = 1.
        return q


class StackedSimpleSource(SimpleSource):
    """SimpleSource augmented with N zero rows for the second Eurus field (source.py:110-119)."""

    SERVES_3D = False        # (Eurus is 2-D: there is no second field to stack in 3-D)

    def __call__(self, loc):
        q = SimpleSource.__call__(self, loc)
        return np.vstack([q, np.zeros(q.shape, dtype=np.complex128)])


class SparseKaiserSource(SimpleSource):
    """Kaiser-windowed-sinc point sources (Hicks 2002) as a sparse (N, nsrc) matrix (source.py:122-322)."""

    initMap = {
        'ireg':           (False,    '_ireg',      np.int64),
        'freeSurf':       (False,    '_freeSurf',  tuple),
    }

    # Hicks' optimal Kaiser b for each half-width (source.py:138-149)
    HC_KAISER = {1: 1.24, 2: 2.94, 3: 4.53, 4: 6.31, 5: 7.91, 6: 9.42, 7: 10.95, 8: 12.53, 9: 14.09, 10: 14.18}

    @property
    def ireg(self):
        'half-width of the source region in nodes (default 4)'
        return getattr(self, '_ireg', 4)

    @staticmethod
    def modifyGrid(Zi, Xi, aZi, aXi):
        return Zi, Xi

    def kws(self, offset, aZi, aXi):
        'the (2 ireg + 1)^2 windowed-sinc patch for a source `offset` cells off its nearest node (source.py:156-211)'
        ireg = int(self.ireg)
        b = self.HC_KAISER.get(ireg)
        width = 2 * ireg + 1
        xoff, zoff = offset
        Zi, Xi = np.mgrid[:width, :width]
        Zi, Xi = self.modifyGrid(Zi, Xi, aZi, aXi)
        dZ = zoff + ireg - Zi
        dX = xoff + ireg - Xi
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            tZ = np.nan_to_num(np.sqrt(1 - (dZ / ireg) ** 2))
            tX = np.nan_to_num(np.sqrt(1 - (dX / ireg) ** 2))
            tZ[tZ == np.inf] = 0
            tX[tX == np.inf] = 0
        respZ = np.sinc(dZ) * (i0(b * tZ) / i0(b))
        respX = np.sinc(dX) * (i0(b * tX) / i0(b))
        return respX * respZ

    def _response1(self, off):
        'the 2 ireg + 1 windowed-sinc responses of one axis for a source `off` cells off its nearest node: the 1-D factor of `kws`'
        ireg = int(self.ireg)
        b = self.HC_KAISER.get(ireg)
        d = off + ireg - np.arange(2 * ireg + 1)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t = np.nan_to_num(np.sqrt(1 - (d / ireg) ** 2))
            t[t == np.inf] = 0
        return np.sinc(d) * (i0(b * t) / i0(b))

    def _call3(self, sLocs):
        """3-D: sparse (N, nsrc) right-hand sides, column s the separable (2 ireg + 1)^3 product of the 1-D responses of its three offsets, scaled by
        1 / (dx dy dz) and clipped at the six faces; ireg = 0: the scaled delta.  The 3-D operator has no free surface."""
        if any(self.freeSurf):
            raise ValueError('freeSurf is %r: the 3-D operator has no free surface (C-PML on all six faces); leave freeSurf out of a 3-D config' % (tuple(self.freeSurf),))
        sLocs = np.asarray(sLocs, dtype=np.float64)
        ireg = int(self.ireg)
        nsrc = sLocs.shape[0]
        nz, ny, nx = int(self.nz), int(self.ny), int(self.nx)
        N = nz * ny * nx
        scale = 1. / (self.dx * self.dy * self.dz)
        idx = self._nearest3(sLocs)
        if ireg == 0:
            node = (idx[2] * ny + idx[1]) * nx + idx[0]
            return sp.coo_matrix((scale * np.ones(nsrc, dtype=np.complex128), (np.arange(nsrc), node)), shape=(nsrc, N)).T
        data, rows, cols = [], [], []
        for i in range(nsrc):
            resp, where = [], []
            for a, (o, d, n) in enumerate(self._axes3()):
                node = int(idx[a][i])
                r = self._response1(sLocs[i, a] - o - node * d)
                j = node + np.arange(-ireg, ireg + 1)
                keep = (j >= 0) & (j < n)                       # (clipped at the two faces of this axis)
                resp.append(r[keep]); where.append(j[keep])
            (rx, ry, rz), (jx, jy, jz) = resp, where
            patch = scale * (rz[:, None, None] * ry[None, :, None] * rx[None, None, :])
            lin = (jz[:, None, None] * ny + jy[None, :, None]) * nx + jx[None, None, :]
            data.append(patch.ravel()); cols.append(lin.ravel()); rows.append(np.full(patch.size, i))
        q = sp.coo_matrix((np.concatenate(data).astype(np.complex128), (np.concatenate(rows), np.concatenate(cols))), shape=(nsrc, N), dtype=np.complex128)
        return q.T

    def __call__(self, sLocs):
        'sparse (N, nsrc) right-hand sides; patches are clipped (or mirrored with sign flip under a free surface) at the edges (source.py:213-317)'
        if hasattr(self, 'ny'):
            return self._call3(sLocs)
        sLocs = np.asarray(sLocs)
        ireg = int(self.ireg)
        fs = self.freeSurf
        nsrc = sLocs.shape[0]
        nz, nx = int(self.nz), int(self.nx)
        N = nz * nx
        scale = 1. / (self.dx * self.dz)
        node = self.linIndexOf(sLocs)

        if ireg == 0:
            q = sp.coo_matrix((scale * np.ones(nsrc), (np.arange(nsrc), node)), shape=(nsrc, N))
            return q.T

        zsh, xsh = np.mgrid[-ireg:ireg + 1, -ireg:ireg + 1]
        lin_shift = zsh * nx + xsh
        data, rows, cols = [], [], []
        for i in range(nsrc):
            Zi, Xi = node[i] // nx, np.mod(node[i], nx)
            off = (sLocs[i][0] - self.xorig - Xi * self.dx, sLocs[i][1] - self.zorig - Zi * self.dz)
            patch = self.kws(off, Zi, Xi)
            shift = lin_shift.copy()

            if Zi < ireg:                                   # patch sticks out above iz = 0
                k = ireg - Zi
                if fs[2]:
                    lift = np.flipud(patch[:k, :])
                patch = patch[k:, :]
                shift = shift[k:, :]
                if fs[2]:
                    patch[:k, :] -= lift
            if Zi > nz - ireg - 1:                          # below iz = nz-1
                k = nz - ireg - 1 - Zi
                if fs[0]:
                    lift = np.flipud(patch[k:, :])
                patch = patch[:k, :]
                shift = shift[:k, :]
                if fs[0]:
                    patch[k:, :] -= lift
            if Xi < ireg:                                   # left of ix = 0
                k = ireg - Xi
                if fs[3]:
                    lift = np.fliplr(patch[:, :k])
                patch = patch[:, k:]
                shift = shift[:, k:]
                if fs[3]:
                    patch[:, :k] -= lift
            if Xi > nx - ireg - 1:                          # right of ix = nx-1
                k = nx - ireg - 1 - Xi
                if fs[1]:
                    lift = np.fliplr(patch[:, k:])
                patch = patch[:, :k]
                shift = shift[:, :k]
                if fs[1]:
                    patch[:, k:] -= lift

            data.append(scale * patch.ravel())
            cols.append(node[i] + shift.ravel())
            rows.append(np.full(patch.size, i))

        q = sp.coo_matrix((np.concatenate(data).astype(np.complex128), (np.concatenate(rows), np.concatenate(cols))),
                          shape=(nsrc, N), dtype=np.complex128)
        return q.T


class KaiserSource(SparseKaiserSource):
    'dense version of SparseKaiserSource (source.py:325-334)'

    def __call__(self, sLocs):
        return SparseKaiserSource.__call__(self, sLocs).toarray()


class AnisotropicKaiserSource(SparseKaiserSource, BaseAnisotropic):
    'Kaiser source on the anisotropically stretched local grid (source.py:337-351)'

    SERVES_3D = False        # (theta, eps and delta are fields of the 2-D anisotropic operators)

    def modifyGrid(self, Zi, Xi, aZi, aXi):
        theta = self.theta[aZi, aXi]
        epsilon = self.eps[aZi, aXi]
        delta = self.delta[aZi, aXi]
        root = np.sqrt(1 + (2 * delta))
        wx = (1. + (2 * epsilon) + root) / (1 + epsilon + root)
        wz = (1. + root) / (1 + epsilon + root)
        Xn = Xi * (wx * np.cos(theta)) + Xi * (wz * np.sin(theta))
        Zn = Zi * (wx * np.sin(theta)) + Zi * (wz * np.cos(theta))
        return Zn, Xn
