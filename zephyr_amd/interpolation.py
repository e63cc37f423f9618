"""Transfers between regular grids (interface of zephyr/backend/interpolation.py:12-205).

`SplineGridInterpolator(sc) * f` carries a field on the (nz, nx) grid of `sc` to the grid coarsened by `scale` -- what the reference does with
scipy's RectBivariateSpline(kx=3, ky=3, s=0) (not-a-knot cubic interpolation along each axis, points beyond the input's extent clamped to its
edge) -- in libhelm (zephyr_amd/csrc/regrid.hip): the 1-D operators are built once per grid pair and applied by two windowed passes on the GPU.
Building an interpolator and reading its geometry needs no GPU; the first application creates the plan of its device and grid pair.

One deliberate difference from the reference: `.T` lands exactly on the native grid (the reference recomputes round(snx * scale), which can be
one node off -- nx = 101, scale = 3 gives 102).
"""
import ctypes
import threading
import numpy as np

from .base import BaseModelDependent
from .config import BaseSCCache
from . import _lib


_PLANS = {}
_PLANS_MU = threading.Lock()


def regrid_plan(device, src, dst, zorig=0., xorig=0.):
    'the transfer plan of `device` from grid src = (nz, nx, dz, dx) to grid dst, created on first use and kept for the process'
    key = (int(device),) + tuple(int(v) for v in src[:2]) + tuple(float(v) for v in src[2:]) + tuple(int(v) for v in dst[:2]) + tuple(float(v) for v in dst[2:])
    with _PLANS_MU:
        plan = _PLANS.get(key)
        if plan is None:
            lib = _lib.load()
            _lib.require_gpu()
            plan = lib.helm_regrid_create(int(device), int(src[0]), int(src[1]), float(src[2]), float(src[3]),
                                          int(dst[0]), int(dst[1]), float(dst[2]), float(dst[3]), float(zorig), float(xorig))
            if not plan:
                raise _lib.HelmError(-1, _lib.last_error())
            _PLANS[key] = plan
    return plan


def regrid_axis(n_in, h_in, n_out, h_out):
    'the 1-D transfer of helm_regrid_axis as (start[n_out], taps[n_out, W]) (host only)'
    lib = _lib.load()
    W = _lib.check(lib.helm_regrid_axis(int(n_in), float(h_in), int(n_out), float(h_out), None, None, 0))
    start = np.zeros(int(n_out), dtype=np.int32)
    taps = np.zeros((int(n_out), W), dtype=np.float64)
    _lib.check(lib.helm_regrid_axis(int(n_in), float(h_in), int(n_out), float(h_out), _lib.ptr(start), _lib.ptr(taps), taps.size))
    return start, taps


class BaseGridInterpolator(BaseModelDependent, BaseSCCache):
    """Geometry of a transfer between the native grid of a config and the grid coarsened by `scale` (interpolation.py:12-177)."""

    initMap = {
        #   key            required  rename        cast
        'scale':          (True,     None,         np.float64),
        'eCons':          (False,    '_eCons',     bool),
    }

    @property
    def eCons(self):
        return getattr(self, '_eCons', False)

    @staticmethod
    def genGrid(nx, nz, dx, dz, xorig, zorig):
        Zi, Xi = np.mgrid[0:nz, 0:nx]
        return Zi * dz + zorig, Xi * dx + xorig

    @property
    def nativeGrid(self):
        return self.genGrid(self.nx, self.nz, self.dx, self.dz, self.xorig, self.zorig)

    @property
    def Xg(self):
        return self.nativeGrid[1]

    @property
    def Zg(self):
        return self.nativeGrid[0]

    @property
    def Z(self):
        return self.zorig + self.dz * np.arange(self.nz)

    @property
    def X(self):
        return self.xorig + self.dx * np.arange(self.nx)

    # target grid: the native grid coarsened by `scale` (numpy's round: half to even), or -- for the transpose -- the grid it came from
    @property
    def snx(self):
        t = self.__dict__.get('_target')
        return int(t[0]) if t else int(np.round(self.nx / self.scale))

    @property
    def snz(self):
        t = self.__dict__.get('_target')
        return int(t[1]) if t else int(np.round(self.nz / self.scale))

    @property
    def sdx(self):
        t = self.__dict__.get('_target')
        return float(t[2]) if t else self.dx * self.scale

    @property
    def sdz(self):
        t = self.__dict__.get('_target')
        return float(t[3]) if t else self.dz * self.scale

    @property
    def scaledGrid(self):
        return self.genGrid(self.snx, self.snz, self.sdx, self.sdz, self.xorig, self.zorig)

    @property
    def sXg(self):
        return self.scaledGrid[1]

    @property
    def sZg(self):
        return self.scaledGrid[0]

    @property
    def sZ(self):
        return self.zorig + self.sdz * np.arange(self.snz)

    @property
    def sX(self):
        return self.xorig + self.sdx * np.arange(self.snx)

    @property
    def compression(self):
        return self.scale ** 2

    @property
    def shape(self):
        return (self.snx * self.snz, self.nx * self.nz)

    @property
    def T(self):
        'the transfer back to this grid (lands exactly on it; see the module docstring)'
        if '_T' not in self.__dict__:
            sc = dict(self.systemConfig)
            sc.update({'scale': 1. / self.scale, 'nx': self.snx, 'nz': self.snz, 'dx': self.sdx, 'dz': self.sdz})
            t = self.__class__(sc)
            t._target = (self.nx, self.nz, self.dx, self.dz)
            t._T = self
            self._T = t
        return self._T

    @property
    def scaleUpdate(self):
        return {'nx': self.snx, 'nz': self.snz, 'dx': self.sdx, 'dz': self.sdz}

    def __mul__(self, value):
        raise NotImplementedError

    def __call__(self, value):
        return self * value


class SplineGridInterpolator(BaseGridInterpolator):
    """Bicubic-spline transfer (interpolation.py:180-205) run by libhelm.  `* f`: host arrays of shape (N,) or (N, k), real or complex;
    `apply_device`: device buffers."""

    @property
    def identity(self):
        return self.shape[0] == self.shape[1]

    @property
    def gain(self):
        return self.compression if self.eCons else 1.

    def _grids(self):
        return (self.nz, self.nx, self.dz, self.dx), (self.snz, self.snx, self.sdz, self.sdx)

    def plan(self, device):
        src, dst = self._grids()
        return regrid_plan(device, src, dst, self.zorig, self.xorig)

    @property
    def device(self):
        dev = self.systemConfig.get('device')
        if dev is not None:
            return int(dev)
        from . import dispatch
        return int(dispatch.visible_devices()[0])

    def __mul__(self, rhs):
        if self.identity:
            return rhs
        if hasattr(rhs, 'toarray'):
            rhs = rhs.toarray()
        rhs = np.asarray(rhs)
        if rhs.ndim > 2:
            raise NotImplementedError('%s does not support %dD inputs' % (self.__class__.__name__, rhs.ndim))
        na, nb = self.shape[1], self.shape[0]
        if rhs.shape[0] != na:
            raise ValueError('%s: input has %d rows, the grid %d points' % (self.__class__.__name__, rhs.shape[0], na))
        real = not np.iscomplexobj(rhs)
        k = 1 if rhs.ndim == 1 else rhs.shape[1]
        src = np.ascontiguousarray(rhs, dtype=np.complex128)
        out = np.empty((nb,) if rhs.ndim == 1 else (nb, k), dtype=np.complex128)
        if k:
            lib = _lib.load()
            plan = self.plan(self.device)
            # (N, k) C order: element i of field f at f + i k
            _lib.check(lib.helm_regrid_apply(plan, k, src.ctypes.data_as(ctypes.c_void_p), 1, k, out.ctypes.data_as(ctypes.c_void_p), 1, k,
                                             float(self.gain), 0., 0., None))
        return out.real.copy() if real else out

    def apply_device(self, src, dst, k=None, op=None, gain=1., beta=0., mul=None, layout='kN', device=None):
        """dst = beta dst + mul (.) (gain' T src) for k complex128 fields held on the device (torch tensors or pointers), gain' = gain times the
        eCons factor.  layout 'kN': field f contiguous at f N (the fast one); 'Nk': element i of all fields contiguous at i k.  `op`: a
        discretization (or raw handle) whose stream the transfer is queued on, after what that stream already holds; mul: N_b complex or None.
        Returns when the transfer is done."""
        def addr(x):
            return None if x is None else (int(x.data_ptr()) if hasattr(x, 'data_ptr') else int(x))
        if k is None:
            k = 1 if src.dim() == 1 else (src.shape[0] if layout == 'kN' else src.shape[1])
        if device is None:
            device = src.device.index if hasattr(src, 'device') else self.device
        na, nb = self.shape[1], self.shape[0]
        ifs, ies = (na, 1) if layout == 'kN' else (1, k)
        ofs, oes = (nb, 1) if layout == 'kN' else (1, k)
        handle = getattr(op, 'handle', op)
        g = complex(gain) * self.gain
        if self.identity:                  # (the reference's identity case: the same grid, nothing to interpolate)
            if not hasattr(src, 'data_ptr'):
                raise TypeError('apply_device of an identity transfer takes torch tensors')
            v = src * g if mul is None else (src * g) * (mul if layout == 'kN' else mul.reshape(-1, 1))
            if beta == 0.:
                dst.copy_(v)
            else:
                dst.mul_(beta).add_(v)
            return dst
        lib = _lib.load()
        _lib.check(lib.helm_regrid_apply_device(self.plan(device), handle, int(k), addr(src), ifs, ies, addr(dst), ofs, oes,
                                                g.real, g.imag, float(beta), addr(mul)), handle)
        return dst
