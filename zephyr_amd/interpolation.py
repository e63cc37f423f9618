"""Transfers between regular grids (interface of zephyr/backend/interpolation.py:12-205).

`SplineGridInterpolator(sc) * f` carries a field on the (nz, nx) grid of `sc` to the grid coarsened by `scale` -- what the reference does with
scipy's RectBivariateSpline(kx=3, ky=3, s=0) (not-a-knot cubic interpolation along each axis, points beyond the input's extent clamped to its
edge) -- in libhelm (zephyr_amd/csrc/regrid.hip): the 1-D operators are built once per grid pair and applied by two windowed passes on the GPU.
Building an interpolator and reading its geometry needs no GPU; the first application creates the plan of its device and grid pair.

One deliberate difference from the reference: `.T` lands exactly on the native grid (the reference recomputes round(snx * scale), which can be
one node off -- nx = 101, scale = 3 gives 102).

`.T` interpolates back up; it is not the transpose of the matrix.  That is `.adjoint`: the exact transpose of the windowed transfer the device
applies (helm_regrid_create_t), which a derivative of anything computed on the coarse grid needs.  The forward transfer samples the field at
the coarse nodes, it does not average it, so the adjoint puts a coarse value on the few native nodes around its sample point: the column sums
of a 1-D axis at scale 2.47 run from -0.25 to 1.07, and at an integer scale s only every s-th node receives anything.  `.matrix` is the
forward transfer as a scipy CSR built on the host from the same taps; with the config key `hostTransfer=True`, `*` uses it instead of the GPU.
"""
import ctypes
import threading
import numpy as np

from .base import BaseModelDependent
from .config import BaseSCCache
from . import _lib


_PLANS = {}
_PLANS_MU = threading.Lock()


def regrid_plan(device, src, dst, zorig=0., xorig=0., transposed=False):
    """the transfer plan of `device` from grid src = (nz, nx, dz, dx) to grid dst, created on first use and kept for the process;
    transposed: the plan from dst to src that applies the exact transpose of that transfer"""
    key = (int(device),) + tuple(int(v) for v in src[:2]) + tuple(float(v) for v in src[2:]) + tuple(int(v) for v in dst[:2]) + tuple(float(v) for v in dst[2:])
    if transposed:
        key += ('T',)
    with _PLANS_MU:
        plan = _PLANS.get(key)
        if plan is None:
            lib = _lib.load()
            _lib.require_gpu()
            plan = (lib.helm_regrid_create_t if transposed else lib.helm_regrid_create)(int(device), int(src[0]), int(src[1]), float(src[2]), float(src[3]),
                                          int(dst[0]), int(dst[1]), float(dst[2]), float(dst[3]), float(zorig), float(xorig))
            if not plan:
                msg = _lib.last_error()
                if transposed and 'no transposed plan' in msg:
                    raise NotImplementedError(msg)
                raise _lib.HelmError(-1, msg)
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


def regrid_axis_t(n_in, h_in, n_out, h_out):
    """the transpose of regrid_axis for the same arguments, as (start[n_in], taps[n_in, WT]) (host only): row j holds the forward taps of the
    outputs start[j] .. start[j] + WT - 1 at input node j.  NotImplementedError when WT would exceed 64 (an up-sampling axis)"""
    lib = _lib.load()
    WT = lib.helm_regrid_axis_t(int(n_in), float(h_in), int(n_out), float(h_out), None, None, 0)
    if WT == -4:
        raise NotImplementedError(_lib.last_error())
    _lib.check(WT)
    start = np.zeros(int(n_in), dtype=np.int32)
    taps = np.zeros((int(n_in), WT), dtype=np.float64)
    _lib.check(lib.helm_regrid_axis_t(int(n_in), float(h_in), int(n_out), float(h_out), _lib.ptr(start), _lib.ptr(taps), taps.size))
    return start, taps


def _axis_csr(n_in, h_in, n_out, h_out):
    'the 1-D transfer of regrid_axis as an (n_out, n_in) CSR (zero taps of a window dropped)'
    import scipy.sparse as sp
    start, taps = regrid_axis(n_in, h_in, n_out, h_out)
    W = taps.shape[1]
    cols = (start[:, None] + np.arange(W)[None, :]).ravel()
    rows = np.repeat(np.arange(int(n_out)), W)
    m = sp.csr_matrix((taps.ravel(), (rows, cols)), shape=(int(n_out), int(n_in)))
    m.eliminate_zeros()
    return m


class BaseGridInterpolator(BaseModelDependent, BaseSCCache):
    """Geometry of a transfer between the native grid of a config and the grid coarsened by `scale` (interpolation.py:12-177)."""

    initMap = {
        #   key            required  rename        cast
        'scale':          (True,     None,         np.float64),
        'eCons':          (False,    '_eCons',     bool),
        'hostTransfer':   (False,    '_hostTransfer', bool),
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

    @property
    def hostTransfer(self):
        return getattr(self, '_hostTransfer', False)

    @property
    def matrix(self):
        """the forward transfer as a scipy CSR of shape (N_target, N_native): the Kronecker product of the two regrid_axis windows times the
        gain -- the taps the device applies, built on the host (no GPU needed) once per interpolator"""
        if '_matrix' not in self.__dict__:
            import scipy.sparse as sp
            if self.identity:
                self._matrix = sp.identity(self.shape[0], dtype=np.float64, format='csr')
            else:
                src, dst = self._grids()
                m = sp.kron(_axis_csr(src[0], src[2], dst[0], dst[2]), _axis_csr(src[1], src[3], dst[1], dst[3]), format='csr')
                self._matrix = m * float(self.gain) if self.gain != 1. else m
        return self._matrix

    @property
    def adjoint(self):
        'the exact transpose of this transfer (an object of shape (N_native, N_target)); `.T` is not that: it interpolates back'
        if '_adjoint' not in self.__dict__:
            self._adjoint = SplineGridAdjoint(self)
        return self._adjoint

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
        if self.hostTransfer:
            return self.matrix @ rhs
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


class SplineGridAdjoint(object):
    """The exact transpose of a SplineGridInterpolator `ds` (`ds.adjoint`): shape (N_native, N_target), the forward's gain carried along.
    `* g`: host arrays of shape (N_target,) or (N_target, k), real or complex -- run by the transposed plan of libhelm, or as
    `ds.matrix.T @ g` without a GPU or under `hostTransfer=True`; `apply_device`: device buffers, the signature of
    SplineGridInterpolator.apply_device (mul on the native grid).  The adjoint of an identity transfer is the identity and needs no plan."""

    def __init__(self, forward):
        self.adjoint = forward

    @property
    def shape(self):
        return self.adjoint.shape[::-1]

    @property
    def identity(self):
        return self.adjoint.identity

    @property
    def gain(self):
        return self.adjoint.gain

    @property
    def device(self):
        return self.adjoint.device

    def plan(self, device):
        fw = self.adjoint
        src, dst = fw._grids()
        return regrid_plan(device, src, dst, fw.zorig, fw.xorig, transposed=True)

    def __mul__(self, rhs):
        if self.identity:
            return rhs
        if hasattr(rhs, 'toarray'):
            rhs = rhs.toarray()
        rhs = np.asarray(rhs)
        if rhs.ndim > 2:
            raise NotImplementedError('%s does not support %dD inputs' % (self.__class__.__name__, rhs.ndim))
        nout, nin = self.shape
        if rhs.shape[0] != nin:
            raise ValueError('%s: input has %d rows, the grid %d points' % (self.__class__.__name__, rhs.shape[0], nin))
        if self.adjoint.hostTransfer or not _lib.gpu_usable():
            self._requireWindows()
            return self.adjoint.matrix.T @ rhs
        real = not np.iscomplexobj(rhs)
        k = 1 if rhs.ndim == 1 else rhs.shape[1]
        src = np.ascontiguousarray(rhs, dtype=np.complex128)
        out = np.empty((nout,) if rhs.ndim == 1 else (nout, k), dtype=np.complex128)
        if k:
            lib = _lib.load()
            _lib.check(lib.helm_regrid_apply(self.plan(self.device), k, src.ctypes.data_as(ctypes.c_void_p), 1, k,
                                             out.ctypes.data_as(ctypes.c_void_p), 1, k, float(self.gain), 0., 0., None))
        return out.real.copy() if real else out

    def __call__(self, value):
        return self * value

    def _requireWindows(self):
        'what the device plan refuses the host route refuses too: NotImplementedError where a transposed window of either axis would exceed 64 taps (up-sampling)'
        if '_windowsOk' not in self.__dict__:
            src, dst = self.adjoint._grids()
            regrid_axis_t(src[0], src[2], dst[0], dst[2])
            regrid_axis_t(src[1], src[3], dst[1], dst[3])
            self._windowsOk = True

    def apply_device(self, src, dst, k=None, op=None, gain=1., beta=0., mul=None, layout='kN', device=None):
        """dst = beta dst + mul (.) (gain' T^T src) for k complex128 fields held on the device: SplineGridInterpolator.apply_device with the
        grids' roles exchanged (src on the target grid, dst and mul on the native one), gain' = gain times the forward's eCons factor."""
        fw = self.adjoint
        if self.identity:
            return fw.apply_device(src, dst, k=k, op=op, gain=gain, beta=beta, mul=mul, layout=layout, device=device)

        def addr(x):
            return None if x is None else (int(x.data_ptr()) if hasattr(x, 'data_ptr') else int(x))
        if k is None:
            k = 1 if src.dim() == 1 else (src.shape[0] if layout == 'kN' else src.shape[1])
        if device is None:
            device = src.device.index if hasattr(src, 'device') else self.device
        nout, nin = self.shape
        ifs, ies = (nin, 1) if layout == 'kN' else (1, k)
        ofs, oes = (nout, 1) if layout == 'kN' else (1, k)
        handle = getattr(op, 'handle', op)
        g = complex(gain) * self.gain
        lib = _lib.load()
        _lib.check(lib.helm_regrid_apply_device(self.plan(device), handle, int(k), addr(src), ifs, ies, addr(dst), ofs, oes,
                                                g.real, g.imag, float(beta), addr(mul)), handle)
        return dst
