"""Eurus / EurusHD on the GPU (interface of zephyr/backend/eurus.py:14-552)."""
import ctypes

import numpy as np
from . import _lib
from .base import BaseAnisotropic
from .discretization import BaseDiscretization
from .sparse import eurus_block_matrix


class Eurus(BaseDiscretization, BaseAnisotropic):
    """TTI mixed-grid 9-point operator (Operto 2009), 2N x 2N two-field system; the assembly
    formulas of eurus.py:28-485 run in the HIP kernel `k_assemble_eurus`.

    Solves are available whenever eps == delta (isotropic and elliptical media): then M3 == 0
    and the system is block-triangular, u = M1^-1 (q1 - M2 M4^-1 q2).

    Config key eurusDerivatives=True (opt-in, eps == delta): `transposed=True` is accepted and the handle holds M1^T (helm_set_transposed_m1), and the
    methods the derivative pipelines call run the maps of M1 (csrc/survey_eurus.hip).  Without the key everything is as it was.
    """

    VARIANT = _lib.HELM_EURUS

    initMap = {
        'nPML':           (False,    '_nPML',      np.int64),
        'freq':           (True,     None,         np.complex128),
        'mord':           (False,    '_mord',      tuple),
        'cPML':           (False,    '_cPML',      np.float64),
        'eurusDerivatives': (False,  '_eurusDerivatives', bool),      # opt-in: M1^T (helm_set_transposed_m1) and the derivative maps of M1 where eps == delta
    }

    _SET_TRANSPOSED = 'helm_set_transposed_m1'

    def __init__(self, systemConfig, *args, **kwargs):
        self._eurusDerivatives = bool(systemConfig.get('eurusDerivatives', False))      # (before `transposed` is set: its setter asks TRANSPOSABLE)
        super().__init__(systemConfig, *args, **kwargs)

    @property
    def eurusDerivatives(self):
        "config key (default False): this operator serves its transposed first block and the derivative maps of M1 -- only where eps == delta everywhere"
        return bool(self.__dict__.get('_eurusDerivatives', False))

    @property
    def elliptical(self):
        'eps == delta in every cell: the system is block-triangular and an N-row right-hand side is solved through M1 alone'
        return bool(np.all(np.asarray(self.eps) == np.asarray(self.delta)))

    @property
    def TRANSPOSABLE(self):
        return self.eurusDerivatives and self.elliptical

    def _setTransposed(self, value):
        if value and self.eurusDerivatives and not self.elliptical:
            raise NotImplementedError('%s has no transposed operator where eps != delta: the coupled 2N x 2N system [[M1, M2], [M3, M4]] has no transposed solve '
                                      '(helm_set_transposed_m1 serves M1 of a model with eps == delta)' % (type(self).__name__,))
        BaseDiscretization.transposed.fset(self, value)

    transposed = property(BaseDiscretization.transposed.fget, _setTransposed, doc=BaseDiscretization.transposed.__doc__)

    @property
    def mord(self):
        'matrix ordering; only the default (-nx, +1) is supported (eurus.py:494-498)'
        return getattr(self, '_mord', (-self.nx, +1))

    @property
    def cPML(self):
        return getattr(self, '_cPML', 1e3)

    @property
    def nPML(self):
        return getattr(self, '_nPML', 10)

    def _model_arrays(self):
        c, rho, _, _, _ = BaseDiscretization._model_arrays(self)
        aniso = any(getattr(self, n, None) is not None for n in ('_theta', '_eps', '_delta'))
        if not aniso:
            return c, rho, None, None, None
        dims = (int(self.nz), int(self.nx))
        return (c, rho, _lib.f64(self.theta.reshape(dims)), _lib.f64(self.eps.reshape(dims)),
                _lib.f64(self.delta.reshape(dims)))

    def _assemble_args(self):
        if tuple(int(v) for v in self.mord) != (-int(self.nx), 1):
            raise NotImplementedError('non-default mord re-wires the matrix (eurus.py:117-127); '
                                      'only (-nx,+1) is supported')
        return 0.0, float(self.cPML)

    @property
    def A(self):
        'The sparse 2N x 2N system matrix [[M1,M2],[M3,M4]] (eurus.py:449-463,487-492)'
        if getattr(self, '_A', None) is None:
            self._A = eurus_block_matrix(self.diagonals(), int(self.nz), int(self.nx))
        return self._A

    def diagonals(self):
        'Coefficient planes from the device: (4, 9, nz, nx) complex128; a transposed operator holds M1^T alone: (1, 9, nz, nx)'
        if not self.transposed:
            return BaseDiscretization.diagonals(self)
        out = np.empty((1, 9, int(self.nz), int(self.nx)), dtype=np.complex128)
        _lib.check(_lib.load().helm_get_block_diagonals(self.handle, 0, _lib.ptr(out)), self.handle)
        return out

    # ---- the derivative maps of M1 on the device (csrc/survey_eurus.hip; host twins frechet.eurusPlanes / eurusAdjoint / lagProducts(edges=True)) ----
    def eurusPlanesDevice(self, d_dc, d_db, d_c):
        """dC = V[dc] + L[db] on the device, frechet.eurusPlanes: the nine planes (9 nrow complex128 at d_c) of d M1 along the real perturbations dc and db
        (nrow float64 each, either may be None); edge rows carry the derivative of their centre entry."""
        dc, db = (None if p is None else ctypes.c_void_p(p) for p in (d_dc, d_db))
        _lib.check(_lib.load().helm_eurus_planes_device(self.handle, dc, db, ctypes.c_void_p(d_c)), self.handle)

    def eurusAdjointDevice(self, d_p, w, d_gc, d_gb, conj=False):
        """Gc += w V^T P, Gb += w L^T P (conj: the conjugated coefficients) on the device from one pass over P, frechet.eurusAdjoint: d_p 9 nrow complex128, d_gc /
        d_gb nrow complex128 (either may be None), w a complex number"""
        w = complex(w)
        gc, gb = (None if p is None else ctypes.c_void_p(p) for p in (d_gc, d_gb))
        _lib.check(_lib.load().helm_eurus_adjoint_device(self.handle, ctypes.c_void_p(d_p), w.real, w.imag, 1 if conj else 0, gc, gb), self.handle)

    def lagCentreEdgesAccumulateDevice(self, d_uf, d_ub, nsrc, d_p, d_exp=None, rows=None):
        """P_4 += sum_s UB[s] (.) UF[s] on the boundary cells, what lagImagingAccumulateDevice leaves out and an Eurus edge row needs (frechet.lagProducts with
        edges=True); arguments as there"""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        if d_exp is not None:
            _lib.check(lib.helm_lag_centre_edges_accumulate_c64_device(self.handle, ctypes.c_void_p(d_uf), ctypes.c_void_p(d_exp), rows, ctypes.c_void_p(d_ub), rows,
                                                                       int(nsrc), ctypes.c_void_p(d_p)), self.handle)
            return
        _lib.check(lib.helm_lag_centre_edges_accumulate_device(self.handle, ctypes.c_void_p(d_uf), rows, ctypes.c_void_p(d_ub), rows, int(nsrc),
                                                               ctypes.c_void_p(d_p)), self.handle)

    def _configureHandle(self, lib, h):
        if self.eurusDerivatives:
            _lib.check(lib.helm_set_eurus_derivatives(h, 1), h)

    # ---- what the device pipelines of the exact derivatives call (device_survey._bornPlanesFromFields, _gradientPlanesFromFields, jointGradientFromFields) ----
    # With the key, the MiniZephyr maps are replaced by those of M1: V is its mass term alone (the C-PML does not depend on the model), so the velocity and the
    # mass maps are the same.  Without the key every method is the base class's, which the library refuses for an Eurus handle as it always did.
    def velocityPlanesDevice(self, d_dc, d_db, d_c):
        if not self.eurusDerivatives:
            return BaseDiscretization.velocityPlanesDevice(self, d_dc, d_db, d_c)
        self.eurusPlanesDevice(d_dc, d_db, d_c)

    def massPlanesDevice(self, d_dc, d_c):
        if not self.eurusDerivatives:
            return BaseDiscretization.massPlanesDevice(self, d_dc, d_c)
        self.eurusPlanesDevice(d_dc, None, d_c)

    def buoyancyPlanesDevice(self, d_db, d_c):
        if not self.eurusDerivatives:
            return BaseDiscretization.buoyancyPlanesDevice(self, d_db, d_c)
        self.eurusPlanesDevice(None, d_db, d_c)

    def velocityAdjointDevice(self, d_p, w, d_g, conj=False):
        if not self.eurusDerivatives:
            return BaseDiscretization.velocityAdjointDevice(self, d_p, w, d_g, conj=conj)
        self.eurusAdjointDevice(d_p, w, d_g, None, conj=conj)

    def massAdjointDevice(self, d_p, w, d_g, conj=False):
        if not self.eurusDerivatives:
            return BaseDiscretization.massAdjointDevice(self, d_p, w, d_g, conj=conj)
        self.eurusAdjointDevice(d_p, w, d_g, None, conj=conj)

    def buoyancyAdjointDevice(self, d_p, w, d_g, conj=False):
        if not self.eurusDerivatives:
            return BaseDiscretization.buoyancyAdjointDevice(self, d_p, w, d_g, conj=conj)
        self.eurusAdjointDevice(d_p, w, None, d_g, conj=conj)

    def jointAdjointDevice(self, d_p, w, d_gc, d_gb, conj=False):
        "Gc += w V^T P and Gb += w L^T P from ONE read of P: what jointGradientFromFields calls where an operator has it"
        self.eurusAdjointDevice(d_p, w, d_gc, d_gb, conj=conj)

    def lagImagingAccumulateDevice(self, d_uf, d_ub, nsrc, d_p, d_exp=None, rows=None):
        BaseDiscretization.lagImagingAccumulateDevice(self, d_uf, d_ub, nsrc, d_p, d_exp=d_exp, rows=rows)
        if self.eurusDerivatives:
            self.lagCentreEdgesAccumulateDevice(d_uf, d_ub, nsrc, d_p, d_exp=d_exp, rows=rows)          # (an edge row keeps a centre entry that depends on the model)

    @property
    def shape(self):
        n = 2 * self.nrow
        return (n, n)

    def __mul__(self, rhs):
        'N-row rhs: zero-pad the second field and clip the result; 2N-row rhs: full result (eurus.py:512-533)'
        rhs, onedim = self._as_rhs(rhs)
        n2 = self.shape[1]
        if 2 * rhs.shape[0] == n2:
            rows = self.nrow
        elif rhs.shape[0] == n2:
            rows = n2
        else:
            raise ValueError('dimension mismatch')
        u = self._solve(rhs, rows)
        return u[:, 0] if onedim else u


class EurusHD(Eurus):
    """Eurus with half-differentiation of the source by default (eurus.py:536-552)."""

    @property
    def premul(self):
        return getattr(self, '_premul', np.sqrt(2j * np.pi * self.freq))
