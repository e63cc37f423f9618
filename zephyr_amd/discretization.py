"""GPU-backed discretisation base classes.

Interface of zephyr/backend/discretization.py:18-169: an object built from a `systemConfig`
dict that supports `obj * rhs` -> conj(A^-1 (premul * rhs)).  The sparse LU behind the
reference's `Ainv` (external problemo.BestSolver, discretization.py:78-85) is replaced by libhelm on
the MI355X: assembly on the device, a sparse direct factorisation kept per assembled operator in 2-D
(Krylov methods in 3-D and as fallback), the stencil kernel checking the true residual.
"""
import copy
import ctypes
import os
import numpy as np
import scipy.sparse as sp

from . import _lib
from .base import BaseModelDependent
from .config import BaseSCCache


def default_device():
    for key in ('HELM_DEVICE', 'LOCAL_RANK'):
        if key in os.environ:
            try:
                return int(os.environ[key])
            except ValueError:
                pass
    return 0


class BaseDiscretization(BaseModelDependent):
    """Model properties, device operator handle and the `A^-1 * rhs` action (discretization.py:18-106)."""

    VARIANT = None

    initMap = {
        #   key            required  rename        cast
        'c':              (True,     '_c',         np.complex128),
        'rho':            (False,    '_rho',       np.float64),
        'freq':           (True,     None,         np.complex128),
        'Solver':         (False,    '_Solver',    None),       # accepted for compatibility; the GPU Krylov solver is used
        'tau':            (False,    '_tau',       np.float64),
        'premul':         (False,    '_premul',    np.complex128),
        # solver controls (additions of this implementation)
        'rtol':           (False,    '_rtol',      np.float64),
        'maxit':          (False,    '_maxit',     np.int64),
        'method':         (False,    '_method',    str),
        'batch':          (False,    '_batch',     np.int64),
        'checkEvery':     (False,    '_checkEvery', np.int64),
        'device':         (False,    '_device',    np.int64),
        'transposed':     (False,    None,         bool),       # the operator is A^T: `obj * rhs` -> conj(A^-T (premul * rhs)) (helm_set_transposed)
    }

    TRANSPOSABLE = False       # classes whose device operator has a transposed assembly (the 2-D MiniZephyr family; Helm3DTransposed is a class of its own)
    _SET_TRANSPOSED = 'helm_set_transposed'      # the entry point that asks the handle for the transposed planes (Eurus: helm_set_transposed_m1)

    # ---- model properties -----------------------------------------------------------------
    @property
    def tau(self):
        'Laplace-domain damping time constant (discretization.py:33-36)'
        return getattr(self, '_tau', np.inf)

    @property
    def dampCoeff(self):
        return 1j / self.tau

    @property
    def premul(self):
        return getattr(self, '_premul', 1.)

    @property
    def c(self):
        'Complex wave velocity (discretization.py:49-55)'
        if isinstance(self._c, np.ndarray) and self._c.ndim > 0:
            return self._c
        return self._c * np.ones((self.nz, self.nx), dtype=np.complex128)

    @property
    def rho(self):
        'Bulk density; Gardner default 310 Re(c)^0.25 (discretization.py:57-72)'
        if hasattr(self, '_rho'):
            if not (isinstance(self._rho, np.ndarray) and self._rho.ndim > 0):
                return self._rho * np.ones((self.nz, self.nx), dtype=np.float64)
        else:
            self._rho = 310. * self.c.real ** 0.25
        return self._rho

    @property
    def transposed(self):
        """config key (default False): the device operator is assembled as A^T, so that `self * rhs` is conj(A^-T (premul * rhs)) -- what back-propagates a
        residual exactly when A is not symmetric (HelmBaseProblem.Jtvec(adjoint='transpose')).  The 2-D MiniZephyr family only (the 3-D operator: the class Helm3DTransposed)."""
        return bool(self.__dict__.get('_transposed', False))

    @transposed.setter
    def transposed(self, value):
        if value and not self.TRANSPOSABLE:
            raise NotImplementedError('%s has no transposed operator: helm_set_transposed serves 2-D MiniZephyr handles (not Eurus, not the 3-D operator)'
                                      % (type(self).__name__,))
        self._transposed = bool(value)

    # ---- solver controls -------------------------------------------------------------------
    @property
    def rtol(self):
        return float(getattr(self, '_rtol', 1e-10))

    @property
    def maxit(self):
        return int(getattr(self, '_maxit', 200000))

    @property
    def method(self):
        return getattr(self, '_method', 'auto')

    @property
    def device(self):
        return int(getattr(self, '_device', default_device()))

    # ---- device operator --------------------------------------------------------------------
    def _model_arrays(self):
        'returns (c, rho, theta, eps, delta) host arrays (None where not applicable)'
        dims = (int(self.nz), int(self.nx))
        # no density given: the library evaluates the Gardner default on the device (same formula as the `rho` property)
        rho = _lib.f64(self.rho.reshape(dims)) if hasattr(self, '_rho') else None
        return _lib.c128(self.c.reshape(dims)), rho, None, None, None

    def _assemble_args(self):
        'returns (ky, cPML)'
        return 0.0, 0.0

    @property
    def handle(self):
        'The assembled device operator (lazily created; replaces the LU `Ainv`, discretization.py:78-85)'
        if getattr(self, '_handle', None) is None:
            lib = _lib.load()
            _lib.require_gpu()
            fs = (ctypes.c_int * 4)(*[1 if f else 0 for f in self.freeSurf])
            ky, cpml = self._assemble_args()
            h = lib.helm_create(self.device, self.VARIANT, int(self.nz), int(self.nx), float(self.dx), float(self.dz),
                                int(self.nPML), fs)
            if not h:
                raise _lib.HelmError(-2, _lib.last_error(None))
            try:
                c, rho, theta, eps, delta = self._model_arrays()
                _lib.check(lib.helm_set_model(h, _lib.ptr(c), _lib.ptr(rho), _lib.ptr(theta), _lib.ptr(eps), _lib.ptr(delta)), h)
                if self.transposed:
                    _lib.check(getattr(lib, self._SET_TRANSPOSED)(h, 1), h)
                self._configureHandle(lib, h)
                f = complex(self.freq)
                _lib.check(lib.helm_assemble(h, f.real, f.imag, float(self.tau), float(ky), float(cpml)), h)
            except Exception:
                lib.helm_destroy(h)
                raise
            self._handle = h
        return self._handle

    def _configureHandle(self, lib, h):
        'what a class sets on a fresh handle before its first assembly (Eurus: the opt-in of its derivative routes)'

    @property
    def Ainv(self):
        return self.handle

    def prefactor(self, nrhs=None):
        """Start the factorisation the next solve on this operator needs and return at once (helm_prefactor): the launches go
        to a high-priority stream of the handle and run beside the solves of other operators.  The reference builds its LU
        lazily inside the first `Disc * rhs` (discretization.py:78-85); its dispatcher overlaps frequencies with a process
        pool (distributors.py:161-168) -- `zephyr_amd.dispatch` does it with this call.  3-D operators build their multigrid
        hierarchy here, in the calling thread (helm_prefactor_n: `nrhs` = right-hand sides the solve will bring)."""
        m = str(self.method).lower()
        if m in ('auto', 'direct') or (m == 'mg' and getattr(self, 'heavyPrepare', False)):
            lib = _lib.load()
            lib.helm_set_tolerance_hint(self.handle, float(self.rtol))      # the factors are conditioned for the tolerance the solves will ask for
            _lib.check(lib.helm_prefactor_n(self.handle, int(nrhs or 0)), self.handle)

    def reserve(self, nrhs, rows=None, concurrent=1):
        """Bring into being what `concurrent` host-array solves of `nrhs` right-hand sides on this operator's GPU take from the
        library's pools (helm_reserve) -- called by the dispatcher before it starts its workers."""
        if str(self.method).lower() in ('auto', 'direct'):
            _lib.load().helm_reserve(self.handle, int(nrhs), int(rows if rows else self.nz * self.nx), int(concurrent))

    @Ainv.deleter
    def Ainv(self):
        h = getattr(self, '_handle', None)
        if h is not None:
            _lib.load().helm_destroy(h)
            self._handle = None

    @property
    def factors(self):
        'True when a device operator is resident (mirrors the LU-cache flag, discretization.py:91-96)'
        return getattr(self, '_handle', None) is not None

    @factors.deleter
    def factors(self):
        del self.Ainv

    def __del__(self):
        try:
            del self.factors
        except Exception:
            pass

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_handle', None)     # device handles do not pickle; they are rebuilt lazily
        state.pop('_A', None)
        return state

    # ---- operator views -----------------------------------------------------------------------
    def diagonals(self):
        'Coefficient planes from the device: (nblocks, 9, nz, nx) complex128'
        lib = _lib.load()
        h = self.handle
        nb = lib.helm_num_blocks(h)
        out = np.empty((nb, 9, int(self.nz), int(self.nx)), dtype=np.complex128)
        _lib.check(lib.helm_get_diagonals(h, _lib.ptr(out)), h)
        return out

    def applyForward(self, x, block=0, adjoint=False):
        'A x (or A^H x) on the device for one block; x: (N,) or (N, nrhs)'
        lib = _lib.load()
        h = self.handle
        x2, onedim = self._dense_rhs(x)
        X = np.ascontiguousarray(x2.T, dtype=np.complex128)
        Y = np.empty_like(X)
        _lib.check(lib.helm_apply(h, int(block), 1 if adjoint else 0, _lib.ptr(X), _lib.ptr(Y), X.shape[0]), h)
        return Y.T[:, 0] if onedim else Y.T

    @property
    def shape(self):
        return (self.nrow, self.nrow)

    def _solve_opts(self):
        o = _lib.SolveOpts()
        o.method = _lib.METHODS[self.method.lower()]
        o.rtol = self.rtol
        o.maxit = self.maxit
        o.check_every = int(getattr(self, '_checkEvery', 0))
        o.batch = int(getattr(self, '_batch', 0))
        o.flags = 0
        return o

    def _solve(self, rhs, rows):
        """rhs: (rows, nrhs) dense complex or scipy-sparse -> (rows, nrhs) complex128, C-order like the reference's `lu.solve` result.

        Arrays cross the C ABI in the reference's own layout (HELM_NODE_MAJOR): no transposes on the host or on the device.  A sparse
        right-hand side (the surveys' source matrices) is not densified on the host -- only its triplets go to the GPU (helm_solve_coo),
        where problemo's `b.toarray()` happens.  The result array lives in pinned host memory so the copy back runs at the PCIe rate."""
        lib = _lib.load()
        h = self.handle
        nrhs = int(rhs.shape[1])
        info = (_lib.SolveInfo * nrhs)()
        opts = self._solve_opts()
        opts.flags = _lib.HELM_NODE_MAJOR
        pm = complex(self.premul)
        nbytes = int(rows) * nrhs * 16
        U = _lib.pinned_empty((int(rows), nrhs), np.complex128) if nbytes >= (1 << 20) else np.empty((int(rows), nrhs), dtype=np.complex128)
        if sp.issparse(rhs):
            coo = sp.coo_matrix(rhs)
            coo.sum_duplicates()
            row = np.ascontiguousarray(coo.row, dtype=np.int64)
            col = np.ascontiguousarray(coo.col, dtype=np.int32)
            val = np.ascontiguousarray(coo.data, dtype=np.complex128)
            rc = lib.helm_solve_coo(h, _lib.ptr(row), _lib.ptr(col), _lib.ptr(val), int(coo.nnz), _lib.ptr(U), nrhs, int(rows),
                                    pm.real, pm.imag, ctypes.byref(opts), info)
        else:
            R = np.ascontiguousarray(rhs, dtype=np.complex128)
            rc = lib.helm_solve(h, _lib.ptr(R), _lib.ptr(U), nrhs, int(rows), pm.real, pm.imag, ctypes.byref(opts), info)
        _lib.check(rc, h)
        self.lastInfo = [dict(iterations=i.iterations, status=i.status, restarts=i.restarts, method=i.method,
                              relres=i.relres) for i in info]
        if rc > 0:
            worst = max(i.relres for i in info)
            raise ArithmeticError('%d of %d right-hand sides did not reach rtol=%g (worst relative residual %.3e, maxit=%d)'
                                  % (rc, nrhs, self.rtol, worst, self.maxit))
        return U

    def solveDevice(self, d_rhs, d_u, nrhs, rows=None, layout='rhs', support=None):
        '''Solve with right-hand sides and wavefields already resident in HBM.

        d_rhs / d_u: device pointers (ints) to complex128 buffers: layout 'rhs' = [nrhs][rows], each right-hand side contiguous;
        layout 'node' = [rows][nrhs], the reference's (N, nrhs) C-order arrays (no transposes inside the direct path).
        support: what rhsSupportFromSparse made of the sparse matrix these right-hand sides were filled from (layout 'node' only; the caller's
        guarantee that they are zero elsewhere; HELM_ND_SUPPORT_CHECK=1 verifies it).
        Returns the per-RHS info list; raises if a right-hand side misses the tolerance.'''
        lib = _lib.load()
        h = self.handle
        rows = int(self.nrow if rows is None else rows)
        if support is not None and layout == 'node':
            _lib.check(lib.helm_set_rhs_support(h, ctypes.c_void_p(support.data_ptr()), rows, int(nrhs)), h)
        info = (_lib.SolveInfo * nrhs)()
        opts = self._solve_opts()
        opts.flags = _lib.HELM_NODE_MAJOR if layout == 'node' else 0
        pm = complex(self.premul)
        rc = lib.helm_solve_device(h, ctypes.c_void_p(d_rhs), ctypes.c_void_p(d_u), int(nrhs), rows, pm.real, pm.imag,
                                   ctypes.byref(opts), info)
        _lib.check(rc, h)
        self.lastInfo = [dict(iterations=i.iterations, status=i.status, restarts=i.restarts, method=i.method,
                              relres=i.relres) for i in info]
        if rc > 0:
            raise ArithmeticError('%d of %d right-hand sides did not reach rtol=%g' % (rc, nrhs, self.rtol))
        return self.lastInfo

    def imagingAccumulateDevice(self, d_uf, d_ub, nsrc, d_scaler, d_g, d_exp=None):
        """G += scaler * sum_s UF[s] * UB[s] on the device (zero-lag imaging condition, problem.py:152); all device pointers.  d_exp given: UF is a
        complex64 store with those column exponents (packDevice)."""
        lib = _lib.load()
        if d_exp is not None:
            _lib.check(lib.helm_imaging_accumulate_c64_device(self.handle, ctypes.c_void_p(d_uf), ctypes.c_void_p(d_exp), ctypes.c_void_p(d_ub), int(nsrc),
                                                              ctypes.c_void_p(d_scaler), ctypes.c_void_p(d_g)), self.handle)
            return
        _lib.check(lib.helm_imaging_accumulate_device(self.handle, ctypes.c_void_p(d_uf), ctypes.c_void_p(d_ub), int(nsrc),
                                                      ctypes.c_void_p(d_scaler), ctypes.c_void_p(d_g)), self.handle)

    def energyAccumulateDevice(self, d_u, nsrc, alpha, d_w, d_e, d_exp=None, rows=None):
        """E += alpha * W * sum_s |U[s]|^2 on the device (the illumination of HelmBaseProblem.illumination); d_u [nsrc][rows] complex128, d_e and d_w
        (None: no weight) nrow float64, alpha >= 0.  d_exp given: d_u is a complex64 store with those column exponents (packDevice).  All device
        pointers; returns when E is complete."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        w = None if d_w is None else ctypes.c_void_p(d_w)
        if d_exp is not None:
            _lib.check(lib.helm_energy_accumulate_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, float(alpha), w,
                                                             ctypes.c_void_p(d_e)), self.handle)
            return
        _lib.check(lib.helm_energy_accumulate_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, float(alpha), w, ctypes.c_void_p(d_e)), self.handle)

    def virtualSourcesDevice(self, d_u, nsrc, d_w, d_r, d_exp=None, rows=None):
        """R[s] = conj(W (.) U[s]) on the device, the right-hand sides of HelmBaseProblem.JvecBorn: d_u [nsrc][rows] complex128 (d_exp given: a complex64 store
        with those column exponents), d_w nrow complex128, d_r [nsrc][rows] complex128.  All device pointers; returns when R is complete."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        if d_exp is not None:
            _lib.check(lib.helm_virtual_sources_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, ctypes.c_void_p(d_w),
                                                           ctypes.c_void_p(d_r), rows), self.handle)
            return
        _lib.check(lib.helm_virtual_sources_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_w), ctypes.c_void_p(d_r), rows), self.handle)

    def virtualSourcesOpDevice(self, d_u, nsrc, d_w, coef, d_r, conj=True, d_exp=None, rows=None):
        """R[s] = coef mask_int (.) M0(W (.) conj-or-not(U[s])) on the device, the right-hand sides of JvecBorn(linearisation='operator'): the mass stencil of
        the assembled 2-D MiniZephyr operator applied to W (.) U[s], boundary lines zeroed.  Arguments as for virtualSourcesDevice; coef a complex number."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        coef = complex(coef)
        if d_exp is not None:
            _lib.check(lib.helm_virtual_sources_op_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, ctypes.c_void_p(d_w),
                                                              coef.real, coef.imag, 1 if conj else 0, ctypes.c_void_p(d_r), rows), self.handle)
            return
        _lib.check(lib.helm_virtual_sources_op_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_w), coef.real, coef.imag,
                                                      1 if conj else 0, ctypes.c_void_p(d_r), rows), self.handle)

    def imagingOpAccumulateDevice(self, d_uf, d_ub, nsrc, d_w, d_g, d_exp=None, rows=None):
        """G += W (.) sum_s UF[s] (.) M0(mask_int (.) UB[s]) on the device, the imaging sum of Jtvec(linearisation='operator').  Arguments as for
        imagingAccumulateDevice, both fields [nsrc][rows]."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        if d_exp is not None:
            _lib.check(lib.helm_imaging_op_accumulate_c64_device(self.handle, ctypes.c_void_p(d_uf), ctypes.c_void_p(d_exp), rows, ctypes.c_void_p(d_ub), rows,
                                                                 int(nsrc), ctypes.c_void_p(d_w), ctypes.c_void_p(d_g)), self.handle)
            return
        _lib.check(lib.helm_imaging_op_accumulate_device(self.handle, ctypes.c_void_p(d_uf), rows, ctypes.c_void_p(d_ub), rows, int(nsrc),
                                                         ctypes.c_void_p(d_w), ctypes.c_void_p(d_g)), self.handle)

    def buoyancyPlanesDevice(self, d_db, d_c):
        """dC = L[db] on the device: the nine planes (9 nrow complex128 at d_c, boundary rows zero) of d A / d b along the buoyancy perturbation db (nrow
        float64 at d_db) for the operator this object holds -- frechet.buoyancyPlanes.  2-D MiniZephyr operators."""
        _lib.check(_lib.load().helm_buoyancy_planes_device(self.handle, ctypes.c_void_p(d_db), ctypes.c_void_p(d_c)), self.handle)

    def stencilSourcesDevice(self, d_u, nsrc, d_c, coef, d_r, conj=True, d_exp=None, rows=None):
        """R[s] = coef sum_k C_k (.) shift_k(conj-or-not(U[s])) on the device, the right-hand sides of JvecBorn(linearisation='operator', parameter='rho'):
        d_c the nine planes of buoyancyPlanesDevice; the other arguments as for virtualSourcesOpDevice."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        coef = complex(coef)
        if d_exp is not None:
            _lib.check(lib.helm_stencil_sources_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, ctypes.c_void_p(d_c),
                                                           coef.real, coef.imag, 1 if conj else 0, ctypes.c_void_p(d_r), rows), self.handle)
            return
        _lib.check(lib.helm_stencil_sources_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_c), coef.real, coef.imag,
                                                   1 if conj else 0, ctypes.c_void_p(d_r), rows), self.handle)

    def lagImagingAccumulateDevice(self, d_uf, d_ub, nsrc, d_p, d_exp=None, rows=None):
        """P_k += sum_s UB[s] (.) shift_k(UF[s]) on the device for the nine lags k, interior cells only: the per-source half of
        Jtvec(linearisation='operator', parameter='rho').  d_p: 9 nrow complex128; the fields as for imagingOpAccumulateDevice."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        if d_exp is not None:
            _lib.check(lib.helm_lag_imaging_accumulate_c64_device(self.handle, ctypes.c_void_p(d_uf), ctypes.c_void_p(d_exp), rows, ctypes.c_void_p(d_ub), rows,
                                                                  int(nsrc), ctypes.c_void_p(d_p)), self.handle)
            return
        _lib.check(lib.helm_lag_imaging_accumulate_device(self.handle, ctypes.c_void_p(d_uf), rows, ctypes.c_void_p(d_ub), rows, int(nsrc),
                                                          ctypes.c_void_p(d_p)), self.handle)

    def buoyancyAdjointDevice(self, d_p, w, d_g, conj=False):
        "G += w L^T P (conj: conj(L)^T P) on the device, frechet.buoyancyAdjoint: d_p 9 nrow complex128, d_g nrow complex128, w a complex number"
        w = complex(w)
        _lib.check(_lib.load().helm_buoyancy_adjoint_device(self.handle, ctypes.c_void_p(d_p), w.real, w.imag, 1 if conj else 0, ctypes.c_void_p(d_g)), self.handle)

    def velocityPlanesDevice(self, d_dc, d_db, d_c):
        """dC = V[dc] + L[db] on the device, frechet.velocityPlanes: the nine planes (9 nrow complex128 at d_c, boundary rows zero) of d A / d c along the
        velocity perturbation dc (nrow float64 at d_dc) at the density this operator assembled with; d_db (nrow float64, or None) the buoyancy perturbation that
        goes with dc where the density follows c.  2-D MiniZephyr operators."""
        db = None if d_db is None else ctypes.c_void_p(d_db)
        _lib.check(_lib.load().helm_velocity_planes_device(self.handle, ctypes.c_void_p(d_dc), db, ctypes.c_void_p(d_c)), self.handle)

    def velocityAdjointDevice(self, d_p, w, d_g, conj=False):
        "G += w V^T P (conj: conj(V)^T P) on the device, frechet.velocityAdjoint: d_p 9 nrow complex128, d_g nrow complex128, w a complex number"
        w = complex(w)
        _lib.check(_lib.load().helm_velocity_adjoint_device(self.handle, ctypes.c_void_p(d_p), w.real, w.imag, 1 if conj else 0, ctypes.c_void_p(d_g)), self.handle)

    def velocityCurvatureDevice(self, d_p, d_v, w, d_g, conj=False, stretch=True):
        """G += w v (.) (the second derivative of the operator along e_j contracted with P) on the device, frechet.velocityCurvature: d_p 9 nrow complex128, d_v nrow
        float64 (the perturbation), d_g nrow complex128, w a complex number; conj: the conjugated coefficients; stretch False: the mass term alone"""
        w = complex(w)
        _lib.check(_lib.load().helm_velocity_curvature_device(self.handle, ctypes.c_void_p(d_p), ctypes.c_void_p(d_v), w.real, w.imag, 1 if conj else 0,
                                                              1 if stretch else 0, ctypes.c_void_p(d_g)), self.handle)

    def massPlanesDevice(self, d_dc, d_c):
        "dC = the mass term of velocityPlanesDevice alone on the device, frechet.massPlanes (linearisation='operator'): d_dc nrow float64, d_c 9 nrow complex128"
        _lib.check(_lib.load().helm_mass_planes_device(self.handle, ctypes.c_void_p(d_dc), ctypes.c_void_p(d_c)), self.handle)

    def massAdjointDevice(self, d_p, w, d_g, conj=False):
        "G += w M^T P (conj: conj(M)^T P) on the device, M the map of massPlanesDevice: frechet.velocityAdjoint(stretch=False); arguments as velocityAdjointDevice"
        w = complex(w)
        _lib.check(_lib.load().helm_mass_adjoint_device(self.handle, ctypes.c_void_p(d_p), w.real, w.imag, 1 if conj else 0, ctypes.c_void_p(d_g)), self.handle)

    def velocityAdjointBuoyancyDevice(self, d_p, d_b, w, d_g, conj=False, stretch=True):
        """G += w (V at the buoyancy B)^T P on the device, frechet.mixedAdjointC: velocityAdjointDevice (stretch False: massAdjointDevice) with the field d_b (nrow
        float64, any sign) in the place of 1 / rho -- the transpose in the velocity of the mixed (c, b) second derivative"""
        w = complex(w)
        _lib.check(_lib.load().helm_velocity_adjoint_b_device(self.handle, ctypes.c_void_p(d_p), ctypes.c_void_p(d_b), w.real, w.imag, 1 if conj else 0,
                                                              1 if stretch else 0, ctypes.c_void_p(d_g)), self.handle)

    def mixedAdjointDevice(self, d_p, d_v, w, d_g, conj=False, stretch=True):
        """G += w M_b^T[v] P on the device, frechet.mixedAdjointB: the transpose in the buoyancy of the mixed (c, b) second derivative along the velocity
        perturbation d_v (nrow float64); d_p 9 nrow complex128, d_g nrow complex128, w a complex number; stretch False: the mass term alone"""
        w = complex(w)
        _lib.check(_lib.load().helm_mixed_adjoint_device(self.handle, ctypes.c_void_p(d_p), ctypes.c_void_p(d_v), w.real, w.imag, 1 if conj else 0,
                                                         1 if stretch else 0, ctypes.c_void_p(d_g)), self.handle)

    def viscoPerturbationDevice(self, d_q, lam, d_vc, d_vq, d_dcz):
        """dc~ = gamma vc + chi vQ on the device, frechet.viscoChain at the complex velocity this operator holds: d_q nrow float64 (Q, inf allowed), lam the
        dispersion scalar of its frequency, d_vc / d_vq nrow float64 (either may be None), d_dcz nrow complex128"""
        vc, vq = (None if p is None else ctypes.c_void_p(p) for p in (d_vc, d_vq))
        _lib.check(_lib.load().helm_visco_perturbation_device(self.handle, ctypes.c_void_p(d_q), float(lam), vc, vq, ctypes.c_void_p(d_dcz)), self.handle)

    def velocityPlanesComplexDevice(self, d_dcz, d_c):
        "dC = V[dc~] on the device, frechet.velocityPlanes with a complex perturbation: d_dcz nrow complex128 (viscoPerturbationDevice), d_c 9 nrow complex128"
        _lib.check(_lib.load().helm_velocity_planes_z_device(self.handle, ctypes.c_void_p(d_dcz), ctypes.c_void_p(d_c)), self.handle)

    def viscoChainAdjointDevice(self, d_q, lam, d_t, d_gc, d_gq, conj=False):
        """Gc += gamma (.) T, GQ += chi (.) T (conj: the conjugated chain) on the device, the transpose of viscoPerturbationDevice: d_t nrow complex128, the complex
        cell gradient of one item; d_gc / d_gq nrow complex128 (either may be None)"""
        gc, gq = (None if p is None else ctypes.c_void_p(p) for p in (d_gc, d_gq))
        _lib.check(_lib.load().helm_visco_chain_adjoint_device(self.handle, ctypes.c_void_p(d_q), float(lam), ctypes.c_void_p(d_t), 1 if conj else 0, gc, gq), self.handle)

    def stencilSourcesTransposedDevice(self, d_u, nsrc, d_c, coef, d_r, conj=False, d_exp=None, rows=None, accumulate=False):
        """R[s] = coef (dC)^T U[s] (conj: (dC)^H U[s]) on the device, frechet.applyPlanesTransposed: d_c the nine planes of velocityPlanesDevice or
        buoyancyPlanesDevice, read at the neighbouring cell -- the transposed set is never formed; the other arguments as for stencilSourcesDevice, but conj
        conjugates the planes, not the columns.  accumulate: R[s] += the CONJUGATE of that value instead."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        coef = complex(coef)
        if d_exp is not None:
            _lib.check(lib.helm_stencil_sources_t_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, ctypes.c_void_p(d_c),
                                                             coef.real, coef.imag, 1 if conj else 0, 1 if accumulate else 0, ctypes.c_void_p(d_r), rows), self.handle)
            return
        _lib.check(lib.helm_stencil_sources_t_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_c), coef.real, coef.imag,
                                                     1 if conj else 0, 1 if accumulate else 0, ctypes.c_void_p(d_r), rows), self.handle)

    PSEUDO_HESSIAN_MODES = {'velocity': 0, 'buoyancy': 1, 'gardner': 2}

    def pseudoHessianAccumulateDevice(self, d_u, nsrc, mode, d_chain, alpha, d_w, d_h, d_exp=None, rows=None):
        """H += alpha * W * sum_s ||(d A / d p_i) u^_s||^2 on the device, frechet.pseudoHessianDiagonal on the stored columns conj(u^): d_u [nsrc][rows]
        complex128 (d_exp given: a complex64 store with those column exponents), mode 'velocity' (p = c at the density of the operator), 'buoyancy' (p = b)
        or 'gardner' (p = c with d b / d c = d_chain, nrow float64; None otherwise), d_w (None: no weight) and d_h nrow float64, alpha >= 0.  All device
        pointers; returns when H is complete.  2-D MiniZephyr operators."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        mode = self.PSEUDO_HESSIAN_MODES[mode]
        w = None if d_w is None else ctypes.c_void_p(d_w)
        ch = None if d_chain is None else ctypes.c_void_p(d_chain)
        if d_exp is not None:
            _lib.check(lib.helm_pseudo_hessian_accumulate_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, mode, ch,
                                                                     float(alpha), w, ctypes.c_void_p(d_h)), self.handle)
            return
        _lib.check(lib.helm_pseudo_hessian_accumulate_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, mode, ch, float(alpha), w, ctypes.c_void_p(d_h)),
                   self.handle)

    GAUSS_NEWTON_MODES = {'velocity': 0, 'buoyancy': 1, 'gardner': 2, 'mass': 3, 'diagonal': 4}

    def lagGramAccumulateDevice(self, d_u, nsrc, d_c, d_exp=None, rows=None):
        """C_l += sum_s U[s] (.) conj(shift_l(U[s])) on the device for the 13 lags of frechet.GRAM_LAGS, wherever the partner is inside the grid (frechet.lagGram):
        d_u [nsrc][rows] complex128 (d_exp given: a complex64 store with those column exponents), d_c 13 nrow complex128.  All device pointers; returns when C
        is complete.  2-D MiniZephyr operators."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        if d_exp is not None:
            _lib.check(lib.helm_lag_gram_accumulate_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, ctypes.c_void_p(d_c)), self.handle)
            return
        _lib.check(lib.helm_lag_gram_accumulate_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_c)), self.handle)

    def gaussNewtonDiagonalDevice(self, mode, d_chain, d_w, d_cu, d_cg, alpha, d_h):
        """H += alpha * W * Re tr(E^H Gamma E Phi) per cell on the device, frechet.gaussNewtonDiagonal: d_cu and d_cg the planes of lagGramAccumulateDevice of the
        stored columns and of the transposed solves of the receiver rows (13 nrow complex128 each), mode 'velocity', 'buoyancy', 'gardner' (d_chain nrow float64;
        None otherwise), 'mass' (the mass term alone) or 'diagonal' (W the squared weight), d_w (None: no weight) and d_h nrow float64, alpha >= 0."""
        w = None if d_w is None else ctypes.c_void_p(d_w)
        ch = None if d_chain is None else ctypes.c_void_p(d_chain)
        _lib.check(_lib.load().helm_gauss_newton_diagonal_device(self.handle, self.GAUSS_NEWTON_MODES[mode], ch, w, ctypes.c_void_p(d_cu), ctypes.c_void_p(d_cg),
                                                                 float(alpha), ctypes.c_void_p(d_h)), self.handle)

    def gaussNewtonBlocksDevice(self, stretch, d_cu, d_cg, alpha, d_h, ldh=None):
        """The three rows H_cc, H_crho, H_rhorho of the per-cell (c, rho) blocks, H[a] += alpha d_a Re tr(E^a^H Gamma E^b Phi), on the device
        (frechet.gaussNewtonBlocks): d_cu, d_cg as for gaussNewtonDiagonalDevice, stretch False: the mass term alone for E^c; d_h three rows of nrow float64, ldh
        (default nrow) apart; alpha >= 0."""
        ldh = int(self.nrow if ldh is None else ldh)
        _lib.check(_lib.load().helm_gauss_newton_blocks_device(self.handle, 1 if stretch else 0, ctypes.c_void_p(d_cu), ctypes.c_void_p(d_cg), float(alpha),
                                                               ctypes.c_void_p(d_h), ldh), self.handle)

    def pseudoHessianBlocksDevice(self, d_u, nsrc, stretch, alpha, d_h, ldh=None, d_exp=None, rows=None):
        """The same three rows for the pseudo-Hessian, H[a] += alpha d_a sum_s Re <E^a u^_s, E^b u^_s> (frechet.pseudoHessianBlocks), from the stored columns d_u as
        pseudoHessianAccumulateDevice takes them (d_exp given: the complex64 store)."""
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        ldh = int(self.nrow if ldh is None else ldh)
        if d_exp is not None:
            _lib.check(lib.helm_pseudo_hessian_blocks_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), rows, 1 if stretch else 0,
                                                                 float(alpha), ctypes.c_void_p(d_h), ldh), self.handle)
            return
        _lib.check(lib.helm_pseudo_hessian_blocks_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, 1 if stretch else 0, float(alpha), ctypes.c_void_p(d_h),
                                                         ldh), self.handle)

    def packDevice(self, d_u, nsrc, d_out, d_exp, rows=None):
        """The complex64 store of the wavefields d_u ([nsrc][rows] complex128): d_out [nsrc][rows] complex64 values x * 2^-e_s, d_exp the nsrc int32 column
        exponents e_s (fieldstore.pack_reference states the format).  All device pointers; returns when both are complete."""
        rows = int(self.nrow if rows is None else rows)
        _lib.check(_lib.load().helm_pack_c64_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), rows, ctypes.c_void_p(d_out), ctypes.c_void_p(d_exp)), self.handle)

    def rhsFromSparseDevice(self, q, d_rhs, layout='rhs'):
        '''Fill the device buffer d_rhs ([ncols][nrow] complex128; layout 'node': [nrow][ncols]) from the scipy-sparse right-hand-side
        matrix q (nrow x ncols) without densifying it on the host: only the COO triplets cross PCIe.'''
        import torch
        lib = _lib.load()
        if isinstance(q, tuple):                 # (rows, cols, values, shape): triplets the caller has made itself, no two of them at the same place
            r_, c_, v_, shape = q
            nnz = int(len(v_))
        else:
            # duplicates are summed where they can exist at all: a CSR / CSC matrix in canonical form has none, and its COO view needs no sort
            if sp.isspmatrix_csr(q) or sp.isspmatrix_csc(q):
                if not q.has_canonical_format:
                    q = q.copy()
                    q.sum_duplicates()
                coo = q.tocoo(copy=False)
            else:
                coo = sp.coo_matrix(q)
                coo.sum_duplicates()
            r_, c_, v_, shape, nnz = coo.row, coo.col, coo.data, coo.shape, int(coo.nnz)
        dev = torch.device('cuda', self.device)
        row = _lib.to_device(r_, dev, np.int64)
        col = _lib.to_device(c_, dev, np.int32)
        val = _lib.to_device(v_, dev, np.complex128)
        _lib.wait_torch_stream(dev)                         # (the copies of THIS thread: a device-wide synchronisation would wait for the other workers' kernels too)
        _lib.check(lib.helm_rhs_from_coo_device_layout(self.handle, ctypes.c_void_p(row.data_ptr()), ctypes.c_void_p(col.data_ptr()),
                                                       ctypes.c_void_p(val.data_ptr()), nnz, ctypes.c_void_p(d_rhs), int(shape[1]),
                                                       int(shape[0]), _lib.HELM_RHS_NODE_MAJOR if layout == 'node' else 0), self.handle)

    def rhsSupportFromSparse(self, q):
        '''The support of the scipy-sparse right-hand-side matrix q (nrow x ncols, ncols <= 512) as solveDevice(..., support=) takes it: a uint8 device
        tensor, one byte per row, bit b = block b of 64 columns has an entry in that row.  Where a source matrix is nonzero is part of the reference's
        input (scipy-sparse sources, survey.py:86-89,162-188); with it the direct path does not read the dense right-hand sides to find out.'''
        import torch
        lib = _lib.load()
        coo = sp.coo_matrix(q)
        dev = torch.device('cuda', self.device)
        row = _lib.to_device(coo.row, dev, np.int64)
        col = _lib.to_device(coo.col, dev, np.int32)
        bits = torch.zeros(((int(coo.shape[0]) + 3) // 4) * 4, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        _lib.check(lib.helm_rhs_support_from_coo(self.handle, ctypes.c_void_p(row.data_ptr()), ctypes.c_void_p(col.data_ptr()), int(coo.nnz),
                                                 ctypes.c_void_p(bits.data_ptr()), int(coo.shape[0]), int(coo.shape[1])), self.handle)
        return bits

    def sampleDevice(self, d_u, nsrc, csr_dev, d_out, d_exp=None):
        """d_out[nrec][nsrc] = R u for the CSR receiver matrix uploaded by the caller: csr_dev = (rowptr, col, val, nrec[, row_stride]) device tensors.
        row_stride (default 0: one array for every source) = nrec: source s samples row s * nrec + r of the stacked matrices of a moving array
        (survey.stackedReceivers; `rowptr` then starts at the first source of the batch).  d_exp given: d_u is a complex64 store with those column
        exponents (packDevice)."""
        rowptr, col, val, nrec = csr_dev[:4]
        stride = int(csr_dev[4]) if len(csr_dev) > 4 else 0
        lib = _lib.load()
        if d_exp is not None:
            _lib.check(lib.helm_sample_rows_c64_device(self.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), int(nsrc), int(self.nrow),
                                                       ctypes.c_void_p(rowptr.data_ptr()), ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()),
                                                       int(nrec), stride, 1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(d_out)), self.handle)
        elif stride == 0:
            _lib.check(lib.helm_sample_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), int(self.nrow), ctypes.c_void_p(rowptr.data_ptr()),
                                              ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()), int(nrec),
                                              ctypes.c_void_p(d_out)), self.handle)
        else:
            _lib.check(lib.helm_sample_rows_device(self.handle, ctypes.c_void_p(d_u), int(nsrc), int(self.nrow), ctypes.c_void_p(rowptr.data_ptr()),
                                                   ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()), int(nrec), stride,
                                                   1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(d_out)), self.handle)

    def rhsFromSamplesDevice(self, d_resid, ld, plan_dev, c0, c1, d_rhs, rows=None):
        """Fill the device buffer d_rhs ([c1 - c0][rows] complex128) with the back-sources R_s^T resid[:, s] of the sources c0 .. c1-1 of a moving receiver
        array.  d_resid: device pointer to the residual samples of one frequency, [nrec][ld] with column s - c0 that of source s; plan_dev: the survey's
        adjointPlan with its arrays as device tensors (src_ptr stays on the host).  Only the samples cross PCIe."""
        t0, t1 = int(plan_dev['src_ptr'][c0]), int(plan_dev['src_ptr'][c1])
        rows = int(self.nrow if rows is None else rows)
        _lib.check(_lib.load().helm_rhs_from_samples_device(
            self.handle, ctypes.c_void_p(d_resid), int(ld), int(plan_dev['nrec']), int(c1 - c0), int(c0),
            ctypes.c_void_p(plan_dev['tptr'].data_ptr() + 8 * t0), ctypes.c_void_p(plan_dev['tsrc'].data_ptr() + 4 * t0),
            ctypes.c_void_p(plan_dev['tcell'].data_ptr() + 8 * t0), ctypes.c_void_p(plan_dev['trec'].data_ptr()),
            ctypes.c_void_p(plan_dev['tval'].data_ptr()), t1 - t0, ctypes.c_void_p(d_rhs), rows), self.handle)

    def setProfiling(self, on=True):
        'time every stencil-apply launch of subsequent solves with HIP events on the solver stream'
        _lib.check(_lib.load().helm_set_profiling(self.handle, 1 if on else 0), self.handle)

    def lastTiming(self):
        t = _lib.Timing()
        _lib.check(_lib.load().helm_last_timing(self.handle, ctypes.byref(t)), self.handle)
        return dict(solve_ms=t.solve_ms, apply_ms=t.apply_ms, apply_launches=t.apply_launches, apply_bytes=t.apply_bytes,
                    factor_ms=t.factor_ms, gemm_ms=t.gemm_ms, gemm_launches=t.gemm_launches, gemm_flops=t.gemm_flops,
                    gemm_big_ms=t.gemm_big_ms, gemm_big_launches=t.gemm_big_launches, gemm_big_flops=t.gemm_big_flops,
                    gemm_bytes=t.gemm_bytes, gemm_sol_ms=t.gemm_sol_ms)

    @staticmethod
    def _dense_rhs(rhs):
        if sp.issparse(rhs):
            rhs = rhs.toarray()
        rhs = np.asarray(rhs, dtype=np.complex128)
        onedim = rhs.ndim == 1
        if onedim:
            rhs = rhs.reshape((-1, 1))
        return rhs, onedim

    @staticmethod
    def _as_rhs(rhs):
        'like _dense_rhs, but a scipy-sparse right-hand side stays sparse (it is expanded on the GPU)'
        if sp.issparse(rhs):
            return rhs, False
        return BaseDiscretization._dense_rhs(rhs)

    def __mul__(self, rhs):
        'conj(A^-1 (premul * rhs))  (discretization.py:101-103)'
        rhs, onedim = self._as_rhs(rhs)
        if rhs.shape[0] != self.nrow:
            raise ValueError('dimension mismatch')
        u = self._solve(rhs, self.nrow)
        return u[:, 0] if onedim else u

    def __call__(self, value):
        return self * value


def prefactor_many(ops):
    """Start the factorisations the next solves on `ops` need in the SAME launches and return at once (helm_prefactor_many): operators of one grid on one GPU,
    at most four; the latency-bound top of the elimination tree is then walked once for all of them.  Every operator's factors are bit for bit what
    `op.prefactor()` would have made; operators the library cannot take together are prefactored one by one.  The reference's dispatcher overlaps
    frequencies with a process pool (distributors.py:161-168) -- `zephyr_amd.dispatch` groups its prepare step around this call."""
    ops = [op for op in ops if op is not None]
    if not ops:
        return
    direct = [op for op in ops if getattr(type(op), 'VARIANT', None) in (_lib.HELM_MINIZEPHYR, _lib.HELM_EURUS) and str(getattr(op, 'method', '')).lower() in ('auto', 'direct')]
    for op in ops:
        if op not in direct and hasattr(op, 'prefactor'):
            op.prefactor()
    lib = _lib.load()
    for i in range(0, len(direct), 4):
        part = direct[i:i + 4]
        for op in part:
            lib.helm_set_tolerance_hint(op.handle, float(op.rtol))       # the factors are conditioned for the tolerance the solves will ask for
        hs = (ctypes.c_void_p * len(part))(*[op.handle for op in part])
        _lib.check(lib.helm_prefactor_many(hs, len(part)), part[0].handle)


class DiscretizationWrapper(BaseSCCache):
    """Composite of sub-problems built from per-sub-problem config updates (discretization.py:109-169)."""

    initMap = {
        'Disc':           (True,     None,         None),
        'scaleTerm':      (False,    '_scaleTerm', np.complex128),
    }

    maskKeys = {'scaleTerm'}
    cacheItems = ['_subProblems']

    @property
    def scaleTerm(self):
        return getattr(self, '_scaleTerm', 1.)

    @property
    def _spConfigs(self):
        updates = list(self.spUpdates)
        base = copy.copy(self.systemConfig)
        # one complex128 copy of the velocity model for ALL sub-problems (read-only, so that config.cast_value hands it on as it is): every Disc used to make its
        # own -- 0.25 ms per frequency at 512^2, 1.2 ms at 1024^2, in the calling thread before anything reaches the GPU
        c = base.get('c')
        if isinstance(c, np.ndarray) and c.ndim > 0 and not any('c' in u for u in updates):
            shared = np.array(c, dtype=np.complex128)
            shared.setflags(write=False)
            base['c'] = shared

        def merged(update):
            cfg = copy.copy(base)
            cfg.update(update)
            return cfg
        return (merged(update) for update in updates)

    @property
    def subProblems(self):
        if getattr(self, '_subProblems', None) is None:
            self._subProblems = [self.Disc(cfg) for cfg in self._spConfigs]
        return self._subProblems

    @property
    def factors(self):
        subs = getattr(self, '_subProblems', None)
        return subs is not None and any(sub.factors for sub in subs)

    @factors.deleter
    def factors(self):
        subs = getattr(self, '_subProblems', None)
        if subs is not None:
            for sub in subs:
                del sub.factors

    @property
    def spUpdates(self):
        raise NotImplementedError

    def __mul__(self, rhs):
        raise NotImplementedError
