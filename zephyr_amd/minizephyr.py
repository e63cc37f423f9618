"""MiniZephyr / MiniZephyrHD on the GPU (interface of zephyr/backend/minizephyr.py:27-343)."""
import ctypes
import numpy as np
import scipy.sparse as sp
from . import _lib
from functools import reduce
from .discretization import BaseDiscretization, DiscretizationWrapper, prefactor_many
from .sparse import planes_to_csr


class MiniZephyr(BaseDiscretization):
    """Isotropic 2-D (visco)acoustic 9-point operator with PML; the assembly formulas of
    minizephyr.py:40-298 run in the HIP kernel `k_assemble_mz`."""

    VARIANT = _lib.HELM_MINIZEPHYR
    TRANSPOSABLE = True

    initMap = {
        'nPML':           (False,    '_nPML',      np.int64),
        'ky':             (False,    '_ky',        np.float64),
        'mord':           (False,    '_mord',      tuple),
    }

    @property
    def mord(self):
        'matrix ordering; only the default (+nx, +1) is supported (minizephyr.py:308-312)'
        return getattr(self, '_mord', (self.nx, +1))

    @property
    def nPML(self):
        return getattr(self, '_nPML', 10)

    @property
    def ky(self):
        return getattr(self, '_ky', 0.)

    def _assemble_args(self):
        if tuple(int(v) for v in self.mord) != (int(self.nx), 1):
            raise NotImplementedError('non-default mord re-wires the matrix (minizephyr.py:147-166); '
                                      'only (+nx,+1) is supported')
        return float(self.ky), 0.0

    @property
    def A(self):
        'The sparse system matrix, rebuilt from the device coefficient planes (minizephyr.py:300-306)'
        if getattr(self, '_A', None) is None:
            self._A = planes_to_csr(self.diagonals()[0], int(self.nz), int(self.nx))
        return self._A


class MiniZephyrHD(MiniZephyr):
    """MiniZephyr with half-differentiation of the source by default (minizephyr.py:327-343)."""

    @property
    def premul(self):
        return getattr(self, '_premul', np.sqrt(2j * np.pi * self.freq))


class MiniZephyr25D(BaseDiscretization, DiscretizationWrapper):
    """2.5-D modelling by Fourier summation over cross-line wavenumbers: nky MiniZephyr sub-problems
    with `ky` and quadrature weights in `premul`, summed and scaled by e^{i pi}/(4 pi)
    (minizephyr.py:346-460).  Every sub-problem is an independent GPU operator; the reference's
    per-ky process pool (`parallel`) is accepted and ignored."""

    initMap = {
        'Disc':           (False,    '_Disc',      None),
        'nky':            (True,     '_nky',       np.int64),
        'parallel':       (False,    '_parallel',  bool),
        'cmin':           (False,    '_cmin',      np.float64),
        # additions of this implementation: where the ky sum is formed and how long the ky operators live
        'kyOnDevice':     (False,    '_kyOnDevice', bool),
        'kyRelease':      (False,    '_kyRelease', bool),
    }

    maskKeys = ['nky', 'Disc', 'parallel', 'kyOnDevice', 'kyRelease']
    TRANSPOSABLE = True        # (`transposed` stays in the config the ky sub-problems are built from: every A_ky is transposed)

    @property
    def Disc(self):
        """discretisation of the ky sub-problems.  A frequency dispatcher hands its own 'Disc' key down (distributors.py:254 masks only 'freqs'),
        so under `Helm25DProblem` / `MultiFreq(Disc=MiniZephyr25D)` this class finds ITSELF there: in the reference that recursion ends in
        "requires parameter 'nky'" (minizephyr.py:353-370; oracle/make_golden.py g11 asserts it), here it means the default."""
        d = getattr(self, '_Disc', None)
        if d is None or (isinstance(d, type) and issubclass(d, MiniZephyr25D)):
            self._Disc = MiniZephyr
        return self._Disc

    @property
    def nky(self):
        if getattr(self, '_nky', None) is None:
            self._nky = 1
        return self._nky

    @property
    def cmin(self):
        'minimum velocity of the model (or a representative equivalent)'
        if getattr(self, '_cmin', None) is None:
            return np.min(self.c)
        return self._cmin

    @property
    def pkys(self):
        'regularly sampled cross-line wavenumbers (an inverse DFT quadrature), minizephyr.py:380-394'
        indices = np.arange(self.nky)
        dky = self.freq / (self.cmin * (self.nky - 1)) if self.nky > 1 else 0.
        return indices * np.real(dky)

    @property
    def kyweights(self):
        return 1. + (np.arange(self.nky) > 0)

    @property
    def spUpdates(self):
        weightfac = 1. / (2 * self.nky - 1) if self.nky > 1 else 1.
        return [{'ky': ky, 'premul': weightfac * (1. + (ky > 0))} for ky in self.pkys]

    @property
    def parallel(self):
        return False

    @property
    def scaleTerm(self):
        return getattr(self, '_scaleTerm', 1.) * np.exp(1j * np.pi) / (4 * np.pi)

    # ---- the ky sum on the device -------------------------------------------------------------------------
    # The composite presents itself to the device pipelines (device_survey.gradient / dpred, BaseMPDist) as ONE device operator: right-hand
    # sides are expanded / uploaded once (they are shared by all ky), every ky is solved into a scratch buffer in HBM and added to the caller's
    # buffer by helm_axpby_device, and what leaves the GPU is the sum (or its receiver samples).

    @property
    def kyOnDevice(self):
        'config key (default True): False forces the host reduction -- every ky returns its wavefields to the host, numpy adds them'
        return bool(getattr(self, '_kyOnDevice', True))

    @property
    def kyRelease(self):
        """config key (default False: every ky operator lives until `del factors`): destroy a ky operator after its last solve of the current call.  A
        1024^2 factorisation is 2.9 GB; many frequencies x many ky do not fit into HBM together."""
        return bool(getattr(self, '_kyRelease', False))

    @property
    def deviceCapable(self):
        """True when every ky sub-problem is a device operator whose product IS the library's solve: it has solveDevice and has not replaced
        `__mul__` (a sub-class that computes its product some other way is not represented by the solveDevice it inherits)."""
        return all(hasattr(sub, 'solveDevice') and type(sub).__mul__ is BaseDiscretization.__mul__ for sub in self.subProblems)

    @property
    def kySumOnDevice(self):
        'the ky sum of this composite is formed in HBM (given a GPU): what the device pipelines of problem.py ask before they take it as an operator'
        return self.kyOnDevice and self.deviceCapable

    def _onDevice(self):
        if not self.kySumOnDevice:
            return False
        if '_gpuThere' not in self.__dict__:
            self._gpuThere = _lib.gpu_usable()
        return self._gpuThere

    # (BaseDiscretization's `factors` looks at the handle of the object itself, which a composite does not have)
    @property
    def factors(self):
        return DiscretizationWrapper.factors.fget(self)

    @factors.deleter
    def factors(self):
        DiscretizationWrapper.factors.fdel(self)

    @property
    def handle(self):
        raise AttributeError('MiniZephyr25D is a sum of operators and has no device handle of its own')

    def prefactor(self, nrhs=None):
        """Start the factorisations of the first KY_GROUP ky operators and return at once (the dispatchers' prepare step); the rest are enqueued by the ky loop
        itself, one group ahead of the solves (ky_schedule).  Host reduction: nothing -- every ky factors inside its own first solve."""
        if self._onDevice():
            prefactor_many(self.subProblems[:KY_GROUP])

    def reserve(self, nrhs, rows=None, concurrent=1):
        'the library pools serve host-array solves (the host reduction); the device path keeps its buffers in torch tensors'
        if not self._onDevice():
            self.subProblems[0].reserve(nrhs, rows=rows, concurrent=concurrent)

    def rhsFromSparseDevice(self, q, d_rhs, layout='rhs'):
        return self.subProblems[0].rhsFromSparseDevice(q, d_rhs, layout=layout)         # (the right-hand sides are the same for all ky)

    def rhsFromSamplesDevice(self, d_resid, ld, plan_dev, c0, c1, d_rhs, rows=None):
        return self.subProblems[0].rhsFromSamplesDevice(d_resid, ld, plan_dev, c0, c1, d_rhs, rows=rows)

    def rhsSupportFromSparse(self, q):
        return self.subProblems[0].rhsSupportFromSparse(q)

    def _liveSub(self):
        'a ky operator for a kernel that reads no operator data (imaging, sampling, packing): any handle on this GPU serves -- one that is alive, if there is one'
        subs = self.subProblems
        return next((s for s in subs if s.factors), subs[0])

    def imagingAccumulateDevice(self, d_uf, d_ub, nsrc, d_scaler, d_g, d_exp=None):
        sub = self._liveSub()
        sub.imagingAccumulateDevice(d_uf, d_ub, nsrc, d_scaler, d_g, d_exp=d_exp)
        if self.kyRelease:
            del sub.factors

    def energyAccumulateDevice(self, d_u, nsrc, alpha, d_w, d_e, d_exp=None, rows=None):
        'the energy of wavefields that are the ky SUM already (solveDevice formed it)'
        sub = self._liveSub()
        sub.energyAccumulateDevice(d_u, nsrc, alpha, d_w, d_e, d_exp=d_exp, rows=rows)
        if self.kyRelease:
            del sub.factors

    def sampleDevice(self, d_u, nsrc, csr_dev, d_out, d_exp=None):
        'receiver samples of wavefields that are the ky SUM already (device_survey.dpredFromFields: solveDevice formed it in the store)'
        self._liveSub().sampleDevice(d_u, nsrc, csr_dev, d_out, d_exp=d_exp)

    def packDevice(self, d_u, nsrc, d_out, d_exp, rows=None):
        self._liveSub().packDevice(d_u, nsrc, d_out, d_exp, rows=rows)

    def virtualSourcesDevice(self, d_u, nsrc, d_w, d_r, d_exp=None, rows=None):
        'virtual sources from wavefields that are the ky SUM already'
        self._liveSub().virtualSourcesDevice(d_u, nsrc, d_w, d_r, d_exp=d_exp, rows=rows)

    def _kyLoop(self, each):
        'each(k, sub) for k = 0 .. nky-1 in the order of ky_schedule, the factorisations of the next group enqueued while the current one is being solved'
        subs = self.subProblems
        for step, arg in ky_schedule(len(subs), KY_GROUP):
            if step == 'prefactor':
                prefactor_many([subs[k] for k in arg])
            else:
                each(arg, subs[arg])
                if self.kyRelease:
                    del subs[arg].factors

    def _kyCoefficients(self, k):
        """(alpha, beta) of term k of  scaleTerm * (((u_0 + u_1) + u_2) + ... + u_{nky-1}):  the partial sums are formed unscaled in the reference's order
        (reduce(np.add, ...)), and the LAST accumulation applies the scale to both of its operands, acc = scaleTerm * acc + scaleTerm * u_last.
        That is scaleTerm * (acc + u_last) with the product distributed over the final addition: the same terms, one rounding more per element
        than the reference's single product, and no scaling pass over the result."""
        st = complex(self.scaleTerm)
        last = k == len(self.subProblems) - 1
        alpha = st if last else 1.0 + 0.0j
        beta = 0.0j if k == 0 else (st if last else 1.0 + 0.0j)
        return alpha, beta

    def solveDevice(self, d_rhs, d_u, nrhs, rows=None, layout='rhs', support=None):
        """d_u = scaleTerm * sum_ky conj(A_ky^-1 (premul_ky * rhs)) with everything in HBM (arguments of BaseDiscretization.solveDevice).  d_u need not be
        initialised.  `support` is handed to every ky solve (the library forgets it after one)."""
        import torch
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        n = rows * int(nrhs)
        scratch = torch.empty(n, dtype=torch.complex128, device=torch.device('cuda', self.device))
        infos = []

        def each(k, sub):
            infos.append(sub.solveDevice(d_rhs, scratch.data_ptr(), nrhs, rows, layout=layout, support=support))
            a, b = self._kyCoefficients(k)
            _lib.check(lib.helm_axpby_device(sub.handle, a.real, a.imag, ctypes.c_void_p(scratch.data_ptr()), b.real, b.imag, ctypes.c_void_p(d_u), n), sub.handle)
        self._kyLoop(each)
        self.lastInfo = infos
        return infos

    def sampleSumDevice(self, d_rhs, nrhs, csr_dev, d_out, rows=None):
        """d_out[nrec][nrhs] = scaleTerm * sum_ky R u_ky for the receiver CSR csr_dev = (rowptr, col, val, nrec[, row_stride]) (device tensors, as for
        BaseDiscretization.sampleDevice; right-hand sides in layout 'rhs'): sampling is linear, so each ky's samples are accumulated and the summed
        wavefields are never formed."""
        import torch
        lib = _lib.load()
        rows = int(self.nrow if rows is None else rows)
        rowptr, col, val, nrec = csr_dev[:4]
        stride = int(csr_dev[4]) if len(csr_dev) > 4 else 0
        scratch = torch.empty(rows * int(nrhs), dtype=torch.complex128, device=torch.device('cuda', self.device))
        infos = []

        def each(k, sub):
            infos.append(sub.solveDevice(d_rhs, scratch.data_ptr(), nrhs, rows))
            a, b = self._kyCoefficients(k)
            _lib.check(lib.helm_sample_rows_device(sub.handle, ctypes.c_void_p(scratch.data_ptr()), int(nrhs), rows, ctypes.c_void_p(rowptr.data_ptr()),
                                                   ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()), int(nrec), stride, a.real, a.imag, b.real, b.imag,
                                                   ctypes.c_void_p(d_out)), sub.handle)
        self._kyLoop(each)
        self.lastInfo = infos
        return infos

    def __mul__(self, rhs):
        if not self._onDevice():
            return self.scaleTerm * reduce(np.add, (sub * rhs for sub in self.subProblems))
        # right-hand sides up ONCE (a sparse matrix as triplets, expanded on the GPU), the ky sum in HBM, the result down ONCE -- in the reference's own
        # (N, nrhs) C-order layout, so that no transpose exists on either side
        import torch
        rhs, onedim = self._as_rhs(rhs)
        if rhs.shape[0] != self.nrow:
            raise ValueError('dimension mismatch')
        N, ncol = int(self.nrow), int(rhs.shape[1])
        dev = torch.device('cuda', self.device)
        U = torch.empty((N, ncol), dtype=torch.complex128, device=dev)
        support = None
        if sp.issparse(rhs):
            R = torch.empty((N, ncol), dtype=torch.complex128, device=dev)
            self.rhsFromSparseDevice(rhs, R.data_ptr(), layout='node')
            if ncol <= 512:
                support = self.rhsSupportFromSparse(rhs)
        else:
            R = _lib.to_device(rhs, dev, np.complex128)
        _lib.wait_torch_stream(dev)
        self.solveDevice(R.data_ptr(), U.data_ptr(), ncol, N, layout='node', support=support)
        del R, support
        u = _lib.from_device_pinned(U)
        return u[:, 0] if onedim else u


KY_GROUP = 2        # ky operators whose factorisations are enqueued together (helm_prefactor_many takes up to 4)


def ky_schedule(nky, group=KY_GROUP):
    """The order of steps of one pass over the ky operators: a list of ('prefactor', (k, ...)) and ('solve', k).  Solves in ascending ky (the order of the
    reference's sum); every ky is prefactored exactly once, in groups of `group`, before its solve; the next group is enqueued just before the first solve of
    the current one, so its factorisations run beside those solves, and never more than 2 * group operators are prefactored and unsolved."""
    nky, group = int(nky), max(1, int(group))
    steps, nxt = [], 0
    for k in range(nky):
        if k % group == 0:
            while nxt < min(nky, k + 2 * group):          # (the first solve is preceded by its own group and the next one)
                part = tuple(range(nxt, min(nky, nxt + group)))
                steps.append(('prefactor', part))
                nxt = part[-1] + 1
        steps.append(('solve', k))
    return steps
