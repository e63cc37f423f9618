"""Forward problem and FWI gradient on top of the frequency dispatcher.

Interface of zephyr/middleware/problem.py:17-212 (HelmBaseProblem / Helm2DProblem) without SimPEG:
`lazyFields` (forward wavefields per frequency), `Jtvec` (gradient by the zero-lag imaging
condition; both the "mux" branch that solves forward and back-propagated sources together and the
branch that re-uses given forward fields) and `updateModel`.

Multi-GPU, two ways.  In one process (no process group): the system wrapper's parallel mode deals work items
(frequency, source batch) frequency-major over the visible GPUs -- one solve thread and one prepare-ahead
thread per GPU (`zephyr_amd.dispatch`), sources of a frequency split over spare GPUs when there are fewer
frequencies than GPUs -- and the per-GPU partial gradients / data panels are summed on the host.  One
process per GPU (`shardFreqs`, default on when torch.distributed is initialised): frequencies are sharded
over ranks and the only collective is one all-reduce of the gradient (problem.py:152,162 sum over
frequencies) or of the receiver data.  The device-resident loops of `dpred` and the mux `Jtvec` (item dealing,
per-worker buffers, partial gradients) live in `zephyr_amd.device_survey`; `_dpredDevice` / `_JtvecDevice` delegate to it.  `fieldsDevice` leaves the
forward wavefields in HBM (`zephyr_amd.fieldstore.DeviceFields`) for `survey.dpred(m, u=F)` and `Jtvec(m, v, u=F)`.  `illumination` (no counterpart in the
reference) returns the source- or receiver-side illumination, the diagonal pseudo-Hessian or the exact diagonal of the Gauss-Newton Hessian from those fields,
what a gradient is preconditioned with; `hessianBlocks` returns the per-cell 2 x 2 blocks of the joint (c, rho) Hessian for a two-parameter gradient
(`frechet.blockSolve` divides by them).
"""
import contextlib

import numpy as np
import scipy.sparse as sp

from .base import BaseModelDependent
from .config import BaseSCCache
from .distributors import MultiFreq, ViscoMultiFreq, ViscoMultiGridMultiFreq
from .survey import HelmBaseSurvey, HelmMultiGridSurvey, Helm2DSurvey, Helm25DSurvey
from . import parallel
from . import device_survey
from . import _lib
from .fieldstore import DeviceFields
from .frechet import MZ_MASS, maskInterior, massStencil, operatorWeight      # noqa: F401 (what linearisation='operator' is made of)
from .frechet import applyPlanes, buoyancyAdjoint, buoyancyPlanes, lagProducts      # (and what parameter='rho' is made of)
from .frechet import gardnerChain, velocityAdjoint, velocityPlanes                  # (and linearisation='full')
from .frechet import operatorPseudoHessianWeight, pseudoHessianDiagonal              # (and the pseudo-Hessian diagonal of either)
from .frechet import gaussNewtonDiagonal, lagGram                                   # (and the exact diagonal of the Gauss-Newton Hessian)
from .frechet import applyPlanesTransposed, massPlanes, velocityCurvature           # (and the residual part of the Newton Hessian)
from .frechet import mixedAdjointB, mixedAdjointC                                   # (and the mixed second derivative of parameter='joint')
from .frechet import gaussNewtonBlocks, pseudoHessianBlocks                         # (and the per-cell 2 x 2 blocks of the joint Hessian)
from .frechet import eurusAdjoint, eurusPlanes                                      # (and the derivative maps of the Eurus block M1)
from .frechet import viscoChain                                                     # (and the chain from (c, Q) to the complex velocity of a visco problem)

EPS = 1e-15


def _norm2(d):
    """||d||_2 without BLAS.  np.linalg.norm hands a vector of this size to a threaded dot product, and OpenBLAS's workers (64 of them on a large host) then
    spin for ~100 ms waiting for more work: under a container CPU quota (cgroup cpu.max, 16 CPUs on the GPU boxes of this project) that burns the period's
    budget in 25 ms and the scheduler freezes EVERY thread of the process -- the ones feeding the GPU included -- for the remaining 75 ms.  Round 6: this one
    call cost dpred / Jtvec 60-80 of their 110-140 ms (problem.py:51-66 compares the models the same way)."""
    d = np.asarray(d)
    return float(np.sqrt(np.add.reduce(np.square(d.real)) + (np.add.reduce(np.square(d.imag)) if np.iscomplexobj(d) else 0.0)))


class HelmBaseProblem(BaseModelDependent, BaseSCCache):

    initMap = {
        #   key              required  rename       cast
        'SystemWrapper':    (True,     None,        None),
        'shardFreqs':       (False,    '_shard',    bool),
        'hostGradient':     (False,    '_hostGradient', bool),    # force the numpy imaging condition
        'fieldsDtype':      (False,    '_fieldsDtype', str),      # what fieldsDevice() keeps: 'complex128' (default) or 'complex64' (half the memory)
        'eurusDerivatives': (False,    '_eurusDerivatives', bool),    # an Eurus problem (eps == delta) serves the exact adjoint and the exact derivatives through M1^T
        'viscoDerivatives': (False,    '_viscoDerivatives', bool),    # a visco problem serves the exact derivatives ('operator' / 'full') through the chain from (c, Q)
        'kyDerivatives':    (False,    '_kyDerivatives', bool),       # a 2.5-D problem serves the exact derivatives from the forward fields kept PER ky (fieldsDevice(perKy=True))
        'multiscaleDerivatives': (False, '_multiscaleDerivatives', bool),    # a multiscale pairing serves the exact derivatives: per-grid maps, then the transposed grid transfer
        'misfitHostData':   (False,    '_misfitHostData', bool),      # a DataMisfit keeps to its generic route: the data come down, the adjoint source goes up
    }

    surveyPair = HelmBaseSurvey
    cacheItems = ['_system', '_adjointSystem']

    def __init__(self, systemConfig, *args, **kwargs):
        BaseSCCache.__init__(self, systemConfig, *args, **kwargs)
        self.survey = None

    # ---- pairing (SimPEG's BaseProblem.pair) -----------------------------------------------------------
    def pair(self, survey):
        if not isinstance(survey, self.surveyPair):
            raise TypeError('%s must be paired with a %s' % (self.__class__.__name__, self.surveyPair.__name__))
        self.survey = survey
        survey.prob = self

    @property
    def ispaired(self):
        return self.survey is not None

    def _requirePaired(self):
        if not self.ispaired:
            raise Exception('%s instance is not paired to a survey' % (self.__class__.__name__,))

    # ---- model -----------------------------------------------------------------------------------------
    def updateModel(self, m, loneKey='c'):
        'problem.py:51-66'
        if m is None:
            return
        if isinstance(m, dict):
            self.systemConfig.update(m)
            self.clearCache()
        elif isinstance(m, (np.ndarray, np.inexact, complex, float)):
            m = np.asarray(m)
            old = np.asarray(self.systemConfig.get(loneKey, 0.))
            if old.size != m.size or not _norm2(m.ravel() - old.ravel()) < EPS:
                self.systemConfig[loneKey] = m
                self.clearCache()
        else:
            raise Exception('Class %s doesn\'t know how to update with model of type %s' % (self.__class__.__name__, type(m)))

    def clearCache(self):
        self._modelStamp = self.__dict__.get('_modelStamp', 0) + 1        # (what a DeviceFields remembers: fields of an earlier model are refused)
        for name in ('_system', '_adjointSystem'):
            sysw = self.__dict__.get(name, None)
            if sysw is not None:
                del sysw.factors
        BaseSCCache.clearCache(self)

    @property
    def system(self):
        if getattr(self, '_system', None) is None:
            self._system = self.SystemWrapper(self.systemConfig)
        return self._system

    @property
    def adjointSystem(self):
        """The system wrapper of the TRANSPOSED operators: the class of `system`, built from the same systemConfig plus `transposed=True` when first asked for
        -- the same frequencies on the same devices, the same replicas for split sources.  `sub * q` there is conj(A_f^-T (premul q)), what
        Jtvec(adjoint='transpose') back-propagates through.  It goes with the problem's cache on a model change, and `del prob.factors` releases it too.
        While both wrappers are in use the factors of A_f and of A_f^T are resident side by side: twice the device memory of `system` alone.
        2-D MiniZephyr / MiniZephyrHD / MiniZephyr25D on one grid, and Eurus / EurusHD with eurusDerivatives=True and eps == delta (M1^T, helm_set_transposed_m1);
        Eurus otherwise and the 3-D operator raise NotImplementedError (Helm3DProblem has an adjointSystem of its own); so do the multiscale wrappers unless the config sets multiscaleDerivatives=True (then the
        transposed operator of every frequency lives on that frequency's grid)."""
        if getattr(self, '_adjointSystem', None) is None:
            from .distributors import MultiGridMultiFreq
            cls = type(self.system)
            if (issubclass(cls, MultiGridMultiFreq) or isinstance(self.survey, HelmMultiGridSurvey)) and not self._multiscaleServed():
                raise NotImplementedError('the transposed operator serves single-grid problems: a multiscale pairing has no exact-adjoint route')
            self._refuseMultiscale('adjointSystem')           # (with the key: the visco / 2.5-D / Eurus pairings and a transfer without a transpose say why not)
            cfg = dict(self.systemConfig)
            cfg['transposed'] = True
            adj = cls(cfg)
            adj.subProblems                                # (Eurus / 3-D refuse here, not in the middle of a product)
            self._adjointSystem = adj
        return self._adjointSystem

    # ---- sharding --------------------------------------------------------------------------------------
    @property
    def ownedFreqs(self):
        'frequency indices this rank solves'
        nf = self.survey.nfreq
        if getattr(self, '_shard', True):
            return parallel.owned_indices(nf)
        return list(range(nf))

    @property
    def _sharded(self):
        '''True when the frequencies are split over ranks.  The decision is the same on every rank (it must be: it
        guards a collective -- a rank that owns every frequency of a short list still has to enter the all-reduce
        the ranks that own none are waiting in).'''
        return bool(getattr(self, '_shard', True)) and parallel.rank_and_size()[1] > 1

    def _solveOwned(self, rhs_list, sysw=None):
        'generator of (ifreq, scaleTerm * sub * rhs) over the owned frequencies; sysw: the wrapper to solve with (default `system`; `adjointSystem` for A^-T)'
        owned = self.ownedFreqs
        sysw = self.system if sysw is None else sysw
        if len(owned) == self.survey.nfreq and getattr(sysw, 'parallel', False) and hasattr(sysw, 'devices'):
            # every frequency is this process's: the wrapper's own dispatch (all visible GPUs, prepare-ahead) does the loop
            rl = list(rhs_list) if isinstance(rhs_list, (list, tuple)) else rhs_list
            for ifreq, u in enumerate(sysw * rl):
                yield ifreq, u
            return
        subs = sysw.subProblems
        scale = sysw.scaleTerm
        for ifreq in owned:
            r = rhs_list[ifreq] if isinstance(rhs_list, (list, tuple)) else rhs_list
            yield ifreq, scale * (subs[ifreq] * r)

    # ---- device-resident work items ---------------------------------------------------------------------------
    def _deviceItems(self, owned, ncols):
        "work items (worker, operator, ifreq, c0, c1) of the device-resident dpred / Jtvec loops: device_survey.deviceItems for this problem's system"
        return device_survey.deviceItems(self.system, owned, ncols)

    # ---- gradient scalers (problem.py:74-85) --------------------------------------------------------------
    def scaledTerms(self, ifreq):
        omega = 2 * np.pi * self.survey.freqs[ifreq]
        c = self.system.subProblems[ifreq].c
        return omega, c

    def gradientScaler(self, ifreq):
        omega, c = self.scaledTerms(ifreq)
        return self.survey.postProcessors[ifreq](-(omega ** 2 / c ** 3).ravel())

    def sensScaler(self, ifreq):
        'problem.py:83-85'
        omega, c = self.scaledTerms(ifreq)
        return self.survey.postProcessors[ifreq](-(c ** 3 / omega ** 2).ravel())

    # ---- forward -----------------------------------------------------------------------------------------
    def lazyFields(self, m=None):
        'generator of forward wavefields (N, nsrc) for the owned frequencies, in frequency order (problem.py:166-179)'
        self._requirePaired()
        self.updateModel(m)
        qf = self.survey.getSources()
        return (u for _, u in self._solveOwned(qf))

    def _requirePerKy(self, what):
        'perKy=True is the fields of a 2.5-D composite per cross-line wavenumber: ValueError on any other problem'
        from .minizephyr import MiniZephyr25D
        subs = self.system.subProblems
        if not (subs and isinstance(subs[0], MiniZephyr25D)) or isinstance(self.survey, HelmMultiGridSurvey):
            raise ValueError('%s(perKy=True) serves single-grid 2.5-D problems (MiniZephyr25D): %s has no ky axis'
                             % (what, type(subs[0]).__name__ if subs else type(self.system).__name__))

    def fields(self, m=None, perKy=False, ownGrid=False):
        """list of forward wavefields for ALL frequencies on this rank (no sharding), on the native grid (problem.py:181-191: post-processed).
        ownGrid (multiscale pairings; on a single grid it changes nothing): every frequency's fields on ITS grid, as they were solved and not up-scaled --
        what the exact derivatives of a multiscale problem (multiscaleDerivatives=True) take as host `u`, and what `dpred(u=)` samples without a round trip.
        perKy (2.5-D problems): one (nky, N, nsrc) array per frequency, the fields of every cross-line wavenumber apart -- their sum over ky is the default's
        entry -- what the exact derivatives of a 2.5-D problem take as host `u`."""
        self._requirePaired()
        self.updateModel(m)
        qf = self.survey.getSources()
        if perKy:
            self._requirePerKy('fields')
            return [self._kyFieldsHost(i, device_survey._ofFrequency(qf, i)) for i in range(self.survey.nfreq)]
        if ownGrid:
            return [np.asarray(u) for u in self.system * qf]
        return [pp(u) for u, pp in zip(self.system * qf, self.survey.postProcessors)]

    @property
    def fieldsDtype(self):
        "config key: the number format of the store fieldsDevice() fills -- 'complex128' (default), or 'complex64' with one power-of-two scale per column"
        return getattr(self, '_fieldsDtype', 'complex128')

    def fieldsDevice(self, m=None, perKy=False):
        """The forward wavefields of the owned frequencies, solved once and LEFT in HBM: a fieldstore.DeviceFields to hand to `survey.dpred(m, u=F)` and
        `Jtvec(m, v, u=F)`, which then solve nsrc columns per frequency between them and the back-propagation instead of re-solving the forward fields.
        `F[ifreq]` downloads what `fields()[ifreq]` would be.  Single-grid surveys (2-D, and 2.5-D with the ky sum on the device); without the device
        path (no GPU, hostGradient, a host ky reduction) this raises and `fields()` is the route.  A multiscale pairing with multiscaleDerivatives=True: every
        frequency's fields on ITS grid (a slice is (k, N_f)), `F[ifreq]` what `fields(ownGrid=True)[ifreq]` would be; without the key it raises as it always did.
        That store serves `dpred(u=F)` and the 'operator' / 'full' routes of Jtvec(adjoint='transpose') / JvecBorn / Hvec; the reference's `Jtvec(m, v, u=F)` and
        `illumination(u=F)` read native-grid fields and refuse it (NotImplementedError).
        perKy (2.5-D problems; ValueError elsewhere): every ky of an item is solved into its own block of the item's slice, nky times the memory -- what the
        exact derivatives of a 2.5-D problem (kyDerivatives=True) read; `dpred(u=)` forms the ky sum while sampling and `F[ifreq]` still downloads the sum."""
        self._requirePaired()
        self.updateModel(m)
        if perKy:
            self._requirePerKy('fieldsDevice')
        if isinstance(self.survey, HelmMultiGridSurvey):
            if not self._multiscaleServed():
                return device_survey.fields(self, [], self.fieldsDtype)        # (raises NotImplementedError with the reason)
            self._refuseMultiscale('fieldsDevice')                             # (with the key: every frequency's fields on ITS grid; the other pairings say why not)
        if not self._deviceGradientAvailable():
            raise RuntimeError('fieldsDevice needs the device path (GPU operators with solveDevice, no hostGradient, the ky sum on the device): use fields()')
        return device_survey.fields(self, self.ownedFreqs, self.fieldsDtype, perKy=bool(perKy))

    # ---- sensitivity times vector ------------------------------------------------------------------------
    def Jvec(self, m=None, v=None, u=None):
        """Data perturbation for a model perturbation v (problem.py:87-122): one virtual source
        `v * (-c^3/omega^2)` per frequency is solved, and dpert[:, :, f] is the outer product of the
        receiver and source samplings of that field.  Fixed receiver arrays only: the reference's
        relative-geometry branch multiplies mismatched shapes (problem.py:117-120).

        This is the reference's one-column outer-product approximation and stays as it is; it is NOT the adjoint of Jtvec.  The Born data that
        pair with Jtvec(adjoint='transpose') exactly are `JvecBorn`."""
        self._requirePaired()
        if v is None:
            raise Exception('Actually, Jvec requires a perturbation vector')
        self.updateModel(m)
        sv = self.survey
        if sv.mode != 'fixed':
            raise ValueError('dimension mismatch')
        perturb = np.asarray(v).reshape((self.nz * self.nx, 1))
        qv = [sv.preProcessors[i](perturb * self.sensScaler(i).reshape((self.nz * self.nx, 1))) for i in range(sv.nfreq)]
        qf = sv.getSources()
        dpert = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
        for ifreq, uFreq in self._solveOwned(qv):
            srcTerms = qf[ifreq].T * uFreq
            recTerms = sv.rVec(0, ifreq) * uFreq
            dpert[:, :, ifreq] = np.asarray(recTerms).reshape((sv.nrec, 1)) * np.asarray(srcTerms).reshape((1, sv.nsrc))
        if self._sharded:
            dpert = parallel.allreduce_sum(dpert)
        return dpert.ravel()

    # ---- gradient ----------------------------------------------------------------------------------------
    def Jtvec(self, m=None, v=None, u=None, adjoint='reciprocity', linearisation='scaler', parameter='c'):
        """FWI gradient g = sum_f scaler_f sum_s uF (.) uB  (problem.py:124-164).

        u is None: "mux" branch -- forward and back-propagated sources are stacked column-wise and
        solved together per frequency; the result is complex (no .real), as in the reference.
        u given (list of forward fields per frequency): only the back-propagation is solved and
        the real part is returned.  u a DeviceFields (fieldsDevice): the same with the forward fields
        read where they were solved, in HBM.

        adjoint='reciprocity' (default): the back-propagation runs through the forward factors, as in the reference.  That is the adjoint of the
        modelling operator only if A is complex-symmetric, which the 9-point MiniZephyr operator is not (PML and density scale its rows).
        adjoint='transpose': the back-propagation runs through A^-T (`adjointSystem`),
            g = Re sum_f w_f (.) sum_s uF_s (.) (scaleTerm S_f^T R_s^T r_s),   S_f^T q = conj(A_f^-T premul q),  w_f = gradientScaler(f),
        always real float64 (N,) -- there is no mux branch, forward and back solves use different factors -- and the exact adjoint of `JvecBorn` under
        <a, b> = Re sum conj(a) b.  u a DeviceFields: on the device; u None with the device path: fieldsDevice() internally, released afterwards;
        u a list of host arrays, or no device path: numpy.  Fixed and moving receiver arrays.  A multiscale pairing raises NotImplementedError unless the
        config sets multiscaleDerivatives=True (below).

        linearisation='scaler' (default): the weight is the reference's gradientScaler w_f = -omega^2 / c^3, the reference's convention.  That is NOT the
        derivative of `dpred`: the assembled operator carries c as K = (omega_d^2 / c^2 - ky^2) / rho spread over nine slots by the mass weights, with
        identity boundary rows, so this g is a rho-dependent rescaling of the gradient (and of the opposite sign).
        linearisation='operator' (needs adjoint='transpose'): g = J^T v with J the derivative of `dpred` (see `JvecBorn`), the gradient of
        1/2 ||dpred - dobs||^2 for v = dpred - dobs,
            g = Re sum_f W_f (.) sum_s U_s (.) M0(mask_int (.) uB_s),   W_f = 2 scaleTerm conj(omega_d^2 / premul) / (c^3 rho),
        U_s the unscaled forward solve and uB_s = conj(A_f^-T premul R_s^H v_s).  `_requireOperatorLinearisation` lists what it serves.
        linearisation='full' (needs adjoint='transpose'): the exact adjoint of JvecBorn(linearisation='full'), the gradient with respect to the velocity in
        every cell -- absorbing layers included, with an explicit or the default density.  With P_f the nine lag products below and V_f the map of
        frechet.velocityPlanes,  g = Re sum_f -(conj(scaleTerm) / premul) (V_f^T P_f + (d b / d c) (.) L_f^T P_f),  the second term only without `rho`.

        parameter='c' (default): all of the above.  parameter='rho' (needs linearisation='operator', hence adjoint='transpose'): the gradient with
        respect to the density of the config at fixed c, the exact adjoint of JvecBorn(parameter='rho'), float64 (N,) in density units.  With
        P_f,k[i] = sum_s z_s[i] u^_s[i + off_k] the nine lag products of the transposed back-propagation z_s = A_f^-T premul R_s^H v_s against the unscaled
        forward solves (zero where i is on a boundary line), and L_f the linear map from a buoyancy field to the nine planes of the interior rows
        (frechet.buoyancyPlanes),
            g_b = Re sum_f -(conj(scaleTerm) / premul) L_f^T P_f,      g_rho = -g_b / rho^2.
        m stays the velocity.  The same routes as 'c'.  With linearisation='full' and an explicit `rho` this is 'operator' under another name; without one
        the density is not a free parameter and the call raises NotImplementedError.
        parameter='joint' ('operator' or 'full', an explicit `rho`): [g_c; g_rho], float64 (2 N,), from ONE back-propagation per source and frequency -- both are
        transposes applied to the same lag products, g_c = Re w V_f^T P_f (its mass term alone for 'operator'), g_rho = -(Re w L_f^T P_f) / rho^2.

        A visco problem (Helm2DViscoProblem: `system` a ViscoMultiFreq; MiniZephyr / MiniZephyrHD on one grid, an explicit `rho`) with 'operator' or 'full' is
        served when the config sets viscoDerivatives=True (opt-in; without the key it is refused with NotImplementedError, as it always was): the
        operator of frequency f is assembled at the complex velocity c~_f = c (1 + lam_f / Q)(1 + i / (2 Q)) and is holomorphic in it, so with
        t_f = w V_f^T P_f the complex cell gradient with respect to c~_f and (gamma_f, chi_f) = d c~_f / d (c, Q) (frechet.viscoChain)
            parameter='c': g_c = Re sum_f gamma_f t_f (at fixed Q),   parameter='Q': g_Q = Re sum_f chi_f t_f,   parameter='cQ': [g_c; g_Q], float64 (2 N,),
        all from ONE back-propagation per source and frequency.  The derivative is with respect to Q itself (for 1 / Q multiply by -Q^2).  parameter='rho' is what
        it is above, at the complex velocity.  'Q' / 'cQ' with 'scaler' or on a problem without Q: ValueError; parameter='joint' and a config without `rho`
        (Gardner's density is not holomorphic in c~): NotImplementedError.  'scaler' on a visco problem stays the reference's weight.

        A 2.5-D problem (Helm25DProblem over MiniZephyr25D, one grid, an explicit `cmin`) with 'operator' or 'full' is served when the config sets kyDerivatives=True
        (opt-in; without the key it is refused as it always was): the data are st R sum_k conj(u^_k), so the gradient is a sum over ky of the expressions above
        on ky sub-operator k and fields of the SAME ky, g = Re sum_f sum_k w_fk T_k^T lag(z_k, u^_k) with w_fk = -conj(st) / premul_k (`_JtvecKy`).  u is then the
        per-ky store of fieldsDevice(perKy=True) (the ky-SUM store: ValueError), a host list of fields(perKy=True), or None.  'scaler' is unchanged.

        A multiscale pairing (MultiGridMultiFreq + Helm2DMultiGridSurvey over MiniZephyr / MiniZephyrHD) with 'operator' or 'full' is served when the config sets
        multiscaleDerivatives=True (opt-in; without the key it is refused as it always was, and the mux gradient is untouched either way).  On the grid of
        frequency f the sub-problem sees c_f = S_f c and rho_f = S_f rho, S_f the real, linear spline down-scaler, so g = sum_f S_f^T g_f: g_f is the expression
        above on that grid -- chains included, -1 / rho_f^2 and Gardner's d b / d c at c_f -- and S_f^T the exact transpose of the windowed transfer
        (`ds.adjoint`; `ds.T`, the interpolation back up that the mux gradient uses, is not that).  u is then the store of fieldsDevice() (every frequency on
        ITS grid), a host list of fields(ownGrid=True) (a native-size array for a coarser frequency: ValueError), or None.  The result is on the native grid.
        What it looks like: S_f SAMPLES the model, it does not average it, so S_f^T puts a coarse cell's gradient on the few native nodes around its sample
        point -- the column sums of a 1-D axis at scale 2.47 run from -0.25 to 1.07, and at an integer scale s only every s-th node receives anything.  That IS
        the derivative of this dpred; smoothing it is the caller's business.  'scaler' with adjoint='transpose', Hvec(resid=), the Hessian diagonals and blocks,
        and visco / 2.5-D / Eurus multiscale pairings are refused with the key (`_refuseMultiscale`).
        """
        self._requirePaired()
        if v is None:
            raise Exception('Actually, Jtvec requires a residual vector')
        if adjoint not in ('reciprocity', 'transpose'):
            raise ValueError('adjoint is %r: \'reciprocity\' or \'transpose\'' % (adjoint,))
        self._checkLinearisation(linearisation)
        if not self._checkViscoParameter(parameter, linearisation):
            self._checkParameter(parameter, linearisation, joint=True)
        if linearisation in ('operator', 'full') and adjoint != 'transpose':
            raise ValueError('linearisation=%r needs adjoint=\'transpose\': the exact derivative back-propagates through A^-T' % (linearisation,))
        self.updateModel(m)
        sv = self.survey
        nsrc = sv.nsrc
        resid = np.asarray(v).reshape((sv.nrec, sv.nsrc, sv.nfreq))
        owned = self.ownedFreqs
        if adjoint == 'transpose':
            return self._JtvecTranspose(resid, u, linearisation, parameter)
        if isinstance(u, DeviceFields):
            # forward fields left in HBM by fieldsDevice(): only the back-propagation is solved, on the store's own items
            self._refusePerGridStore("Jtvec(adjoint='reciprocity', u=F)")
            u.checkCurrent(self)
            return device_survey.gradientFromFields(self, u, self._deviceBackSources(resid), resid)
        if u is None and self._deviceGradientAvailable():
            return self._JtvecDevice(self._deviceBackSources(resid), owned, resid)
        qb = sv.getResidualSources(resid)
        g = np.zeros(self.nrow, dtype=np.complex128)
        if u is None:
            qf = sv.getSources()
            qm = [sp.hstack((qf[i], qb[i])) if i in owned else None for i in range(sv.nfreq)]
            for ifreq, uMux in self._solveOwned(qm):
                pp = sv.postProcessors[ifreq]
                g += self.gradientScaler(ifreq) * pp((uMux[:, :nsrc] * uMux[:, nsrc:]).sum(axis=1))
        else:
            uF = list(u)
            for ifreq, uB in self._solveOwned(qb):
                pp = sv.postProcessors[ifreq]
                g += self.gradientScaler(ifreq) * (np.asarray(uF[ifreq]) * pp(uB)).sum(axis=1)
        if self._sharded:
            g = parallel.allreduce_sum(g)
        return g if u is None else g.real

    # ---- exact adjoint, Born data, Gauss-Newton product ----------------------------------------------------
    def _refuseMultiscale(self, what):
        """a multiscale pairing is refused unless the config sets multiscaleDerivatives=True (opt-in: without the key everything is what it was); with the
        key, what the composition through the transposed grid transfer does not serve is refused here with the reason"""
        if not isinstance(self.survey, HelmMultiGridSurvey):
            return
        if not getattr(self, '_multiscaleDerivatives', False):
            raise NotImplementedError('%s serves single-grid surveys: the transposed operator and the stored forward fields live on one grid' % (what,))
        from .discretization import DiscretizationWrapper
        from .eurus import Eurus
        for ds in self.survey.preProcessors:
            if not hasattr(ds, 'adjoint'):
                raise NotImplementedError('%s with multiscaleDerivatives needs the exact transpose of the grid transfer: %s has no `.adjoint` (its `.T` interpolates '
                                          'back up, which is not the transpose)' % (what, type(ds).__name__))
        if self._isVisco():
            raise NotImplementedError('%s with multiscaleDerivatives does not serve visco problems: the chain from (c, Q) to the complex velocity is formed on the '
                                      'native grid before the down-scaling, and that order is not built into the per-grid routes' % (what,))
        sub = self.system.subProblems[0] if self.system.subProblems else None
        if isinstance(sub, DiscretizationWrapper):
            raise NotImplementedError('%s with multiscaleDerivatives does not serve the 2.5-D composite: the per-ky routes are built for one grid' % (what,))
        if isinstance(sub, Eurus):
            raise NotImplementedError('%s with multiscaleDerivatives does not serve Eurus problems: theta, eps and delta are down-scaled per frequency too, and the '
                                      'derivative maps of M1 are built for one grid' % (what,))

    def _refusePerGridStore(self, what):
        """the store of fieldsDevice() on a multiscale pairing (multiscaleDerivatives=True) holds every frequency on ITS grid: the routes that image or accumulate
        on the native grid -- the reference's u-given gradient, the 'scaler' illumination kinds -- read native-grid fields and are not built for it"""
        if self._multiscaleServed():
            raise NotImplementedError('%s does not read the per-grid store of a multiscale pairing: this route multiplies native-grid forward fields, and the store '
                                      'of multiscaleDerivatives=True holds every frequency on its own grid (u=None or the host list of fields() serve it; the '
                                      'store serves dpred and the \'operator\' / \'full\' routes)' % (what,))

    def _multiscaleServed(self):
        'the config sets multiscaleDerivatives=True and the pairing is a multiscale one: the exact routes run per grid and end in the transposed grid transfer'
        return bool(getattr(self, '_multiscaleDerivatives', False)) and isinstance(self.survey, HelmMultiGridSurvey)

    def _refuseMultiscaleScaler(self, what, linearisation):
        if linearisation == 'scaler' and self._multiscaleServed():
            raise NotImplementedError('%s with linearisation=\'scaler\' does not serve multiscale pairings: the reference\'s weight is up-scaled, not transposed, and has '
                                      'no exact adjoint there (multiscaleDerivatives serves \'operator\' and \'full\')' % (what,))

    def _refuseMultiscaleDiagonal(self, what):
        if self._multiscaleServed():
            raise NotImplementedError('%s does not serve multiscale pairings: the Hessian of frequency f is S_f^T H_f S_f, and diag(S^T H S) is not S^T diag(H) -- the '
                                      'diagonals and blocks of the coarse grids do not compose (Hvec applies the product itself)' % (what,))

    def _ownGridFields(self, u):
        """the forward fields of a multiscale pairing as the exact routes read them: per frequency on ITS grid.  u None: solved now for the owned frequencies (None
        elsewhere); u a host list: checked -- a native-size array for a coarser frequency is what fields() returns, not what was solved"""
        sv = self.survey
        subs = self.system.subProblems
        if u is None:
            uF = [None] * sv.nfreq
            for ifreq, uf in self._solveOwned(sv.getSources()):
                uF[ifreq] = np.asarray(uf)
            return uF
        uF = list(u)
        for ifreq in self.ownedFreqs:
            n = int(subs[ifreq].nz) * int(subs[ifreq].nx)
            if uF[ifreq] is None or np.shape(uF[ifreq])[0] != n:
                raise ValueError('the exact routes of a multiscale pairing read the fields of frequency %d on its own %d x %d grid (%d rows, not %s): pass '
                                 'fields(ownGrid=True)' % (ifreq, subs[ifreq].nz, subs[ifreq].nx, n, None if uF[ifreq] is None else np.shape(uF[ifreq])[0]))
        return uF

    def _gridChains(self, ifreq):
        """(d b / d rho, d b / d c) on the grid of frequency ifreq, float64 (N_f,) each: -1 / rho_f^2 at rho_f = S_f rho where the config gives the density (else
        None), Gardner's chain at c_f = S_f c where it does not (else None).  What depends on the model at a cell is evaluated where the operator is assembled."""
        op = self.system.subProblems[ifreq]
        n = int(op.nz) * int(op.nx)
        if self._hasDensity():
            rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (n,))
            return -1.0 / (rho * rho), None
        return None, gardnerChain(np.broadcast_to(np.asarray(op.c).ravel(), (n,)))

    def _JtvecMultiscale(self, resid, u, linearisation, parameter):
        """Jtvec(adjoint='transpose') of a multiscale pairing with 'operator' or 'full' once the refusals are past: g = sum_f S_f^T g_f, float64 (N,) or (2N,).
        g_f is the single-grid expression on the grid of frequency f -- the lag products of the transposed back-propagation against the forward solves, V_f^T /
        L_f^T, the weight, the real part and the chains (-1 / rho_f^2, or Gardner's at c_f) -- and S_f^T the exact transpose of the down-scaler (`ds.adjoint`)."""
        stretch = linearisation == 'full'
        joint, density = parameter == 'joint', parameter == 'rho'
        adj = self.adjointSystem
        N = self.nrow
        sv = self.survey
        st = complex(self.system.scaleTerm)
        g = np.zeros(2 * N if joint else N, dtype=np.float64)
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                rd = self._hermitianResidual(resid)
                return device_survey.multiscaleGradientFromFields(self, F, self._deviceBackSources(rd), rd, adj, linearisation, parameter)
            qb = [q.conj() for q in sv.getResidualSources(np.conj(resid))]
            for ifreq, uB in self._solveOwned(qb, adj):
                op = self.system.subProblems[ifreq]
                up = sv.preProcessors[ifreq].adjoint
                P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx)
                w = -np.conj(st) / complex(op.premul)
                brho, bc = self._gridChains(ifreq)
                if not density:
                    gf = velocityAdjoint(op, P, stretch=stretch)
                    if bc is not None and stretch:
                        gf = gf + bc * buoyancyAdjoint(op, P)
                    g[:N] += np.asarray(up * np.ascontiguousarray((w * gf).real)).ravel()
                if density or joint:
                    g[-N:] += np.asarray(up * np.ascontiguousarray(brho * (w * buoyancyAdjoint(op, P)).real)).ravel()
        if self._sharded:
            g = parallel.allreduce_sum(g)
        return g

    def _JvecBornMultiscale(self, v, u, linearisation, parameter):
        """JvecBorn of a multiscale pairing with 'operator' or 'full' once the refusals are past: the perturbation goes down once per grid (dc_f = S_f v_c,
        drho_f = S_f v_rho), the buoyancy perturbation is formed there (db_f = -drho_f / rho_f^2, or Gardner's chain at c_f times dc_f), and the planes, the Born
        solve and the sampling are the single-grid ones on the grid of frequency f.  (nrec, nsrc, nfreq) raveled."""
        stretch = linearisation == 'full'
        joint, density = parameter == 'joint', parameter == 'rho'
        sv = self.survey
        N = self.nrow
        if joint:
            vc, vr = self._splitJoint(v, 'JvecBorn')
        else:
            vv = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape((N,)))
            vc, vr = (None, vv) if density else (vv, None)
        subs = self.system.subProblems
        down = {}

        def onGrid(i):
            'the perturbations (dc_f, db_f) on the grid of frequency i, float64 (N_f,) or None: one transfer and one pair of arrays per grid, not per frequency'
            ds = sv.preProcessors[i]
            if id(ds) not in down:
                dc, dr = (None if x is None else np.ascontiguousarray(np.asarray(ds * x, dtype=np.float64).ravel()) for x in (vc, vr))
                brho, bc = self._gridChains(i)
                db = None
                if dr is not None:
                    db = brho * dr
                elif bc is not None and stretch:
                    db = bc * dc
                down[id(ds)] = (dc, db)
            return down[id(ds)]

        def planes(i):
            dc, db = onGrid(i)
            if dc is None:
                return buoyancyPlanes(subs[i], db)
            if stretch:
                return velocityPlanes(subs[i], dc, db)
            return massPlanes(subs[i], dc) if db is None else massPlanes(subs[i], dc) + buoyancyPlanes(subs[i], db)
        data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
        st = complex(self.system.scaleTerm)
        owned = self.ownedFreqs
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                per = {i: onGrid(i) for i in F.ownedFreqs}
                dcs = None if vc is None else {i: per[i][0] for i in per}
                dbs = None if all(per[i][1] is None for i in per) else {i: per[i][1] for i in per}
                data = device_survey._bornPlanesFromFields(self, F, dbs, dc=dcs, stretch=stretch or vc is None)
                return (parallel.allreduce_sum(data) if self._sharded else data).ravel()
            qv = [applyPlanes(planes(i), np.conj(np.asarray(F[i]) / st), subs[i].nz, subs[i].nx) / -complex(subs[i].premul) if i in owned else None
                  for i in range(sv.nfreq)]
            for ifreq, uB in self._solveOwned(qv):
                uB = np.asarray(uB)
                if sv.mode == 'fixed':
                    data[:, :, ifreq] = sv.rVec(0, ifreq) * uB
                else:
                    for isrc in range(sv.nsrc):
                        data[:, isrc, ifreq] = sv.rVec(isrc, ifreq) * uB[:, isrc]
        if self._sharded:
            data = parallel.allreduce_sum(data)
        return data.ravel()

    @staticmethod
    def _checkLinearisation(linearisation):
        if linearisation not in ('scaler', 'operator', 'full'):
            raise ValueError('linearisation is %r: \'scaler\', \'operator\' or \'full\'' % (linearisation,))

    @staticmethod
    def _checkParameter(parameter, linearisation, joint=False):
        """parameter is 'c' or 'rho'; the density has no scaler in the reference, so 'rho' needs linearisation='operator' (or 'full', which is the same there).
        joint: 'joint' is served too -- the stacked pair [c; rho], which has no scaler either"""
        if joint and isinstance(parameter, str) and parameter == 'joint':
            if linearisation not in ('operator', 'full'):
                raise ValueError('parameter=\'joint\' needs linearisation=\'operator\' or \'full\': the reference has no gradient scaler for the density')
            return
        if parameter not in ('c', 'rho'):
            raise ValueError('parameter is %r: \'c\' or \'rho\'' % (parameter,))
        if parameter == 'rho' and linearisation not in ('operator', 'full'):
            raise ValueError('parameter=\'rho\' needs linearisation=\'operator\': the reference has no gradient scaler for the density')

    def _buoyancyChain(self):
        "d b / d rho = -1 / rho^2 per cell, float64 (N,), at the density of the config: b = 1 / rho is what the operator is linear in"
        rho = np.broadcast_to(np.asarray(self.systemConfig['rho'], dtype=np.float64).ravel(), (self.nrow,))       # (a scalar rho is one value for every cell)
        return -1.0 / (rho * rho)

    def _splitJoint(self, v, what):
        "(v_c, v_rho), float64 (N,) each, of a stacked vector [v_c; v_rho] of parameter='joint'; ValueError unless it has 2 N entries"
        v = np.asarray(v)
        if v.size != 2 * self.nrow:
            raise ValueError('%s(parameter=\'joint\') takes the stacked vector [c; rho] of %d entries, not %d' % (what, 2 * self.nrow, v.size))
        v = np.asarray(v, dtype=np.float64).reshape((2 * self.nrow,))
        return np.ascontiguousarray(v[:self.nrow]), np.ascontiguousarray(v[self.nrow:])

    def _hasDensity(self):
        'the config gives the density: it is a parameter of its own.  Otherwise it follows the velocity, rho = 310 Re(c)^0.25 (Gardner)'
        return self.systemConfig.get('rho', None) is not None

    # ---- visco problems: the chain from (c, Q) to the complex velocity ----------------------------------------
    def _isVisco(self):
        'the system wrapper makes a complex velocity from c and Q per frequency (ViscoMultiFreq): the exact derivatives then run through `viscoChain`'
        return isinstance(self.system, ViscoMultiFreq)

    def _checkViscoParameter(self, parameter, linearisation, stacked=True):
        """True when parameter is 'Q' or the stacked 'cQ' and the call may go on (nothing else is left to check of it); False for every other parameter, which
        `_checkParameter` then checks as before.  ValueError: on a problem that has no Q, with the scaler (the reference has none for Q), 'cQ' inside a pair"""
        if not (isinstance(parameter, str) and parameter in ('Q', 'cQ')):
            return False
        if parameter == 'cQ' and not stacked:
            raise ValueError('parameter=\'cQ\' is the stacked vector [c; Q] and cannot be half of a pair: pairs are made of \'c\', \'Q\' and \'rho\'')
        if not self._isVisco():
            raise ValueError('parameter=%r is the quality factor of a visco problem (Helm2DViscoProblem): %s has no Q' % (parameter, type(self.system).__name__))
        if linearisation not in ('operator', 'full'):
            raise ValueError('parameter=%r needs linearisation=\'operator\' or \'full\': the reference has no gradient scaler for Q' % (parameter,))
        return True

    def _refuseViscoDiagonal(self, what):
        if self._isVisco():
            raise NotImplementedError('%s does not serve visco problems: the Hessian diagonals and blocks are not built with the chain from (c, Q) to the complex '
                                      'velocity' % (what,))

    def _viscoLambda(self, ifreq):
        "lam_f = ln(f / freqBase) / pi of `viscoChain` for a frequency of the wrapper, 0 where it does not disperse (no freqBase, or Q infinite everywhere)"
        sysw = self.system
        if not sysw.disperseFreqs:
            return 0.0
        f = complex(sysw.freqs[ifreq])
        if f.imag != 0.0:
            raise ValueError('a visco problem with dispersion (freqBase > 0) needs real frequencies: ln(f / freqBase) of the complex frequency %r is not what '
                             'the Kolsky-Futterman law is defined with' % (sysw.freqs[ifreq],))
        return float(np.log(f.real / float(sysw.freqBase)) / np.pi)

    def _viscoQ(self):
        'Q per cell, float64 (N,), as the wrapper has it: inf where the config gives none'
        return np.ascontiguousarray(np.broadcast_to(np.asarray(self.system.Q, dtype=np.float64).ravel(), (self.nrow,)))

    def _viscoChainOf(self, ifreq):
        '(gamma_f, chi_f) of `viscoChain` per cell at the current model'
        c = np.broadcast_to(np.asarray(self.systemConfig['c']).real.ravel(), (self.nrow,))
        return viscoChain(c, self._viscoQ(), self._viscoLambda(ifreq))

    def _splitStacked(self, v, what):
        "(v_c, v_Q), float64 (N,) each, of a stacked vector [v_c; v_Q] of parameter='cQ'; ValueError unless it has 2 N entries"
        v = np.asarray(v)
        if v.size != 2 * self.nrow:
            raise ValueError('%s(parameter=\'cQ\') takes the stacked vector [c; Q] of %d entries, not %d' % (what, 2 * self.nrow, v.size))
        v = np.asarray(v, dtype=np.float64).reshape((2 * self.nrow,))
        return np.ascontiguousarray(v[:self.nrow]), np.ascontiguousarray(v[self.nrow:])

    def _viscoHalves(self, v, parameter, what):
        "(v_c, v_Q) of a perturbation of 'c', 'Q' or 'cQ': float64 (N,) each, None for the half that is not perturbed"
        if parameter == 'cQ':
            return self._splitStacked(v, what)
        v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape((self.nrow,)))
        return (v, None) if parameter == 'c' else (None, v)

    def _JtvecVisco(self, resid, u, linearisation, parameter):
        """Jtvec(adjoint='transpose') of a visco problem for parameter 'c', 'Q' or 'cQ' once the refusals are past: float64 (N,), or [g_c; g_Q] (2N,), from ONE
        back-propagation per source and frequency.  t_f = w V_f^T P0 is the complex cell gradient with respect to the complex velocity (the mass term alone for
        'operator'), w = -conj(scaleTerm) / premul; the chain is applied per frequency, before the sum: g_c = Re sum_f gamma_f t_f, g_Q = Re sum_f chi_f t_f."""
        stretch = linearisation == 'full'
        adj = self.adjointSystem
        N = self.nrow
        wantC, wantQ = parameter in ('c', 'cQ'), parameter in ('Q', 'cQ')
        lams = [self._viscoLambda(i) for i in range(self.survey.nfreq)]
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                rd = self._hermitianResidual(resid)
                return device_survey.viscoGradientFromFields(self, F, self._deviceBackSources(rd), rd, adj, linearisation, parameter, self._viscoQ(), lams)
            g = np.zeros(2 * N if parameter == 'cQ' else N, dtype=np.complex128)
            st = complex(self.system.scaleTerm)
            qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
            for ifreq, uB in self._solveOwned(qb, adj):
                op = self.system.subProblems[ifreq]
                P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx)
                t = (-np.conj(st) / complex(op.premul)) * velocityAdjoint(op, P, stretch=stretch)
                gamma, chi = self._viscoChainOf(ifreq)
                if wantC:
                    g[:N] += gamma * t
                if wantQ:
                    g[-N:] += chi * t
        if self._sharded:
            g = parallel.allreduce_sum(g)
        return g.real.copy()

    def _JvecBornVisco(self, v, u, linearisation, parameter):
        """JvecBorn of a visco problem for parameter 'c', 'Q' or 'cQ' once the refusals are past: the derivative of dpred along real (v_c, v_Q) is the
        derivative along the complex perturbation gamma_f v_c + chi_f v_Q of the complex velocity of frequency f -- one set of planes and one Born solve."""
        sv = self.survey
        vc, vQ = self._viscoHalves(v, parameter, 'JvecBorn')
        lams = [self._viscoLambda(i) for i in range(sv.nfreq)]
        stretch = linearisation == 'full'
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                data = device_survey.viscoBornFromFields(self, F, vc, vQ, linearisation, self._viscoQ(), lams)
            else:
                data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
                owned = self.ownedFreqs
                st = complex(self.system.scaleTerm)
                subs = self.system.subProblems

                def source(i):
                    gamma, chi = self._viscoChainOf(i)
                    dcz = (0 if vc is None else gamma * vc) + (0 if vQ is None else chi * vQ)
                    C = velocityPlanes(subs[i], dcz) if stretch else massPlanes(subs[i], dcz)
                    return applyPlanes(C, np.conj(np.asarray(F[i]) / st), subs[i].nz, subs[i].nx) / -complex(subs[i].premul)
                qv = [source(i) if i in owned else None for i in range(sv.nfreq)]
                for ifreq, uB in self._solveOwned(qv):
                    uB = np.asarray(uB)
                    if sv.mode == 'fixed':
                        data[:, :, ifreq] = sv.rVec(0, ifreq) * uB
                    else:
                        for isrc in range(sv.nsrc):
                            data[:, isrc, ifreq] = sv.rVec(isrc, ifreq) * uB[:, isrc]
        if self._sharded:
            data = parallel.allreduce_sum(data)
        return data.ravel()

    def _requireOperatorLinearisation(self, what):
        """linearisation='operator' serves Helm2DProblem with MiniZephyr / MiniZephyrHD on a single grid and an explicit density: everything else is refused
        here with the reason"""
        self._requireFullLinearisation(what)
        if not self._hasDensity():
            raise NotImplementedError('%s needs an explicit `rho` in the config: without one the Gardner density follows c, and its sensitivity is not built '
                                      '(linearisation=\'full\' carries it)' % (what,))

    def _requireFullLinearisation(self, what):
        """linearisation='full' serves Helm2DProblem with MiniZephyr / MiniZephyrHD on a single grid, with an explicit density or the default one -- and, with the
        config key eurusDerivatives, Eurus / EurusHD where eps == delta (`_eurusServed`), with the config key kyDerivatives the 2.5-D composite of MiniZephyr
        operators (`_kyServed`): everything else is refused here with the reason"""
        from .minizephyr import MiniZephyr
        from .discretization import DiscretizationWrapper
        self._refuseMultiscale(what)
        if self._isVisco() and not getattr(self, '_viscoDerivatives', False):
            # opt-in: with the key parameter='c' means d/dc at fixed Q through the chain; without it a visco problem is refused as it always was
            raise NotImplementedError('%s does not serve visco problems unless the config sets viscoDerivatives=True: the exact derivatives then run through the chain '
                                      'factor of the complex velocity with respect to c and Q (frechet.viscoChain)' % (what,))
        if self._isVisco() and not self._hasDensity():
            raise NotImplementedError('%s on a visco problem needs an explicit `rho` in the config: the default density rho = 310 Re(c~)^0.25 (Gardner) is not '
                                      'holomorphic in the complex velocity c~, and the chain from (c, Q) runs through the holomorphic derivative' % (what,))
        sub = self.system.subProblems[0] if self.system.subProblems else None
        if sub is not None and isinstance(sub, DiscretizationWrapper):
            if not getattr(self, '_kyDerivatives', False):
                raise NotImplementedError('%s does not serve the 2.5-D composite: the stored fields are the ky SUM, the exact derivative needs the fields per ky' % (what,))
            self._requireKyDerivatives(what, sub)
            return
        if self._eurusServed():
            if not all(op.elliptical for op in self.system.subProblems):
                raise NotImplementedError('%s on %s needs eps == delta in every cell: where they differ the two fields are coupled, and the coupled 2N x 2N system '
                                          '[[M1, M2], [M3, M4]] has no transposed solve' % (what, type(sub).__name__))
            return
        if sub is not None and not (isinstance(sub, MiniZephyr) and getattr(sub, 'ny', None) is None):
            raise NotImplementedError('%s serves the 2-D MiniZephyr operators: %s assembles its mass term differently' % (what, type(sub).__name__))

    # ---- 2.5-D problems: the exact derivatives from the fields per ky ---------------------------------------------
    # d = st R sum_k conj(u^_k), u^_k = A_k^-1 premul_k q, st the product of the wrapper's and the composite's scale terms: the derivative is a sum over ky of
    # the 2-D expressions of the SAME ky -- the maps of frechet.py on the ky sub-operator (its ky and its premul, the quadrature weight) and the weight
    # w_fk = -conj(st) / premul_k.  DESIGN.md 11t has the derivation with the conjugations written out.
    def _kyServed(self):
        'the config sets kyDerivatives=True and the operators are 2.5-D composites: the exact routes run per ky.  Without the key they are refused as they always were.'
        from .discretization import DiscretizationWrapper
        if not getattr(self, '_kyDerivatives', False):
            return False
        subs = self.system.subProblems
        return bool(subs) and isinstance(subs[0], DiscretizationWrapper)

    def _requireKyDerivatives(self, what, sub):
        'what kyDerivatives=True does not serve, refused with the reason: visco composites, a cmin that follows the model, ky sub-operators other than 2-D MiniZephyr'
        from .minizephyr import MiniZephyr, MiniZephyr25D
        if self._isVisco():
            raise NotImplementedError('%s with kyDerivatives does not serve visco problems (Helm25DViscoProblem): the chain from (c, Q) to the complex velocity is not '
                                      'built into the per-ky routes' % (what,))
        if self.systemConfig.get('cmin', None) is None:
            raise NotImplementedError('%s with kyDerivatives needs an explicit `cmin` in the config: without one the cross-line wavenumbers follow min(c), the quadrature '
                                      'nodes move with the model and the data are not differentiable in c' % (what,))
        if not (isinstance(sub, MiniZephyr25D) and isinstance(sub.Disc, type) and issubclass(sub.Disc, MiniZephyr) and getattr(sub, 'ny', None) is None):
            raise NotImplementedError('%s with kyDerivatives serves MiniZephyr25D over the 2-D MiniZephyr operators: %s assembles its mass term differently'
                                      % (what, type(sub).__name__))

    def _refuseKy(self, what, why):
        if self._kyServed():
            raise NotImplementedError('%s does not serve the 2.5-D composite: %s' % (what, why))

    def _kyScale(self, ifreq):
        "st of a frequency: the wrapper's scaleTerm times the composite's own (e^{i pi} / (4 pi) times the config's), which `_solveOwned` never shows apart"
        return complex(self.system.scaleTerm) * complex(self.system.subProblems[ifreq].scaleTerm)

    def _kyFieldsHost(self, ifreq, q):
        """(nky, N, nsrc) complex128: the forward fields of frequency ifreq PER ky on the host, st * (sub_k * q) = st conj(u^_k) for every ky sub-operator --
        their sum over ky is fields()[ifreq].  q: the frequency's source matrix."""
        st = self._kyScale(ifreq)
        return np.stack([st * np.asarray(sub * q) for sub in self.system.subProblems[ifreq].subProblems])

    def _kyBlocks(self, F, ifreq):
        '(nky, N, nsrc) of a host list of per-ky fields, checked: a list of ky SUMS is refused'
        nky = len(self.system.subProblems[ifreq].subProblems)
        Fk = np.asarray(F[ifreq])
        if Fk.ndim != 3 or Fk.shape[0] != nky:
            raise ValueError('the exact derivatives of a 2.5-D problem need the forward fields per ky, (nky, N, nsrc) per frequency: fields(perKy=True) / '
                             'fieldsDevice(perKy=True), not the ky sum of shape %s' % (Fk.shape,))
        return Fk

    def _kyGradientHost(self, resid, F, adj, stretch, wantC, wantB):
        """(g_c, g_b) complex (N,) each (None where not wanted), before the real part and the all-reduce: sum_f sum_k w_fk (V_k^T P_k, L_k^T P_k), P_k the nine lag
        products of z_k = A_k^-T premul_k R^H r against u^_k of the SAME ky, w_fk = -conj(st) / premul_k; stretch False: the mass term of V alone"""
        N = self.nrow
        gc = np.zeros(N, dtype=np.complex128) if wantC else None
        gb = np.zeros(N, dtype=np.complex128) if wantB else None
        qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
        for ifreq in self.ownedFreqs:
            st = self._kyScale(ifreq)
            Fk = self._kyBlocks(F, ifreq)
            for k, (sub, asub) in enumerate(zip(self.system.subProblems[ifreq].subProblems, adj.subProblems[ifreq].subProblems)):
                z = np.conj(np.asarray(asub * qb[ifreq]))          # (sub * q is conj(A^-T premul q))
                P = lagProducts(z, np.conj(Fk[k] / st), sub.nz, sub.nx)
                w = -np.conj(st) / complex(sub.premul)
                if wantC:
                    gc += w * velocityAdjoint(sub, P, stretch=stretch)
                if wantB:
                    gb += w * buoyancyAdjoint(sub, P)
        return gc, gb

    def _JtvecKy(self, resid, u, linearisation, parameter):
        """Jtvec(adjoint='transpose') of a 2.5-D problem with the resolved 'operator' or 'full' once the refusals are past: float64 (N,), or [g_c; g_rho] (2 N,) for
        'joint', from ONE back-propagation per source, frequency and ky"""
        stretch = linearisation == 'full'
        chain = self._gardnerChain() if parameter == 'c' and stretch else None          # (the density follows c: the buoyancy gradient joins through d b / d c)
        wantC, wantB = parameter in ('c', 'joint'), parameter in ('rho', 'joint') or chain is not None
        adj = self.adjointSystem
        N = self.nrow
        with self._forwardFields(u, perKy=True) as F:
            if isinstance(F, DeviceFields):
                rd = self._hermitianResidual(resid)
                g = device_survey.kyGradientFromFields(self, F, self._deviceBackSources(rd), rd, adj, stretch, wantC, wantB)
                gc, gb = g[:N], g[N:]
            else:
                gc, gb = self._kyGradientHost(resid, F, adj, stretch, wantC, wantB)
                g = np.concatenate([np.zeros(N) if x is None else x for x in (gc, gb)])
                if self._sharded:
                    g = parallel.allreduce_sum(g)
                gc, gb = g[:N].real, g[N:].real
        if parameter == 'joint':
            return np.concatenate((gc, self._buoyancyChain() * gb))
        if parameter == 'rho':
            return self._buoyancyChain() * gb
        return np.array(gc) if chain is None else gc + chain * gb

    def _JvecBornKy(self, u, dc, db, stretch):
        """JvecBorn of a 2.5-D problem with 'operator' or 'full' once the refusals are past: the planes V_k[dc] (stretch False: their mass term) + L_k[db] of every
        ky sub-operator applied to u^_k of the SAME ky, solved through A_k and summed -- dc / db (N,) float64, either may be None.  (nrec, nsrc, nfreq)."""
        sv = self.survey
        with self._forwardFields(u, perKy=True) as F:
            if isinstance(F, DeviceFields):
                return device_survey.kyBornFromFields(self, F, dc, db, stretch)
            data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)

            def planes(sub):
                if dc is None:
                    return buoyancyPlanes(sub, db)
                if stretch:
                    return velocityPlanes(sub, dc, db)
                return massPlanes(sub, dc) if db is None else massPlanes(sub, dc) + buoyancyPlanes(sub, db)
            for ifreq in self.ownedFreqs:
                st = self._kyScale(ifreq)
                Fk = self._kyBlocks(F, ifreq)
                uB = None
                for k, sub in enumerate(self.system.subProblems[ifreq].subProblems):
                    qv = applyPlanes(planes(sub), np.conj(Fk[k] / st), sub.nz, sub.nx) / -complex(sub.premul)
                    uk = np.asarray(sub * qv)
                    uB = uk if uB is None else uB + uk
                uB = st * uB
                if sv.mode == 'fixed':
                    data[:, :, ifreq] = sv.rVec(0, ifreq) * uB
                else:
                    for isrc in range(sv.nsrc):
                        data[:, isrc, ifreq] = sv.rVec(isrc, ifreq) * uB[:, isrc]
        return data

    def _eurusServed(self):
        """the config sets eurusDerivatives=True and the operators are 2-D Eurus / EurusHD on one grid: the exact adjoint and the exact derivatives run through M1^T
        and the maps of frechet.eurusPlanes.  Without the key an Eurus problem is refused as it always was."""
        from .eurus import Eurus
        if not getattr(self, '_eurusDerivatives', False):
            return False
        sub = self.system.subProblems[0] if self.system.subProblems else None
        return sub is not None and isinstance(sub, Eurus)

    def _refuseEurus(self, what, why):
        if self._eurusServed():
            raise NotImplementedError('%s does not serve Eurus problems: %s' % (what, why))

    def _eurusGradientHost(self, resid, F, adj):
        """(g_c, g_b) complex (N,) each, before the real part and the all-reduce: sum_f w_f (V_f^T P_f, L_f^T P_f) of an Eurus problem on the host, P_f the nine lag
        products of the transposed back-propagation against the unscaled forward solves, the centre plane on the boundary lines included (an edge row of M1
        keeps a centre entry that depends on the model), w_f = -conj(scaleTerm) / premul"""
        N = self.nrow
        st = complex(self.system.scaleTerm)
        edges = bool(getattr(self, '_eurusEdgeTerms', True))          # (False only in tests: what the result is without the edge rows' derivative)
        gc, gb = np.zeros(N, dtype=np.complex128), np.zeros(N, dtype=np.complex128)
        qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
        for ifreq, uB in self._solveOwned(qb, adj):
            op = self.system.subProblems[ifreq]
            P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx, edges=edges)
            tc, tb = eurusAdjoint(op, P, edges=edges)
            w = -np.conj(st) / complex(op.premul)
            gc += w * tc
            gb += w * tb
        return gc, gb

    def _resolveLinearisation(self, linearisation, parameter, what):
        """the linearisation a route runs with, once what it does not serve is refused: 'full' with parameter='rho' is 'operator' -- the density derivative
        leaves nothing out -- and needs the density to be a parameter of its own"""
        what = '%s(linearisation=%r)' % (what, linearisation)
        if parameter == 'joint' and self._isVisco():
            self._requireFullLinearisation(what)              # (what refuses the operator itself says so first)
            raise NotImplementedError('%s with parameter=\'joint\' does not serve visco problems: the stacked (c, rho) routes are not built with the chain through '
                                      'the complex velocity (parameter \'cQ\' and \'rho\' are served, one call each)' % (what,))
        if parameter == 'joint':
            # [c; rho] stacked: what 'full' serves, and the density a parameter of its own; 'operator' stays 'operator' (the stretch parts left out of the c half)
            self._requireFullLinearisation(what)
            if not self._hasDensity():
                raise NotImplementedError('%s with parameter=\'joint\' needs an explicit `rho` in the config: without one the density follows c and is '
                                          'not a free parameter' % (what,))
            return 'full' if self._eurusServed() else linearisation
        if linearisation == 'operator':
            self._requireOperatorLinearisation(what)
            if self._eurusServed():
                return 'full'                                 # (the C-PML does not depend on c: the mass term is the whole velocity derivative)
        elif linearisation == 'full':
            self._requireFullLinearisation(what)
            if parameter == 'rho':
                if not self._hasDensity():
                    raise NotImplementedError('%s with parameter=\'rho\' needs an explicit `rho` in the config: without one the density follows c and is '
                                              'not a free parameter' % (what,))
                return 'operator'
        return linearisation

    def _gardnerChain(self):
        'd b / d c per cell of the default density at the current model, float64 (N,); None where the config gives the density'
        return None if self._hasDensity() else gardnerChain(np.broadcast_to(np.asarray(self.systemConfig['c']).ravel(), (self.nrow,)))

    def _hermitianResidual(self, resid):
        """resid' with R_s^T resid'_s = R_s^H resid_s, for the device pipelines (which build R_s^T r): a receiver matrix is diag(srTerms) R0 with R0 the real
        columns of the source generator, so resid' = resid (.) conj(srTerms) / srTerms per receiver (0 where the term is 0: that row of R is zero).  A
        generator with complex columns has no such form and is refused."""
        ph = self._hermitianPhase()
        return resid if ph is None else resid * ph[:, None, None]

    def _hermitianPhase(self):
        "conj(srTerms) / srTerms per receiver, (nrec,) complex128: the factor of `_hermitianResidual`; None where the receiver terms are real (nothing to do)"
        sv = self.survey
        t = np.asarray(sv.srTerms, dtype=np.complex128).ravel()
        if not np.any(t.imag):
            return None
        Rm = sp.csr_matrix(sv.rVec(0, 0))
        rows = np.repeat(np.arange(Rm.shape[0]), np.diff(Rm.indptr))
        base = Rm.data * np.conj(t[rows])
        if np.any(np.abs(base.imag) > 1e-12 * np.abs(base)):
            raise NotImplementedError("linearisation='operator' on the device needs a source generator with real receiver columns (complex receiver terms are served)")
        nz = t != 0
        ph = np.zeros_like(t)
        ph[nz] = np.conj(t[nz]) / t[nz]
        return ph

    @contextlib.contextmanager
    def _forwardFields(self, u, perKy=False):
        """`with self._forwardFields(u) as F`: what the exact-adjoint routes read the forward fields from -- a DeviceFields as it is (checked), a list of host
        arrays as a list, None -> a DeviceFields solved now where the device path serves, released when the block is left whatever happened in it, else a
        host list with the owned frequencies' fields (None elsewhere).  perKy (the exact routes of a 2.5-D problem): the fields of every ky apart -- a store of
        fieldsDevice(perKy=True) (the ky-SUM store is refused with ValueError), or a host list of (nky, N, nsrc) arrays."""
        if self._multiscaleServed() and not isinstance(u, DeviceFields) and (u is not None or not self._deviceGradientAvailable()):
            yield self._ownGridFields(u)
        elif isinstance(u, DeviceFields):
            u.checkCurrent(self, perKy=perKy)
            yield u
        elif u is not None:
            yield list(u)
        elif perKy and self._deviceGradientAvailable():
            yield device_survey.liveKyFields(self)          # (no store: the pipelines solve the fields of a ky into their workspace just before they use them)
        elif self._deviceGradientAvailable():
            F = self.fieldsDevice()
            try:
                yield F
            finally:
                F.release()
        elif perKy:
            uF = [None] * self.survey.nfreq
            qf = self.survey.getSources()
            for ifreq in self.ownedFreqs:
                uF[ifreq] = self._kyFieldsHost(ifreq, device_survey._ofFrequency(qf, ifreq))
            yield uF
        else:
            uF = [None] * self.survey.nfreq
            pps = self.survey.postProcessors
            for ifreq, uf in self._solveOwned(self.survey.getSources()):
                uF[ifreq] = pps[ifreq](uf)
            yield uF

    def _deviceBackSources(self, resid):
        """the back-sources as the device pipelines take them: a fixed array keeps its host-built ones (sparse, sent up as triplets); those of an array that
        moves with the source are made on the device from the residual samples (helm_rhs_from_samples_device): None"""
        sv = self.survey
        return sv.getResidualSources(resid) if sv.mode == 'fixed' else None

    def _JtvecTranspose(self, resid, u, linearisation='scaler', parameter='c'):
        "Jtvec(adjoint='transpose') once the model is current and `resid` is (nrec, nsrc, nfreq)"
        self._refuseMultiscale("Jtvec(adjoint='transpose')")
        self._refuseMultiscaleScaler("Jtvec(adjoint='transpose')", linearisation)
        linearisation = self._resolveLinearisation(linearisation, parameter, 'Jtvec')
        if self._multiscaleServed():
            return self._JtvecMultiscale(resid, u, linearisation, parameter)
        if linearisation != 'scaler' and self._kyServed():
            return self._JtvecKy(resid, u, linearisation, parameter)
        if parameter == 'joint':
            return self._JtvecJoint(resid, u, linearisation)
        if linearisation != 'scaler' and parameter in ('c', 'Q', 'cQ') and self._isVisco():
            return self._JtvecVisco(resid, u, linearisation, parameter)
        exact = linearisation == 'operator'
        full = linearisation == 'full'
        density = parameter == 'rho'
        adj = self.adjointSystem
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                if exact or full:
                    resid = self._hermitianResidual(resid)
                if density:
                    return self._buoyancyChain() * device_survey.gradientFromFields(self, F, self._deviceBackSources(resid), resid, system=adj, linearisation=linearisation,
                                                                                    parameter='rho')
                if full:
                    return device_survey.gradientFromFields(self, F, self._deviceBackSources(resid), resid, system=adj, linearisation='full', chain=self._gardnerChain())
                return device_survey.gradientFromFields(self, F, self._deviceBackSources(resid), resid, system=adj, linearisation=linearisation)
            g = np.zeros(self.nrow, dtype=np.complex128)
            if (full or density) and self._eurusServed():
                gc, gb = self._eurusGradientHost(resid, F, adj)
                chain = None if density else self._gardnerChain()
                g = gb if density else (gc if chain is None else gc + chain * gb)
            elif full:
                # the lag products of parameter='rho' against V^T, the transpose of frechet.velocityPlanes; where the density follows c the buoyancy
                # gradient L^T P joins through the real chain d b / d c
                st = complex(self.system.scaleTerm)
                chain = self._gardnerChain()
                qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
                for ifreq, uB in self._solveOwned(qb, adj):
                    op = self.system.subProblems[ifreq]
                    P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx)
                    gf = velocityAdjoint(op, P)
                    if chain is not None:
                        gf = gf + chain * buoyancyAdjoint(op, P)
                    g += (-np.conj(st) / complex(op.premul)) * gf
            elif density:
                # z_s = A^-T premul R_s^H r_s and u^_s from the scaled, conjugated arrays the solves and the host fields are; g_b = Re -(conj(st) / premul) L^T P
                st = complex(self.system.scaleTerm)
                qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
                for ifreq, uB in self._solveOwned(qb, adj):
                    op = self.system.subProblems[ifreq]
                    P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx)
                    g += (-np.conj(st) / complex(op.premul)) * buoyancyAdjoint(op, P)
            elif exact:
                # the back-sources are R_s^H r_s = conj(R_s^T conj(r_s)); the solves come back scaled (scaleTerm uB), the host fields are scaleTerm U: one
                # scaleTerm of the product stays in the weight, the other is divided out
                st = complex(self.system.scaleTerm)
                qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
                for ifreq, uB in self._solveOwned(qb, adj):
                    op = self.system.subProblems[ifreq]
                    w = -np.conj(operatorWeight(op)) / (st * np.conj(complex(op.premul)))
                    g += w * (np.asarray(F[ifreq]) * massStencil(maskInterior(np.asarray(uB), op.nz, op.nx), op.nz, op.nx)).sum(axis=1)
            else:
                for ifreq, uB in self._solveOwned(self.survey.getResidualSources(resid), adj):
                    g += self.gradientScaler(ifreq) * (np.asarray(F[ifreq]) * uB).sum(axis=1)
        if self._sharded:
            g = parallel.allreduce_sum(g)
        return self._buoyancyChain() * g.real if density else g.real

    def _JtvecJoint(self, resid, u, linearisation):
        """Jtvec(adjoint='transpose', parameter='joint') once the refusals are past: [g_c; g_rho], float64 (2N,), from ONE back-propagation per source and
        frequency.  Both gradients are transposes applied to the same nine lag products P0 = lag(z, u^): g_c = Re w V^T P0 (the mass term alone for
        'operator'), g_rho = (-1 / rho^2) Re w L^T P0, w = -conj(scaleTerm) / premul."""
        stretch = linearisation == 'full'
        adj = self.adjointSystem
        N = self.nrow
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                rd = self._hermitianResidual(resid)
                g = device_survey.jointGradientFromFields(self, F, self._deviceBackSources(rd), rd, adj, linearisation)
                g[N:] *= self._buoyancyChain()
                return g
            g = np.zeros(2 * N, dtype=np.complex128)
            st = complex(self.system.scaleTerm)
            if self._eurusServed():
                g[:N], g[N:] = self._eurusGradientHost(resid, F, adj)
            else:
                qb = [q.conj() for q in self.survey.getResidualSources(np.conj(resid))]
                for ifreq, uB in self._solveOwned(qb, adj):
                    op = self.system.subProblems[ifreq]
                    P = lagProducts(np.conj(np.asarray(uB) / st), np.conj(np.asarray(F[ifreq]) / st), op.nz, op.nx)
                    w = -np.conj(st) / complex(op.premul)
                    g[:N] += w * velocityAdjoint(op, P, stretch=stretch)
                    g[N:] += w * buoyancyAdjoint(op, P)
        if self._sharded:
            g = parallel.allreduce_sum(g)
        g = g.real.copy()
        g[N:] *= self._buoyancyChain()
        return g

    def JvecBorn(self, m=None, v=None, u=None, linearisation='scaler', parameter='c'):
        """Born data of the model perturbation v from the forward fields, the ravel of (nrec, nsrc, nfreq) complex128:

            dd[:, s, f] = conj(R_s) . scaleTerm S_f( conj(v (.) w_f (.) uF_s) ),   S_f q = conj(A_f^-1 premul q),  w_f = gradientScaler(f),  uF_s = scaleTerm S_f qf_s

        one virtual source per SOURCE and frequency.  It is the exact adjoint of Jtvec(adjoint='transpose'): <JvecBorn v, r> = <v, Jtvec(r)> under
        <a, b> = Re sum conj(a) b, to solver accuracy.  (`Jvec` is the reference's one-column outer-product approximation, kept as it is; it has no such
        property.)  Only the forward factors are used -- those fieldsDevice has just made.  u a DeviceFields: per stored item the virtual sources are
        made from the slice on the device, solved there and sampled through the conjugated receiver CSR; nrec x k samples come down per item.  u None
        with the device path: fieldsDevice() internally, released afterwards.  u a list of host arrays, or no device path: numpy.  Sharded ranks end
        in one all-reduce.  A multiscale pairing raises NotImplementedError unless the config sets multiscaleDerivatives=True: then ('operator' / 'full') the
        perturbation goes down once per grid, dc_f = S_f v, the buoyancy perturbation is formed there (-(S_f v_rho) / rho_f^2, or Gardner's chain at c_f), and
        the planes, the Born solve and the sampling are those of the grid of frequency f -- the exact adjoint of Jtvec on that pairing (see there).

        linearisation='scaler' (default) is the above: the reference's convention, delta A ~ diag(v (.) w_f).  It is NOT the derivative of `dpred`.
        linearisation='operator': the derivative of `dpred`, d/dh dpred(m + h v) at h = 0, from what the operator is assembled from:

            dd[:, s, f] = R_s . scaleTerm conj(-A_f^-1 delta A u^_s),   delta A u^ = mask_int (.) M0(delta K (.) u^),   delta K = -2 omega_d^2 v / (c^3 rho)

        u^_s = A_f^-1 premul qf_s (the conjugate of the unscaled forward solve), M0 the constant 9-point stencil of the mass weights (centre 0.6248, edges
        0.09381, corners 1.297e-6), mask_int zero on the four boundary lines (their rows are +-identity), omega_d = 2 pi f - i / tau.  v is real.  It is
        the exact adjoint of Jtvec(adjoint='transpose', linearisation='operator').  The dependence of the PML stretch on c is left out: the derivative is
        exact for perturbations that vanish in the absorbing layers (inside them it is the mass-term part only; linearisation='full' is exact there too).
        `_requireOperatorLinearisation` lists what it serves.
        linearisation='full': the TOTAL derivative of `dpred` with respect to the velocity, v non-zero anywhere.  The absorbing layers lie inside the grid and
        their stretch factors X, Z, px, pz are functions of the velocity of the row's own cell; without `rho` in the config the density follows c as well
        (Gardner, rho = 310 Re(c)^0.25).  A row is star(row_i, bn, Kn), linear in (row, Kn) and in (bn, Kn), so the nine planes of delta A are

            star(v_i d row_i / dc, bn[b], Kn_k = (-2 omega_d^2 / c_j^3) b_j v_j)  +  star(row_i, bn[db], Kn_k = kappa_j db_j),   db = -0.25 b / Re(c) (.) v

        (frechet.velocityPlanes; boundary rows zero; the second star only without `rho`; the Kn of the first one alone is 'operator').  Then
        dd[:, s, f] = R_s . scaleTerm conj(-A_f^-1 (delta A) u^_s) as for parameter='rho' below.  The exact adjoint of
        Jtvec(adjoint='transpose', linearisation='full'); the same routes as 'operator', and a config without `rho` is served
        (`_requireFullLinearisation`).

        parameter='c' (default): all of the above.  parameter='rho' (needs linearisation='operator'): v is a density perturbation and the result is
        d/dh dpred(c, rho + h v) at h = 0, at the rho of the config with c held fixed (m stays the velocity).  Every interior row of the operator is linear
        in the buoyancy b = 1 / rho (mass terms and stiffness averages alike) and the PML stretch does not depend on rho, so nothing is left out: with
        db = -v / rho^2 and L_f[db] the nine planes of frechet.buoyancyPlanes (boundary rows zero),

            dd[:, s, f] = R_s . scaleTerm conj(-A_f^-1 (delta A) u^_s),   (delta A) u^ = sum_k L_f[db]_k (.) shift_k(u^)

        exact everywhere, the absorbing layers and the boundary lines included.  The exact adjoint of Jtvec(..., parameter='rho'); the same routes.

        parameter='joint' ('operator' or 'full', an explicit `rho`): v = [v_c; v_rho] of 2 N entries, the derivative of dpred along both at once from one Born
        solve: delta A = V_f[v_c] + L_f[-v_rho / rho^2] is one set of planes (for 'operator' the mass term of V_f alone).  The exact adjoint of
        Jtvec(..., parameter='joint').

        A visco problem with 'operator' or 'full' (served and refused as in `Jtvec`): parameter 'c', 'Q' or the stacked 'cQ' (v = [v_c; v_Q] of 2 N entries) is
        the derivative of dpred along real perturbations of c and of Q, one Born solve: delta A = V_f[gamma_f v_c + chi_f v_Q], the planes of a COMPLEX
        perturbation of the complex velocity of frequency f (frechet.viscoChain; `_JvecBornVisco`)."""
        self._requirePaired()
        if v is None:
            raise Exception('Actually, JvecBorn requires a perturbation vector')
        self._checkLinearisation(linearisation)
        if not self._checkViscoParameter(parameter, linearisation):
            self._checkParameter(parameter, linearisation, joint=True)
        self.updateModel(m)
        self._refuseMultiscale('JvecBorn')
        self._refuseMultiscaleScaler('JvecBorn', linearisation)
        linearisation = self._resolveLinearisation(linearisation, parameter, 'JvecBorn')
        if self._multiscaleServed():
            return self._JvecBornMultiscale(v, u, linearisation, parameter)
        if linearisation != 'scaler' and parameter in ('c', 'Q', 'cQ') and self._isVisco():
            return self._JvecBornVisco(v, u, linearisation, parameter)
        exact = linearisation in ('operator', 'full')
        full = linearisation == 'full'
        density = parameter == 'rho'
        sv = self.survey
        joint = parameter == 'joint'
        if joint:
            # [v_c; v_rho]: dA = V[v_c] + L[db], db = -v_rho / rho^2 -- one set of planes, one Born solve ('operator': the mass term of V alone)
            pert, db = self._splitJoint(v, 'JvecBorn')
            db = self._buoyancyChain() * db
        else:
            pert = np.asarray(v).reshape((self.nrow,))
        if density:
            pert = self._buoyancyChain() * np.asarray(pert, dtype=np.float64)          # (db: the operator is linear in the buoyancy)
        elif full and not joint:
            pert = np.asarray(pert, dtype=np.float64)
            chain = self._gardnerChain()
            db = None if chain is None else chain * pert                                # (the buoyancy perturbation that goes with v: the density follows c)
        if exact and self._kyServed():
            if density:
                data = self._JvecBornKy(u, None, pert, False)
            else:
                data = self._JvecBornKy(u, np.asarray(pert, dtype=np.float64), db if (joint or full) else None, full)
            return (parallel.allreduce_sum(data) if self._sharded else data).ravel()
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                if joint:
                    data = device_survey.bornFromFields(self, F, pert, linearisation=linearisation, parameter='joint', db=db)
                elif density:
                    data = device_survey.bornFromFields(self, F, pert, linearisation=linearisation, parameter='rho')
                elif full:
                    data = device_survey.bornFromFields(self, F, pert, linearisation='full', db=db)
                else:
                    data = device_survey.bornFromFields(self, F, pert, linearisation=linearisation)
            else:
                data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
                owned = self.ownedFreqs
                if density or full or joint:
                    st = complex(self.system.scaleTerm)
                    subs = self.system.subProblems
                    if self._eurusServed():
                        edges = bool(getattr(self, '_eurusEdgeTerms', True))
                        planes = (lambda op: eurusPlanes(op, None, pert, edges=edges)) if density else (lambda op: eurusPlanes(op, pert, db, edges=edges))
                    elif joint and not full:
                        planes = lambda op: massPlanes(op, pert) + buoyancyPlanes(op, db)
                    else:
                        planes = (lambda op: buoyancyPlanes(op, pert)) if density else (lambda op: velocityPlanes(op, pert, db))
                    qv = [applyPlanes(planes(subs[i]), np.conj(np.asarray(F[i]) / st), subs[i].nz, subs[i].nx) / -complex(subs[i].premul)
                          if i in owned else None for i in range(sv.nfreq)]
                elif exact:
                    # F[i] = scaleTerm conj(u^): the scaleTerm is divided out of the virtual source and comes back with the solve (_solveOwned scales)
                    st = complex(self.system.scaleTerm)
                    subs = self.system.subProblems
                    qv = [massStencil((operatorWeight(subs[i]) * pert)[:, None] * np.conj(np.asarray(F[i]) / st), subs[i].nz, subs[i].nx, mask=True)
                          / -complex(subs[i].premul) if i in owned else None for i in range(sv.nfreq)]
                else:
                    qv = [np.conj((pert * np.asarray(self.gradientScaler(i)).ravel())[:, None] * np.asarray(F[i])) if i in owned else None for i in range(sv.nfreq)]
                for ifreq, uB in self._solveOwned(qv):
                    uB = np.asarray(uB)
                    if sv.mode == 'fixed':
                        Rm = sv.rVec(0, ifreq)
                        data[:, :, ifreq] = (Rm if exact else Rm.conj()) * uB
                    else:
                        for isrc in range(sv.nsrc):
                            Rm = sv.rVec(isrc, ifreq)
                            data[:, isrc, ifreq] = (Rm if exact else Rm.conj()) * uB[:, isrc]
        if self._sharded:
            data = parallel.allreduce_sum(data)
        return data.ravel()

    def Hvec(self, m=None, v=None, u=None, weights=None, linearisation='scaler', parameter='c', resid=None):
        """Gauss-Newton Hessian times v: Jtvec(JvecBorn(v) (.) weights, adjoint='transpose'), float64 (N,).  Symmetric and positive semi-definite as an
        operator on real vectors, because the two halves are exact adjoints.  weights: optional, real, non-negative, the shape (or ravel) of the data.
        Both halves read the same forward fields: two solves of nsrc columns per frequency, no forward re-solve; with u None the fields are solved once
        (into HBM where the device path serves) for both halves.  Needs the factors of A and of A^T side by side (see `adjointSystem`).
        linearisation: handed to both halves; with 'operator' this is the Gauss-Newton Hessian of 1/2 ||dpred - dobs||^2 for perturbations that vanish in the
        absorbing layers, with 'full' for any perturbation (with 'scaler' it is not).
        parameter: 'c' (default), 'rho', or a pair (input, output) handed to JvecBorn and Jtvec respectively -- ('c', 'rho') takes a velocity perturbation
        and returns the density block row of the Hessian, the transpose of ('rho', 'c').  Anything with 'rho' needs linearisation='operator' or 'full'.

        resid (default None: all of the above, unchanged): the data residual dpred(m) - dobs, the size of the data.  The result is then the FULL Newton Hessian
        of phi(m) = 1/2 ||dpred(m) - dobs||^2 times v: with g(m) = Jtvec(m, dpred(m) - dobs, adjoint='transpose', linearisation=, parameter=) at fixed dobs,
        d/dh g(m + h v) at h = 0.  Per frequency and source, with u the stored forward solve, lambda = A^-T (the back-source of resid) what the gradient solves,
        dA[v] the planes of the perturbation and du = -A^-1 dA[v] u the Born field, ONE more solve through A^T gives
        dlambda = A^-T (R^H R du - dA[v]^T lambda), and

            (H v)_i = -Re[ <dlambda, d_i A u> + <lambda, d_i A du> + <lambda, (d_i dA[v]) u> ]

        up to the scaleTerm and premul factors of Jtvec: the adjoint of the derivative applied to the lag products of (dlambda, u) and (lambda, du), plus the
        second derivative of the planes contracted with the lag products of (lambda, u) -- the gradient's own.  With an explicit density d^2 A / dc_i dc_j = 0 for
        i != j and that term is local to a cell (frechet.velocityCurvature); for parameter='rho' it is v (.) 2 / rho^3 (.) the buoyancy gradient.  The R^H R du part
        alone is the Gauss-Newton product: with resid = 0 the two agree.  Symmetric; NOT positive semi-definite in general -- the residual part has either
        sign, which is what a truncated-Newton iteration has to cope with.  Three solves of nsrc columns per frequency instead of two.
        Served: Helm2DProblem with MiniZephyr / MiniZephyrHD on one grid and an explicit `rho`; linearisation='full', and 'operator' (the stretch parts of both
        derivatives left out: exact for v that vanishes in the absorbing layers); parameter 'c', 'rho' or 'joint'; fixed and moving receiver arrays; u a DeviceFields or
        None with the device path (both store formats), host lists or no GPU: numpy.  linearisation='scaler' is no derivative and has no Hessian (ValueError); a parameter pair and a
        config without `rho` raise NotImplementedError (the mixed second derivatives are not local to a cell); `weights` together with `resid`: ValueError.

        parameter='joint' (not inside a pair; 'operator' or 'full'; an explicit `rho`): v = [v_c; v_rho] of 2 N entries, the result [H_c; H_rho] of 2 N entries in
        the units of 'c' and 'rho'.  resid None: the sum of the four blocks above from ONE Born solve and ONE back-solve per source and frequency -- the planes
        of the stacked perturbation are one set, V[v_c] + L[db] with db = -v_rho / rho^2.  With resid: d/dh of the joint gradient at (c + h v_c, rho + h v_rho),
        three solves -- the off-diagonal blocks of the Newton Hessian included, which no pair reaches.  A row is bilinear in its stretch factors (of c_i) and the
        averaged buoyancies and linear in the mass terms, so d^2 A / db^2 = 0 and d^2 A / dc db [p, beta] is `velocityPlanes` with beta in the place of the
        buoyancy (frechet.mixedPlanes); with P1 and P0 the lag products above,

            H_c   = Re w [ V^T P1 + velocityCurvature(P0, v_c) + M_c^T[db] P0 ]
            H_rho = (-1 / rho^2) (.) Re w [ L^T P1 + M_b^T[v_c] P0 ]  +  v_rho (.) 2 / rho^3 (.) Re w L^T P0

        M_c^T and M_b^T the transposes of the mixed derivative in its velocity and in its buoyancy argument (frechet.mixedAdjointC / mixedAdjointB; the second
        gathers v_c from the eight rows around a cell).  Hvec([p; 0], resid=r) is [H_cc p; H_rho,c p].

        A visco problem with resid None: parameter 'c', 'Q', 'rho', a pair of them, or the stacked 'cQ' (not inside a pair; v and the result of 2 N entries) --
        the composition of the two halves as above, two solves per source and frequency.  Hvec(resid=) raises NotImplementedError there: the second derivative
        of the chain from (c, Q) to the complex velocity is not built."""
        self._requirePaired()
        if v is None:
            raise Exception('Actually, Hvec requires a vector')
        self._checkLinearisation(linearisation)
        pin, pout = parameter if isinstance(parameter, (tuple, list)) and len(parameter) == 2 else (parameter, parameter)
        joint = isinstance(parameter, str) and parameter == 'joint'           # ('joint' inside a pair is no parameter: ValueError below)
        stacked = isinstance(parameter, str) and parameter == 'cQ'            # (and neither is 'cQ')
        for par in (pin, pout):
            if not self._checkViscoParameter(par, linearisation, stacked=stacked):
                self._checkParameter(par, linearisation, joint=joint)
        if resid is not None and linearisation == 'scaler':
            raise ValueError('linearisation=\'scaler\' is not the derivative of dpred and has no Hessian: Hvec(resid=) needs \'operator\' or \'full\'')
        if resid is not None and weights is not None:
            raise ValueError('Hvec(resid=) takes no data weights: the residual of a weighted misfit is the caller\'s to weigh')
        self.updateModel(m)
        self._refuseMultiscale('Hvec')
        self._refuseMultiscaleScaler('Hvec', linearisation)
        if resid is not None and self._multiscaleServed():
            raise NotImplementedError('Hvec(resid=) does not serve multiscale pairings: the second derivatives of the per-grid chains and the third solve are not '
                                      'built into the per-grid routes (resid=None, the Gauss-Newton product, is served)')
        for par in (pin, pout):
            self._resolveLinearisation(linearisation, par, 'Hvec')                      # (refusals before the fields are solved for both halves)
        if weights is not None:
            weights = np.asarray(weights)
            if np.iscomplexobj(weights) or weights.size != self.survey.nD or not np.all(weights >= 0):
                raise ValueError('weights are real, non-negative and of the size of the data (%d)' % (self.survey.nD,))
            weights = weights.astype(np.float64).ravel()
        if joint:
            self._splitJoint(v, 'Hvec')                                                 # (ValueError unless v is the stacked vector of 2 N entries)
        if stacked:
            self._splitStacked(v, 'Hvec')
        if resid is not None and self._isVisco():
            raise NotImplementedError('Hvec(resid=) does not serve visco problems: the second derivative of the chain from (c, Q) to the complex velocity, '
                                      'd^2 c~ / dQ^2 and d^2 c~ / dc dQ, is not built (resid=None, the Gauss-Newton product, is served)')
        if resid is not None:
            self._refuseKy('Hvec(resid=)', 'the second derivative of the ky operators and the third solve per ky are not built into the per-ky routes (resid=None, the '
                                           'Gauss-Newton product, is served)')
            self._refuseEurus('Hvec(resid=)', 'the second derivative of M1 and the transposed application of its planes are not built (resid=None, the Gauss-Newton '
                                              'product, is served)')
            if pin != pout:
                raise NotImplementedError('Hvec(resid=) serves one parameter: the mixed second derivative of the operator with respect to c and b is not local to a cell')
            if not self._hasDensity():
                raise NotImplementedError('Hvec(resid=) needs an explicit `rho` in the config: where the density follows c the buoyancy of a cell multiplies the '
                                          'stretch factors of its neighbours\' rows, and the second derivative of the operator is not local to a cell')
            resid = np.asarray(resid)
            if resid.size != self.survey.nD:
                raise ValueError('resid is of the size of the data (%d), not %d' % (self.survey.nD, resid.size))
            resid = resid.astype(np.complex128).reshape((self.survey.nrec, self.survey.nsrc, self.survey.nfreq))
            return self._HvecNewton(np.asarray(v, dtype=np.float64).reshape((2 * self.nrow if joint else self.nrow,)), u, resid,
                                    self._resolveLinearisation(linearisation, pin, 'Hvec'), pin)
        with self._forwardFields(u, perKy=linearisation != 'scaler' and self._kyServed()) as F:
            d = self.JvecBorn(None, v, u=F, linearisation=linearisation, parameter=pin)
            if weights is not None:
                d = d * weights
            return self.Jtvec(None, d, u=F, adjoint='transpose', linearisation=linearisation, parameter=pout)

    def _HvecNewton(self, p, u, resid, linearisation, parameter):
        """Hvec(resid=) once the model is current and the refusals are past: p float64 (N,), resid (nrec, nsrc, nfreq), the resolved linearisation.  The numpy
        route below follows `_JtvecTranspose` and the host branch of `JvecBorn` for scaleTerm, premul and conjugations: the host fields are scaleTerm conj(u^),
        a solve returns scaleTerm conj(A^-1 premul q) (A^-T through `adjointSystem`), and the weight of a frequency is -conj(scaleTerm) / premul."""
        sv = self.survey
        N = self.nrow
        density = parameter == 'rho'
        joint = parameter == 'joint'
        stretch = linearisation == 'full'
        adj = self.adjointSystem
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                rd = self._hermitianResidual(resid)
                return device_survey.newtonFromFields(self, F, p, self._deviceBackSources(rd), rd, adj, linearisation, parameter)
            st = complex(self.system.scaleTerm)
            subs = self.system.subProblems
            owned = self.ownedFreqs
            nf = sv.nfreq
            hermitian = lambda r: [q.conj() for q in sv.getResidualSources(np.conj(r))]          # (R_s^H r_s = conj(R_s^T conj(r_s)))
            unscaled = lambda a: np.conj(np.asarray(a) / st)
            if joint:
                pc, prho = p[:N], p[N:]
                db = self._buoyancyChain() * prho
                planes = (lambda op: velocityPlanes(op, pc, db)) if stretch else (lambda op: massPlanes(op, pc) + buoyancyPlanes(op, db))
            elif density:
                pert = self._buoyancyChain() * p
                planes = lambda op: buoyancyPlanes(op, pert)
            else:
                planes = (lambda op: velocityPlanes(op, p)) if stretch else (lambda op: massPlanes(op, p))
            # 1. lambda = A^-T premul R^H r, what the gradient solves
            lam = {i: unscaled(uB) for i, uB in self._solveOwned(hermitian(resid), adj)}
            # 2. the Born field du = -A^-1 dA[p] u^ and its samples
            C = {i: planes(subs[i]) for i in owned}
            uh = {i: unscaled(F[i]) for i in owned}
            qv = [applyPlanes(C[i], uh[i], subs[i].nz, subs[i].nx) / -complex(subs[i].premul) if i in owned else None for i in range(nf)]
            du, dd = {}, np.zeros((sv.nrec, sv.nsrc, nf), dtype=np.complex128)
            for i, uB in self._solveOwned(qv):
                uB = np.asarray(uB)
                du[i] = unscaled(uB)
                if sv.mode == 'fixed':
                    dd[:, :, i] = sv.rVec(0, i) * uB
                else:
                    for isrc in range(sv.nsrc):
                        dd[:, isrc, i] = sv.rVec(isrc, i) * uB[:, isrc]
            # 3. dlambda = A^-T (premul R^H R du - dA[p]^T lambda): the first part alone is the Gauss-Newton product
            qr = hermitian(dd)
            q3 = [np.asarray(qr[i].toarray()) - applyPlanesTransposed(C[i], lam[i], subs[i].nz, subs[i].nx) / complex(subs[i].premul) if i in owned else None
                  for i in range(nf)]
            g = np.zeros(2 * N if joint else N, dtype=np.complex128)
            g0 = np.zeros(N, dtype=np.complex128)
            for i, uB in self._solveOwned(q3, adj):
                op = subs[i]
                dlam = unscaled(uB)
                P1 = lagProducts(dlam, uh[i], op.nz, op.nx) + lagProducts(lam[i], du[i], op.nz, op.nx)
                P0 = lagProducts(lam[i], uh[i], op.nz, op.nx)          # (the gradient's own lag products)
                w = -np.conj(st) / complex(op.premul)
                if joint:
                    # the two mixed terms on the gradient's own lag products: M_c^T[db] P0 joins the c half, M_b^T[p_c] P0 the buoyancy half
                    g[:N] += w * (velocityAdjoint(op, P1, stretch=stretch) + velocityCurvature(op, P0, pc, stretch=stretch) + mixedAdjointC(op, P0, db, stretch=stretch))
                    g[N:] += w * (buoyancyAdjoint(op, P1) + mixedAdjointB(op, P0, pc, stretch=stretch))
                    g0 += w * buoyancyAdjoint(op, P0)
                elif density:
                    g += w * buoyancyAdjoint(op, P1)
                    g0 += w * buoyancyAdjoint(op, P0)
                else:
                    g += w * (velocityAdjoint(op, P1, stretch=stretch) + velocityCurvature(op, P0, p, stretch=stretch))
        if joint:
            g = np.concatenate((g[:N].real, self._buoyancyChain() * g[N:].real + prho * self._buoyancyCurvature() * g0.real))
        elif density:
            # b = 1 / rho: d b / d rho = -1 / rho^2 on the first two terms, d^2 b / d rho^2 = 2 / rho^3 times the buoyancy gradient for the third
            g = self._buoyancyChain() * g.real + p * self._buoyancyCurvature() * g0.real
        else:
            g = g.real
        return parallel.allreduce_sum(g) if self._sharded else g

    def _buoyancyCurvature(self):
        "d^2 b / d rho^2 = 2 / rho^3 per cell, float64 (N,), at the density of the config"
        rho = np.broadcast_to(np.asarray(self.systemConfig['rho'], dtype=np.float64).ravel(), (self.nrow,))
        return 2.0 / (rho * rho * rho)

    # ---- illumination / diagonal pseudo-Hessian ------------------------------------------------------------
    def illumination(self, m=None, u=None, kind='pseudoHessian', side='source', perFreq=False, linearisation='scaler', parameter='c'):
        """What an FWI gradient is divided by: float64 (N,), or (nfreq, N) with perFreq, every entry >= 0.  With uF[f] = fields()[f] and
        E_f[i] = sum_s |uF[f][i, s]|^2:

        kind 'energy':        sum_f E_f                                 (source-side illumination)
        kind 'pseudoHessian': sum_f |gradientScaler(f)|^2 (.) E_f       (the diagonal pseudo-Hessian of Shin, Jang & Min 2001)
        kind 'gaussNewton':   diag(J^T J), sources and receivers         (below)
        perFreq:              the terms of the sum over f, one row each (rows of frequencies other ranks own arrive through the all-reduce)

        side 'receiver': the same with the receiver array as sources, uR_f = scaleTerm * (sub_f * rVec(0, f).T) -- srTerms included, no tsTerms; fixed
        arrays only, and u must be None.  A preconditioned gradient is g / (H + lambda * H.max()).

        linearisation / parameter (kind 'pseudoHessian' only; the defaults are the weight above, which belongs to the 'scaler' gradient): the pseudo-Hessian
        diagonal of the derivative that Jtvec(adjoint='transpose', linearisation=, parameter=) is the gradient of,

            H_p[i] = |scaleTerm|^2 sum_f sum_s || (d A_f / d p_i) u^_s ||_2^2,     u^_s = A_f^-1 premul q_s,

        with d A_f / d p_i the planes of frechet.velocityPlanes along e_i ('full': mass term, PML stretch and the Gardner density where the config gives
        none), its mass term alone ('operator': the closed form |d K_i / d c|^2 S_i sum_s |u^_s[i]|^2), or of frechet.buoyancyPlanes along -e_i / rho_i^2
        (parameter='rho': density units).  For 'scaler' d A / d c_i is the diagonal weight and this is the formula above.  Served and refused as JvecBorn
        (`_resolveLinearisation`); the same routes, sides and perFreq as the default.

        kind 'gaussNewton': the exact diagonal of the Gauss-Newton Hessian that `Hvec` applies, D[i] = e_i . Hvec(m, e_i, linearisation=, parameter=) for every
        cell i -- the receiver side included, which the pseudo-Hessian leaves out:

            D[i] = sum_f sum_s sum_r |d dpred_(r,s,f) / d p_i|^2 = |scaleTerm|^2 sum_f sum_s sum_r |g_r^T (d A_f / d p_i) u^_s|^2,     g_r = A_f^-T R_r^H,

        evaluated as Re tr(E_i^H Gamma_i E_i Phi_i) over the 3 x 3 block around i, Gamma and Phi the Gram blocks of the receiver Green's functions and of the
        forward solves read off their autocorrelation planes at the lags of (-2..2)^2 (frechet.gaussNewtonDiagonal).  Every linearisation and parameter, served
        and refused as JvecBorn; for 'scaler' d A / d c_i is the diagonal weight and D[i] = |w_i|^2 sum_r |g_r[i]|^2 sum_s |u_s[i]|^2.  The receiver columns
        are solved through `adjointSystem`, so the factors of A and of A^T are resident side by side: Helm2DProblem with MiniZephyr / MiniZephyrHD on one
        grid; the 2.5-D composite, visco problems, Eurus, 3-D and multiscale surveys (with or without multiscaleDerivatives: diag(S^T H S) is not S^T diag(H)) raise
        NotImplementedError for every linearisation.  Fixed receiver arrays
        only (with an array that moves with the source Gamma depends on the source and the sum does not factorise: ValueError), side must stay 'source', and
        there are no data weights: a general `weights` array of `Hvec` does not factorise either.

        u a DeviceFields (fieldsDevice): no solve, the store is read where it lies ('gaussNewton': nothing but the nrec receiver columns is solved).  u None with
        the device path on a single-grid survey: the fields are solved into HBM, accumulated there and dropped; only the result comes down.  Otherwise (u a
        list of host arrays, no GPU, hostGradient, a host ky reduction, a multiscale survey): numpy on the host."""
        self._requirePaired()
        if kind not in ('energy', 'pseudoHessian', 'gaussNewton'):
            raise ValueError('kind is %r: \'energy\', \'pseudoHessian\' or \'gaussNewton\'' % (kind,))
        if side not in ('source', 'receiver'):
            raise ValueError('side is %r: \'source\' or \'receiver\'' % (side,))
        self._checkLinearisation(linearisation)
        self._checkParameter(parameter, linearisation)
        if kind == 'energy' and (linearisation != 'scaler' or parameter != 'c'):
            raise ValueError('kind=\'energy\' has no linearisation: linearisation=%r, parameter=%r go with kind=\'pseudoHessian\'' % (linearisation, parameter))
        sv = self.survey
        if kind == 'gaussNewton':
            if side != 'source':
                raise ValueError('kind=\'gaussNewton\' is the diagonal of J^T J, sources and receivers together: side must be \'source\'')
        if side == 'receiver':
            if u is not None:
                raise ValueError('the receiver-side illumination solves its own fields: u must be None')
            if sv.mode != 'fixed':
                raise ValueError('the receiver-side illumination serves fixed receiver arrays (mode is %r)' % (sv.mode,))
        self.updateModel(m)
        if kind == 'gaussNewton' or linearisation != 'scaler':
            self._refuseMultiscaleDiagonal('illumination(kind=%r, linearisation=%r)' % (kind, linearisation))
        if kind == 'gaussNewton' and linearisation == 'scaler':
            self._requireFullLinearisation('illumination(linearisation=\'scaler\')')      # (this kind needs the transposed 2-D operator whatever the linearisation)
            self._refuseKy('illumination(kind=\'gaussNewton\')', 'the Hessian diagonals are not built per ky (the \'scaler\' kinds \'energy\' and \'pseudoHessian\' are served)')
            self._refuseEurus('illumination(kind=\'gaussNewton\')', 'the Hessian diagonals are not built on the derivative maps of M1')
            self._refuseViscoDiagonal('illumination(linearisation=\'scaler\')')
        if linearisation != 'scaler':
            resolved = self._resolveLinearisation(linearisation, parameter, 'illumination')
            self._refuseKy('illumination(linearisation=%r)' % (linearisation,), 'the Hessian diagonals are not built per ky (the \'scaler\' kinds \'energy\' and '
                                                                                 '\'pseudoHessian\' are served)')
            self._refuseEurus('illumination(linearisation=%r)' % (linearisation,), 'the Hessian diagonals are not built on the derivative maps of M1 (the '
                                                                                    '\'scaler\' kinds \'energy\' and \'pseudoHessian\' are served)')
            self._refuseViscoDiagonal('illumination(linearisation=%r)' % (linearisation,))
            linearisation = resolved
        if kind == 'gaussNewton' and sv.mode != 'fixed':          # (after the refusals: what is not served at all says so first)
            raise ValueError('kind=\'gaussNewton\' serves fixed receiver arrays (mode is %r): with an array that moves with the source the sum over '
                             'receivers depends on the source and does not factorise' % (sv.mode,))
        owned = self.ownedFreqs
        if kind == 'gaussNewton' and linearisation != 'scaler' and (isinstance(u, DeviceFields) or (u is None and self._deviceGradientAvailable())):
            self._hermitianResidual(np.zeros((sv.nrec, 1, 1)))          # (the device route solves R^T for R^H: refused where the receiver columns are complex)
        if isinstance(u, DeviceFields):
            self._refusePerGridStore('illumination(u=F)')
            u.checkCurrent(self)
            return device_survey.illuminationFromFields(self, u, kind, bool(perFreq), linearisation, parameter)
        if u is None and not isinstance(sv, HelmMultiGridSurvey) and self._deviceGradientAvailable():
            return device_survey.illumination(self, owned, kind, side, bool(perFreq), linearisation, parameter)
        nf = sv.nfreq
        H = np.zeros((nf, self.nrow) if perFreq else self.nrow, dtype=np.float64)
        if kind == 'gaussNewton':
            green = self._receiverGreens(linearisation)
        if u is None:
            q = sv.getSources() if side == 'source' else [sp.csc_matrix(sv.rVec(0, i).T) for i in range(nf)]
            pps = sv.postProcessors
            fieldsOf = ((ifreq, pps[ifreq](uf)) for ifreq, uf in self._solveOwned(q))
        else:
            uF = list(u)
            fieldsOf = ((ifreq, uF[ifreq]) for ifreq in owned)
        for ifreq, uf in fieldsOf:
            uf = np.asarray(uf)
            uf = uf.reshape((uf.shape[0], -1))
            if kind == 'gaussNewton':
                E = self._gaussNewtonHost(ifreq, uf, green[ifreq], linearisation, parameter)
            elif linearisation != 'scaler':
                E = self._pseudoHessianHost(ifreq, uf, linearisation, parameter)
            else:
                E = np.add.reduce(np.square(uf.real) + np.square(uf.imag), axis=1)      # (no BLAS: _norm2 says why)
            if kind == 'pseudoHessian' and linearisation == 'scaler':
                w = np.asarray(self.gradientScaler(ifreq)).ravel()
                E = (np.square(w.real) + np.square(w.imag)) * E
            if perFreq:
                H[ifreq] = E
            else:
                H += E
        if self._sharded:
            H = parallel.allreduce_sum(H)
        return H

    def _pseudoHessianHost(self, ifreq, uf, linearisation, parameter):
        "one frequency's term of illumination(linearisation='operator' | 'full') on the host: uf = scaleTerm conj(u^) (N, ncols), the resolved linearisation"
        st = complex(self.system.scaleTerm)
        sub = self.system.subProblems[ifreq]
        uh = np.conj(uf / st)
        if linearisation == 'operator' and parameter == 'c':
            H = operatorPseudoHessianWeight(sub) * np.add.reduce(np.square(uh.real) + np.square(uh.imag), axis=1)
        else:
            H = pseudoHessianDiagonal(sub, uh, parameter, self._gardnerChain() if parameter == 'c' else None)
        return (st.real * st.real + st.imag * st.imag) * H

    def _receiverGreens(self, linearisation):
        """{ifreq: (N, nrec)} over the owned frequencies: the fixed array's rows back-propagated through the transposed operators as `_solveOwned` returns
        them, scaleTerm conj(A_f^-T premul q).  q = R^H for the exact derivatives, whose data are R . conj(...); R^T for 'scaler', whose data are conj(R) . (...)."""
        sv = self.survey
        q = [sp.csc_matrix(sv.rVec(0, i).T) for i in range(sv.nfreq)]
        if linearisation != 'scaler':
            q = [m.conj() for m in q]
        return {ifreq: np.asarray(g) for ifreq, g in self._solveOwned(q, self.adjointSystem)}

    def _gaussNewtonHost(self, ifreq, uf, gf, linearisation, parameter):
        """one frequency's term of illumination(kind='gaussNewton') on the host: uf = scaleTerm conj(u^) (N, nsrc), gf = scaleTerm conj(premul g) (N, nrec) of
        `_receiverGreens`, the resolved linearisation.  'scaler': |d_(r,s) / v_i| = |w_i| |uf_s[i]| |gf_r[i]|, the planes of the arrays as they are."""
        sub = self.system.subProblems[ifreq]
        nz, nx = int(sub.nz), int(sub.nx)
        if linearisation == 'scaler':
            return gaussNewtonDiagonal(sub, lagGram(uf, nz, nx), lagGram(gf, nz, nx), linearisation='scaler', weight=self.gradientScaler(ifreq))
        st = complex(self.system.scaleTerm)
        uh = np.conj(uf / st)
        gh = np.conj(gf / (st * np.conj(complex(sub.premul))))
        H = gaussNewtonDiagonal(sub, lagGram(uh, nz, nx), lagGram(gh, nz, nx), parameter, self._gardnerChain() if parameter == 'c' else None, linearisation)
        return (st.real * st.real + st.imag * st.imag) * H

    # ---- per-cell 2 x 2 blocks of the joint (c, rho) Hessian -----------------------------------------------
    def hessianBlocks(self, m=None, u=None, kind='gaussNewton', side='source', perFreq=False, linearisation='full'):
        """What a two-parameter gradient [g_c; g_rho] is divided by: float64 (3, N), or (nfreq, 3, N) with perFreq -- the rows H_cc, H_crho, H_rhorho of the
        2 x 2 diagonal block of the joint Hessian per cell, for frechet.blockSolve.  With E^c_i = d A_f / d c_i (frechet.velocityPlanes along e_i at the config's
        density for 'full', frechet.massPlanes for 'operator'), E^rho_i = -E^b_i / rho_i^2 (E^b_i of frechet.buoyancyPlanes), u^_s = A_f^-1 premul q_s and
        g_r = A_f^-T R_r^H:

        kind 'gaussNewton':   B[a, b][i] = |scaleTerm|^2 sum_f sum_s sum_r Re conj(g_r^T E^a_i u^_s) (g_r^T E^b_i u^_s) = |scaleTerm|^2 sum_f Re tr(E^a_i^H Gamma_i E^b_i Phi_i),
                              the block of the operator Hvec(parameter='joint') applies: B[1][i] = Hvec(m, [0; e_i], parameter='joint')[i], rows 0 and 2 are
                              illumination(kind='gaussNewton', parameter='c' / 'rho').  Fixed receiver arrays, side 'source', as that diagonal.
        kind 'pseudoHessian': B[a, b][i] = |scaleTerm|^2 sum_f sum_s Re <E^a_i u^_s, E^b_i u^_s> over the rows of the 3 x 3 block: the same with Gamma the identity;
                              rows 0 and 2 are illumination(linearisation=, parameter='c' / 'rho').  side 'receiver' and moving arrays as `illumination`.

        Every block is a Gram matrix: B[0], B[2] >= 0, B[1]^2 <= B[0] B[2]; B[1] has either sign.  Served and refused as Hvec(parameter='joint'): an explicit
        `rho`, 'operator' or 'full' (`_resolveLinearisation`).  The routes of `illumination`: u a DeviceFields, u None (solved into HBM and dropped), or numpy on
        the host; sharded ranks end in one all-reduce."""
        self._requirePaired()
        if kind not in ('pseudoHessian', 'gaussNewton'):
            raise ValueError('kind is %r: \'pseudoHessian\' or \'gaussNewton\' (the energy has no density entry)' % (kind,))
        if side not in ('source', 'receiver'):
            raise ValueError('side is %r: \'source\' or \'receiver\'' % (side,))
        self._checkLinearisation(linearisation)
        self._checkParameter('joint', linearisation, joint=True)
        sv = self.survey
        if kind == 'gaussNewton' and side != 'source':
            raise ValueError('kind=\'gaussNewton\' is the block of J^T J, sources and receivers together: side must be \'source\'')
        if side == 'receiver':
            if u is not None:
                raise ValueError('the receiver-side blocks solve their own fields: u must be None')
            if sv.mode != 'fixed':
                raise ValueError('the receiver-side blocks serve fixed receiver arrays (mode is %r)' % (sv.mode,))
        self.updateModel(m)
        self._refuseMultiscaleDiagonal('hessianBlocks')
        linearisation = self._resolveLinearisation(linearisation, 'joint', 'hessianBlocks')
        self._refuseKy('hessianBlocks', 'the per-cell blocks of the joint Hessian are not built per ky')
        self._refuseEurus('hessianBlocks', 'the per-cell blocks of the joint Hessian are not built on the derivative maps of M1')
        if kind == 'gaussNewton' and sv.mode != 'fixed':
            raise ValueError('kind=\'gaussNewton\' serves fixed receiver arrays (mode is %r): with an array that moves with the source the sum over '
                             'receivers depends on the source and does not factorise' % (sv.mode,))
        owned = self.ownedFreqs
        if kind == 'gaussNewton' and (isinstance(u, DeviceFields) or (u is None and self._deviceGradientAvailable())):
            self._hermitianResidual(np.zeros((sv.nrec, 1, 1)))          # (the device route solves R^T for R^H: refused where the receiver columns are complex)
        if isinstance(u, DeviceFields):
            u.checkCurrent(self)
            return device_survey.hessianBlocksFromFields(self, u, kind, bool(perFreq), linearisation)
        if u is None and self._deviceGradientAvailable():
            return device_survey.hessianBlocks(self, owned, kind, side, bool(perFreq), linearisation)
        nf = sv.nfreq
        B = np.zeros((nf, 3, self.nrow) if perFreq else (3, self.nrow), dtype=np.float64)
        if kind == 'gaussNewton':
            green = self._receiverGreens(linearisation)
        if u is None:
            q = sv.getSources() if side == 'source' else [sp.csc_matrix(sv.rVec(0, i).T) for i in range(nf)]
            pps = sv.postProcessors
            fieldsOf = ((ifreq, pps[ifreq](uf)) for ifreq, uf in self._solveOwned(q))
        else:
            uF = list(u)
            fieldsOf = ((ifreq, uF[ifreq]) for ifreq in owned)
        for ifreq, uf in fieldsOf:
            uf = np.asarray(uf)
            uf = uf.reshape((uf.shape[0], -1))
            E = self._gaussNewtonBlocksHost(ifreq, uf, green[ifreq], linearisation) if kind == 'gaussNewton' else self._pseudoHessianBlocksHost(ifreq, uf, linearisation)
            if perFreq:
                B[ifreq] = E
            else:
                B += E
        if self._sharded:
            B = parallel.allreduce_sum(B)
        return B

    def _pseudoHessianBlocksHost(self, ifreq, uf, linearisation):
        "one frequency's term of hessianBlocks(kind='pseudoHessian') on the host: uf = scaleTerm conj(u^) (N, ncols)"
        st = complex(self.system.scaleTerm)
        return (st.real * st.real + st.imag * st.imag) * pseudoHessianBlocks(self.system.subProblems[ifreq], np.conj(uf / st), linearisation)

    def _gaussNewtonBlocksHost(self, ifreq, uf, gf, linearisation):
        "one frequency's term of hessianBlocks(kind='gaussNewton') on the host: uf and gf as `_gaussNewtonHost` takes them"
        sub = self.system.subProblems[ifreq]
        nz, nx = int(sub.nz), int(sub.nx)
        st = complex(self.system.scaleTerm)
        uh = np.conj(uf / st)
        gh = np.conj(gf / (st * np.conj(complex(sub.premul))))
        return (st.real * st.real + st.imag * st.imag) * gaussNewtonBlocks(sub, lagGram(uh, nz, nx), lagGram(gh, nz, nx), linearisation)

    # ---- device-resident gradient (mux branch) -------------------------------------------------------------
    def _deviceGradientAvailable(self):
        'true when the sub-problems are GPU operators and torch can hold the buffers in HBM'
        if getattr(self, '_hostGradient', False):
            return False
        subs = self.system.subProblems
        if not subs or not hasattr(subs[0], 'solveDevice'):
            return False
        from .discretization import DiscretizationWrapper
        if isinstance(subs[0], DiscretizationWrapper):
            # composite sub-problems (2.5-D ky sums) own no single device operator: they serve when they form their sum in HBM themselves
            # (MiniZephyr25D.solveDevice / sampleSumDevice), on a single-grid survey -- the multiscale 2.5-D pairing stays on the host path
            if not getattr(subs[0], 'kySumOnDevice', False) or isinstance(self.survey, HelmMultiGridSurvey):
                return False
        return _lib.gpu_usable()

    def _plainGradientScaler(self):
        "the survey's post-processor is the reference's identity (survey.py:190-196) and the scaler the problem's own: then a device path can make it where it is used"
        return (type(self.survey).postProcessors is HelmBaseSurvey.postProcessors and type(self).gradientScaler is HelmBaseProblem.gradientScaler
                and type(self).scaledTerms is HelmBaseProblem.scaledTerms)

    def _JtvecDevice(self, qb, owned, resid=None):
        'mux branch with the wavefields kept in HBM (device_survey.gradient).  qb None: the back-sources of a moving receiver array, made on the device from `resid`'
        return device_survey.gradient(self, qb, owned, resid)

    def _dpredDevice(self, owned):
        'predicted data (nrec, nsrc, nfreq) of the owned frequencies with the wavefields kept in HBM (device_survey.dpred)'
        return device_survey.dpred(self, owned)

    @property
    def factors(self):
        return self.system.factors

    @factors.deleter
    def factors(self):
        del self.system.factors
        adj = self.__dict__.get('_adjointSystem', None)
        if adj is not None:
            del adj.factors


class Helm2DProblem(HelmBaseProblem):

    initMap = {
        'SystemWrapper':    (False,    None,        None),
    }

    surveyPair = Helm2DSurvey
    SystemWrapper = MultiFreq


class Helm2DViscoProblem(Helm2DProblem):

    SystemWrapper = ViscoMultiFreq


class Helm2DViscoMultiGridProblem(Helm2DProblem):
    """Visco-acoustic multiscale problem (zephyr/middleware/problem.py:220-222): every frequency on its own grid (ViscoMultiGridMultiFreq),
    paired with a Helm2DMultiGridSurvey built from the same config."""

    SystemWrapper = ViscoMultiGridMultiFreq


class Helm25DProblem(HelmBaseProblem):
    """2.5-D counterpart of Helm2DProblem (zephyr/middleware/problem.py:225-235): same machinery, paired with Helm25DSurvey; the caller's
    systemConfig names `Disc = MiniZephyr25D` (and `nky`), every frequency is a sum over cross-line wavenumbers."""

    initMap = {
        'SystemWrapper':    (False,    None,        None),
    }

    surveyPair = Helm25DSurvey
    SystemWrapper = MultiFreq


class Helm25DViscoProblem(Helm25DProblem):
    'zephyr/middleware/problem.py:236-238'

    SystemWrapper = ViscoMultiFreq

