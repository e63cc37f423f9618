"""The 3-D survey problem: `Helm3DProblem` pairs a `Helm3DSurvey` with `MultiFreq` over `Helm3D` and serves predicted data, stored fields, the reference's
gradient and the exact velocity derivative of `dpred` with its adjoint.

The derivative (DESIGN.md has it with the conjugations written out).  `sub * q = conj(A^-1 premul q)`, the wrapper scales by st = scaleTerm, so the stored
fields are uF_s = st conj(u^_s), u^_s = A^-1 premul q_s, and d_s = R_s uF_s.  With an explicit `rho` the whole derivative of A along the velocity is its mass
term, dA[dc] = M~ diag(chi dc), chi = -2 K / c (frechet3d.py), so

    JvecBorn:   dd_s = st R_s conj(-A^-1 M~(chi dc (.) u^_s))                  = R_s . st (sub * (-M~(chi dc (.) u^_s) / premul))
    Jtvec:      g    = Re sum_f w_f chi (.) sum_s u^_s (.) (M~^T z~_s),          z~_s = premul A^-T R_s^H r_s = conj((sub^T * R_s^H r_s)),  w_f = -conj(st) / premul

and Re <r, JvecBorn(v)> = <Jtvec(r), v>.  A is not symmetric, so the back-propagation runs through A^-T: `adjointSystem`, the same wrapper over
`Disc.Transposed` (Helm3DTransposed).  'operator' and 'full' are the same derivative here (as on Eurus: the C-PML does not depend on c).  Without `rho` in the config the Gardner
density moves the Laplacian part with c; that derivative is not built and the exact routes are refused.
"""
import numpy as np

from .distributors import MultiFreq, ViscoMultiFreq, MultiGridMultiFreq
from .fieldstore import DeviceFields
from .helm3d import Helm3D
from .problem import HelmBaseProblem
from .survey import Helm3DSurvey
from . import frechet3d
from . import parallel


class Helm3DProblem(HelmBaseProblem):
    """Forward problem and gradient on a 3-D grid.  The config carries nx, ny, nz (dx, dy, dz, nPML, cPML, ...), `c`, `rho` and `freqs`; `Disc` defaults to Helm3D
    and the system wrapper is MultiFreq (multiscale and visco wrappers are refused: they are built for 2-D grids).

    Served: `survey.dpred(m)`, `dpred(m, u=F)`, `fields(m)`, `fieldsDevice(m)` (complex128 store), `Jtvec(m, r, u=None | F | host list)` in the reference's form
    (adjoint='reciprocity', linearisation='scaler': gradientScaler with the back-propagation through the forward operators) and with adjoint='transpose';
    `Jtvec(..., adjoint='transpose', linearisation='operator' | 'full')` and `JvecBorn(m, v, u=..., linearisation='operator' | 'full')`, exact adjoints of each
    other and the derivative of `dpred`; `illumination` of the 'scaler' kinds; `adjointSystem`; `del prob.factors`; frequencies sharded over ranks, ending in the
    one all-reduce of the (N,) vector.  With a GPU and without hostGradient everything of size N k stays on the device (device_survey3d.py): a 3-D work item
    builds its multigrid hierarchy in the prepare step, strictly one item ahead, for `system` and for `adjointSystem` alike -- and while both wrappers are alive
    TWO hierarchies per frequency are resident, that of A_f and that of A_f^T (`del prob.factors` releases both).

    Refused with the reason: the exact routes without `rho`; parameter other than 'c'; `Jvec`, `Hvec`, `hessianBlocks` and the illumination kinds that need the
    derivative planes; fieldsDtype='complex64' with the exact routes; perKy / ownGrid."""

    initMap = {
        'SystemWrapper':    (False,    None,        None),
    }

    surveyPair = Helm3DSurvey
    SystemWrapper = MultiFreq

    def __init__(self, systemConfig, *args, **kwargs):
        if systemConfig.get('ny', None) is None:
            raise ValueError('Helm3DProblem requires parameter \'ny\': without it the config describes a 2-D grid (Helm2DProblem)')
        systemConfig = dict(systemConfig)
        systemConfig.setdefault('Disc', Helm3D)
        HelmBaseProblem.__init__(self, systemConfig, *args, **kwargs)
        wrapper = self.SystemWrapper
        if isinstance(wrapper, type) and issubclass(wrapper, (MultiGridMultiFreq, ViscoMultiFreq)):
            raise NotImplementedError('Helm3DProblem does not serve %s: the multiscale and visco wrappers are built for 2-D grids (use MultiFreq, the default)'
                                      % (wrapper.__name__,))

    @property
    def adjointSystem(self):
        """The system wrapper of the TRANSPOSED operators: the class of `system`, built from the same systemConfig with `Disc.Transposed` (Helm3DTransposed for
        Helm3D) in the place of `Disc` -- the same frequencies on the same devices.  `sub * q` there is conj(A_f^-T (premul q)).  It goes with the problem's cache
        on a model change, and `del prob.factors` releases it too.  While both wrappers are in use two multigrid hierarchies per frequency are resident."""
        if getattr(self, '_adjointSystem', None) is None:
            cfg = dict(self.systemConfig)
            disc = cfg.get('Disc', Helm3D)
            tdisc = getattr(disc, 'Transposed', None)
            if tdisc is None:
                raise NotImplementedError('%s names no transposed class (`Disc.Transposed`): the exact adjoint back-propagates through A^-T'
                                          % (getattr(disc, '__name__', disc),))
            cfg['Disc'] = tdisc
            adj = type(self.system)(cfg)
            adj.subProblems
            self._adjointSystem = adj
        return self._adjointSystem

    # ---- what is refused ---------------------------------------------------------------------------------------------------------------------
    def _requireExact3(self, what, parameter):
        'the exact routes serve parameter=\'c\' of a config with an explicit `rho` and a complex128 store'
        if parameter != 'c':
            raise NotImplementedError('%s with parameter=%r is not built in 3-D: the density, joint and Q derivatives exist for the 2-D operators only (parameter=\'c\' '
                                      'is served)' % (what, parameter))
        if self.systemConfig.get('rho', None) is None:
            raise NotImplementedError('%s needs an explicit `rho` in the config: without one the Gardner density follows c and moves the Laplacian part of the 3-D '
                                      'operator with it, and that derivative is not built (give `rho`, e.g. 310 c^0.25 as an array)' % (what,))
        if self.fieldsDtype != 'complex128':
            raise NotImplementedError('%s reads a complex128 store: fieldsDtype=%r is not served by the 3-D kernels (leave fieldsDtype at its default)'
                                      % (what, self.fieldsDtype))

    @staticmethod
    def _refuse3(what, remedy):
        raise NotImplementedError('%s is not built for 3-D problems: %s' % (what, remedy))

    def fields(self, m=None, perKy=False, ownGrid=False):
        if perKy or ownGrid:
            raise ValueError('fields(perKy=%r, ownGrid=%r): a 3-D problem has one grid and no ky axis (call fields(m))' % (perKy, ownGrid))
        return HelmBaseProblem.fields(self, m)

    def fieldsDevice(self, m=None, perKy=False):
        if perKy:
            raise ValueError('fieldsDevice(perKy=True) is the per-ky store of a 2.5-D problem: a 3-D problem has no ky axis (call fieldsDevice(m))')
        return HelmBaseProblem.fieldsDevice(self, m)

    def Jvec(self, m=None, v=None, u=None):
        self._refuse3('Jvec', 'the reference\'s one-column outer-product approximation is written for 2-D grids; JvecBorn(linearisation=\'operator\') is the '
                              'derivative of dpred')

    def Hvec(self, *args, **kwargs):
        self._refuse3('Hvec', 'apply Jtvec(JvecBorn(v, linearisation=\'operator\'), adjoint=\'transpose\', linearisation=\'operator\') for the Gauss-Newton product')

    def hessianBlocks(self, *args, **kwargs):
        self._refuse3('hessianBlocks', 'there is no density derivative in 3-D to pair the velocity with; illumination(kind=\'pseudoHessian\') preconditions a gradient')

    def illumination(self, m=None, u=None, kind='pseudoHessian', side='source', perFreq=False, linearisation='scaler', parameter='c'):
        if kind == 'gaussNewton' or linearisation != 'scaler' or parameter != 'c':
            self._refuse3('illumination(kind=%r, linearisation=%r, parameter=%r)' % (kind, linearisation, parameter),
                          'the Hessian diagonals are built on the derivative planes of the 2-D operators; kind \'energy\' and \'pseudoHessian\' with the default '
                          'linearisation=\'scaler\' are served')
        return HelmBaseProblem.illumination(self, m, u, kind, side, perFreq)

    # ---- gradient and Born data ------------------------------------------------------------------------------------------------------------------
    def Jtvec(self, m=None, v=None, u=None, adjoint='reciprocity', linearisation='scaler', parameter='c'):
        """The gradient.  Defaults (adjoint='reciprocity', linearisation='scaler'): the reference's form, sum_f gradientScaler_f (.) sum_s uF_s (.) uB_s with the
        back-propagation through the forward operators (complex with u None, the real part with u given, as in 2-D).  adjoint='transpose': through A^-T
        (`adjointSystem`).  linearisation='operator' or 'full' (the same derivative in 3-D; needs adjoint='transpose' and `rho` in the config): J^T r with J the
        derivative of `dpred` -- float64 (N,), the exact adjoint of JvecBorn(linearisation='operator').  u: None, a DeviceFields of fieldsDevice(), or the host
        list of fields()."""
        if linearisation == 'scaler' and parameter == 'c':
            return HelmBaseProblem.Jtvec(self, m, v, u, adjoint, 'scaler', 'c')
        self._requirePaired()
        if v is None:
            raise Exception('Actually, Jtvec requires a residual vector')
        self._checkLinearisation(linearisation)
        if adjoint not in ('reciprocity', 'transpose'):
            raise ValueError('adjoint is %r: \'reciprocity\' or \'transpose\'' % (adjoint,))
        self._requireExact3('Jtvec(linearisation=%r)' % (linearisation,), parameter)
        if adjoint != 'transpose':
            raise ValueError('linearisation=%r needs adjoint=\'transpose\': the exact derivative back-propagates through A^-T' % (linearisation,))
        self.updateModel(m)
        sv = self.survey
        resid = np.asarray(v).reshape((sv.nrec, sv.nsrc, sv.nfreq))
        adj = self.adjointSystem
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                from . import device_survey3d
                rd = self._hermitianResidual(resid)
                return device_survey3d.gradientFromFields3(self, F, self._deviceBackSources(rd), rd, adj)
            g = np.zeros(self.nrow, dtype=np.float64)
            st = complex(self.system.scaleTerm)
            qb = [q.conj() for q in sv.getResidualSources(np.conj(resid))]        # R_s^H r_s = conj(R_s^T conj(r_s))
            M = None
            for ifreq, uB in self._solveOwned(qb, adj):
                op = self.system.subProblems[ifreq]
                M = frechet3d.massStencil3(op.modelDims) if M is None else M
                P = frechet3d.imagingSum3(op, np.conj(np.asarray(F[ifreq]) / st), np.conj(np.asarray(uB) / st), M)
                g += ((-np.conj(st) / complex(op.premul)) * frechet3d.velocityChain3(op) * P).real
        if self._sharded:
            g = parallel.allreduce_sum(g)
        return g

    def JvecBorn(self, m=None, v=None, u=None, linearisation='scaler', parameter='c'):
        """Born data of the velocity perturbation v (N,), the ravel of (nrec, nsrc, nfreq) complex128.  linearisation='scaler': the reference's convention, as in
        2-D.  'operator' or 'full' (the same in 3-D; `rho` in the config): the derivative of `sv.dpred` along v, d/dh dpred(m + h v) at h = 0, v non-zero
        anywhere -- boundary nodes included, they are columns of interior rows.  u as for Jtvec."""
        if linearisation == 'scaler' and parameter == 'c':
            return HelmBaseProblem.JvecBorn(self, m, v, u, 'scaler', 'c')
        self._requirePaired()
        if v is None:
            raise Exception('Actually, JvecBorn requires a perturbation vector')
        self._checkLinearisation(linearisation)
        self._requireExact3('JvecBorn(linearisation=%r)' % (linearisation,), parameter)
        self.updateModel(m)
        sv = self.survey
        dc = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape((self.nrow,)))
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                from . import device_survey3d
                data = device_survey3d.bornFromFields3(self, F, dc)
            else:
                data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
                st = complex(self.system.scaleTerm)
                subs = self.system.subProblems
                owned = self.ownedFreqs
                M = frechet3d.massStencil3(subs[0].modelDims) if owned else None
                qv = [frechet3d.bornSources3(subs[i], dc, np.conj(np.asarray(F[i]) / st), M) / -complex(subs[i].premul) if i in owned else None
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
