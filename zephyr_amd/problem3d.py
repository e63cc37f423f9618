"""The 3-D survey problem: `Helm3DProblem` pairs a `Helm3DSurvey` with `MultiFreq` over `Helm3D` and serves predicted data, stored fields, the reference's
gradient and the exact velocity derivative of `dpred` with its adjoint.

The derivative (DESIGN.md has it with the conjugations written out).  `sub * q = conj(A^-1 premul q)`, the wrapper scales by st = scaleTerm, so the stored
fields are uF_s = st conj(u^_s), u^_s = A^-1 premul q_s, and d_s = R_s uF_s.  With an explicit `rho` the whole derivative of A along the velocity is its mass
term, dA[dc] = M~ diag(chi dc), chi = -2 K / c (frechet3d.py), so

    JvecBorn:   dd_s = st R_s conj(-A^-1 M~(chi dc (.) u^_s))                  = R_s . st (sub * (-M~(chi dc (.) u^_s) / premul))
    Jtvec:      g    = Re sum_f w_f chi (.) sum_s u^_s (.) (M~^T z~_s),          z~_s = premul A^-T R_s^H r_s = conj((sub^T * R_s^H r_s)),  w_f = -conj(st) / premul

and Re <r, JvecBorn(v)> = <Jtvec(r), v>.  A is not symmetric, so the back-propagation runs through A^-T: `adjointSystem`, the same wrapper over
`Disc.Transposed` (Helm3DTransposed).  'operator' and 'full' are the same derivative here (as on Eurus: the C-PML does not depend on c).  Without `rho` in the config the Gardner
density moves the Laplacian part with c; without the config key derivatives3D the exact routes are then refused.

With derivatives3D=True the derivative along the buoyancy b = 1 / rho is served too (frechet3d.py).  A row is linear in b,
dA[db] = 1/2 diag(db) L + 1/2 L diag(db) + M~ diag(kappa db), kappa = om~^2 / c^2, L the Laplacian part with the stretch tables at the row (not symmetric), so

    Born sources:  R_s = -(1 / premul) [ 1/2 db (.) (L u^_s) + 1/2 L(db (.) u^_s) + M~(kappa db (.) u^_s) ]
    gradient:      g_b = Re sum_f w_f sum_s [ 1/2 z~0_s (.) (L u^_s) + 1/2 u^_s (.) (L^T z~0_s) + kappa (.) u^_s (.) (M~^T z~0_s) ]

(z~0: z~ with its boundary rows masked), g_rho = -g_b / rho^2, db = -drho / rho^2: parameter='rho' and 'joint' ([c; rho] stacked; ONE back-solve, ONE Born solve).  Without `rho`
b = Re(c)^-0.25 / 310 and d b / d c = -b / (4 Re c): linearisation='full', parameter='c' is the mass chain at fixed rho plus the buoyancy maps at db = (d b / d c) dc.  `Hvec` is
the Gauss-Newton product of the two halves.
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
    derivative planes; fieldsDtype='complex64' with the exact routes; perKy / ownGrid.

    With the config key derivatives3D=True (without it all of the above is unchanged): parameter 'rho' and 'joint' on `Jtvec(adjoint='transpose')` and `JvecBorn` with
    linearisation 'operator' | 'full'; without `rho` in the config linearisation='full', parameter='c', the total derivative through the Gardner density ('operator', 'rho'
    and 'joint' stay refused there); `Hvec(m, v, u, weights, linearisation, parameter)`, the Gauss-Newton product; `m` may be {'c': ..., 'rho': ...}.  Still refused: 'Q' / 'cQ',
    `Hvec(resid=)`, `hessianBlocks`, the non-'scaler' illumination kinds, `Jvec`, fieldsDtype='complex64', perKy / ownGrid, the multiscale and visco wrappers.

    With the config key hessian3D=True (without it all of the above is unchanged): what a 3-D gradient is divided by -- the pseudo-Hessian of the exact derivatives, which
    costs no solve.  `illumination(m, u, kind='pseudoHessian', linearisation='operator' | 'full', parameter='c' | 'rho', perFreq)`: float64 (N,) or
    (nfreq, N), H_p[i] = |scaleTerm|^2 sum_f sum_s ||(d A_f / d p_i) u^_s||^2; `hessianBlocks(m, u, kind='pseudoHessian', linearisation=, perFreq)`: the rows H_cc, H_crho,
    H_rhorho, (3, N) or (nfreq, 3, N), for frechet.blockSolve with the 'joint' gradient.  Served by the rules of the gradient being preconditioned: 'c' with an explicit
    `rho` needs this key alone (the closed form |chi|^2 Smu sum_s |u^_s[i]|^2); 'rho', the blocks and -- without `rho` in the config -- linearisation='full', parameter='c'
    (the Gardner total derivative) need derivatives3D=True beside it.  u None, a DeviceFields or the host list; fixed and moving arrays; sharded ranks end in one
    all-reduce.  Refused with a sentence, the key set or not: kind='gaussNewton' (nrec back-solves through A^T per frequency), side='receiver' on the exact kinds,
    fieldsDtype='complex64', 'Q' / 'cQ', illumination(parameter='joint') (use hessianBlocks), hessianBlocks without `rho`.  kind='energy' and the 'scaler'
    pseudo-Hessian return the bits they returned."""

    initMap = {
        'SystemWrapper':    (False,    None,        None),
        'derivatives3D':    (False,    '_derivatives3D', bool),    # serve the density, joint and Gardner derivatives and Hvec (the buoyancy maps of frechet3d.py)
        'hessian3D':        (False,    '_hessian3D', bool),        # serve the exact pseudo-Hessian diagonal and the (c, rho) blocks (illumination, hessianBlocks)
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
    def _requireExact3(self, what, parameter, linearisation='operator'):
        """the exact routes serve parameter='c' of a config with an explicit `rho` and a complex128 store; with derivatives3D=True also 'rho' and 'joint', and
        without `rho` the total velocity derivative through the Gardner density (linearisation='full', parameter='c').  Returns (parameter, gardner)."""
        if getattr(self, '_derivatives3D', False):
            if isinstance(parameter, str) and parameter in ('Q', 'cQ'):
                raise NotImplementedError('%s with parameter=%r is not built in 3-D: the visco wrappers and the chain from (c, Q) to the complex velocity are those of '
                                          'the 2-D operators (parameter \'c\', \'rho\' and \'joint\' are served)' % (what, parameter))
            self._checkParameter(parameter, linearisation, joint=True)
            if self.fieldsDtype != 'complex128':
                raise NotImplementedError('%s reads a complex128 store: fieldsDtype=%r is not served by the 3-D kernels (leave fieldsDtype at its default)'
                                          % (what, self.fieldsDtype))
            if self._hasDensity():
                return parameter, False
            if parameter != 'c' or linearisation != 'full':
                raise NotImplementedError('%s without `rho` in the config serves linearisation=\'full\', parameter=\'c\': the density follows the velocity '
                                          '(Gardner), so it is no parameter of its own and the derivative at fixed density (\'operator\') is not the derivative '
                                          'of dpred (give `rho`, e.g. 310 c^0.25 as an array, for \'operator\', \'rho\' and \'joint\')' % (what,))
            return 'c', True
        if parameter != 'c':
            raise NotImplementedError('%s with parameter=%r is not built in 3-D: the density, joint and Q derivatives exist for the 2-D operators only (parameter=\'c\' '
                                      'is served)' % (what, parameter))
        if self.systemConfig.get('rho', None) is None:
            raise NotImplementedError('%s needs an explicit `rho` in the config: without one the Gardner density follows c and moves the Laplacian part of the 3-D '
                                      'operator with it, and that derivative is not built (give `rho`, e.g. 310 c^0.25 as an array)' % (what,))
        if self.fieldsDtype != 'complex128':
            raise NotImplementedError('%s reads a complex128 store: fieldsDtype=%r is not served by the 3-D kernels (leave fieldsDtype at its default)'
                                      % (what, self.fieldsDtype))
        return 'c', False

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

    def Hvec(self, m=None, v=None, u=None, weights=None, linearisation='operator', parameter='c', resid=None):
        """With derivatives3D=True: the Gauss-Newton product J^T W J v, Jtvec(JvecBorn(v) (.) weights, adjoint='transpose') on the same forward fields -- float64
        (N,), or (2 N,) for parameter='joint' (v = [v_c; v_rho]).  linearisation 'operator' or 'full', parameter 'c', 'rho' or 'joint' as the two halves serve
        them; weights: optional, real, non-negative, of the size of the data.  Two solves of nsrc columns per frequency, no forward re-solve; only the
        nrec x nsrc samples cross to the host between the halves.  resid= (the Newton term) is refused.  Without the key: refused as it always was."""
        if not getattr(self, '_derivatives3D', False):
            self._refuse3('Hvec', 'apply Jtvec(JvecBorn(v, linearisation=\'operator\'), adjoint=\'transpose\', linearisation=\'operator\') for the Gauss-Newton product')
        self._requirePaired()
        if v is None:
            raise Exception('Actually, Hvec requires a vector')
        if resid is not None:
            self._refuse3('Hvec(resid=)', 'the second derivative of the 27-point operator and the third solve of the Newton term are not built; resid=None, the '
                                          'Gauss-Newton product, is served')
        self._checkLinearisation(linearisation)
        if linearisation == 'scaler':
            raise ValueError('Hvec of a 3-D problem composes the exact halves: linearisation is \'operator\' or \'full\'')
        self.updateModel(m)
        self._requireExact3('Hvec(linearisation=%r)' % (linearisation,), parameter, linearisation)
        if weights is not None:
            weights = np.asarray(weights)
            if np.iscomplexobj(weights) or weights.size != self.survey.nD or not np.all(weights >= 0):
                raise ValueError('weights are real, non-negative and of the size of the data (%d)' % (self.survey.nD,))
            weights = weights.astype(np.float64).ravel()
        if parameter == 'joint':
            self._splitJoint(v, 'Hvec')
        with self._forwardFields(u) as F:
            d = self.JvecBorn(None, v, u=F, linearisation=linearisation, parameter=parameter)
            if weights is not None:
                d = d * weights
            return self.Jtvec(None, d, u=F, adjoint='transpose', linearisation=linearisation, parameter=parameter)

    def hessianBlocks(self, *args, **kwargs):
        """With hessian3D=True (and derivatives3D=True, an explicit `rho`): hessianBlocks(m, u, kind='pseudoHessian', side='source', perFreq, linearisation) -- the rows
        H_cc, H_crho, H_rhorho of the per-cell 2 x 2 blocks of the pseudo-Hessian of the joint (c, rho) derivative, float64 (3, N) or (nfreq, 3, N), for
        frechet.blockSolve.  Rows 0 and 2 are illumination(linearisation=, parameter='c' / 'rho'); B[1]^2 <= B[0] B[2].  Without the key: refused as it always was."""
        if getattr(self, '_hessian3D', False):
            return self._hessianBlocks3(*args, **kwargs)
        if getattr(self, '_derivatives3D', False):
            self._refuse3('hessianBlocks', 'the per-cell blocks are built on the derivative planes of the 2-D operators; Hvec(parameter=\'joint\') applies the '
                                           'Gauss-Newton Hessian and illumination(kind=\'pseudoHessian\') preconditions a gradient')
        self._refuse3('hessianBlocks', 'there is no density derivative in 3-D to pair the velocity with; illumination(kind=\'pseudoHessian\') preconditions a gradient')

    def illumination(self, m=None, u=None, kind='pseudoHessian', side='source', perFreq=False, linearisation='scaler', parameter='c'):
        """kind 'energy' and 'pseudoHessian' with the default linearisation='scaler': as in 2-D.  With hessian3D=True also the pseudo-Hessian diagonal of the exact
        derivatives, H_p[i] = |scaleTerm|^2 sum_f sum_s ||(d A_f / d p_i) u^_s||^2: linearisation 'operator' | 'full' with parameter 'c' (an explicit `rho`: the
        closed form |chi|^2 Smu sum_s |u^_s[i]|^2) and, with derivatives3D=True too, parameter 'rho' and -- without `rho` in the config -- linearisation='full',
        parameter='c', the total derivative through the Gardner density.  float64 (N,), or (nfreq, N) with perFreq.  u: None, a DeviceFields or the host list."""
        if kind == 'gaussNewton' or linearisation != 'scaler' or parameter != 'c':
            if getattr(self, '_hessian3D', False):
                return self._pseudoHessian3(m, u, kind, side, perFreq, linearisation, parameter, blocks=False)
            self._refuse3('illumination(kind=%r, linearisation=%r, parameter=%r)' % (kind, linearisation, parameter),
                          'the Hessian diagonals are built on the derivative planes of the 2-D operators; kind \'energy\' and \'pseudoHessian\' with the default '
                          'linearisation=\'scaler\' are served')
        return HelmBaseProblem.illumination(self, m, u, kind, side, perFreq)

    def _hessianBlocks3(self, m=None, u=None, kind='gaussNewton', side='source', perFreq=False, linearisation='full'):
        return self._pseudoHessian3(m, u, kind, side, perFreq, linearisation, 'joint', blocks=True)

    def _pseudoHessian3(self, m, u, kind, side, perFreq, linearisation, parameter, blocks):
        """illumination of the exact kinds and hessianBlocks with hessian3D=True.  What is served follows the gradient being preconditioned (`_requireExact3`): 'c'
        with an explicit `rho` needs this key alone; 'rho', the blocks and the Gardner total derivative need derivatives3D=True beside it."""
        what = 'hessianBlocks' if blocks else 'illumination'
        self._requirePaired()
        if kind not in (('pseudoHessian', 'gaussNewton') if blocks else ('energy', 'pseudoHessian', 'gaussNewton')):
            raise ValueError('kind is %r: %s' % (kind, '\'pseudoHessian\' (the energy has no density entry)' if blocks else '\'energy\' or \'pseudoHessian\''))
        if side not in ('source', 'receiver'):
            raise ValueError('side is %r: \'source\' or \'receiver\'' % (side,))
        self._checkLinearisation(linearisation)
        if kind == 'gaussNewton':
            self._refuse3('%s(kind=\'gaussNewton\')' % (what,), 'the Gauss-Newton diagonal needs nrec back-solves through A^T per frequency, and a 3-D solve is iterative; '
                                                             'kind=\'pseudoHessian\' reads the forward fields alone and Hvec applies the Gauss-Newton Hessian')
        if kind == 'energy':
            raise ValueError('kind=\'energy\' has no linearisation: linearisation=%r, parameter=%r go with kind=\'pseudoHessian\'' % (linearisation, parameter))
        if isinstance(parameter, str) and parameter in ('Q', 'cQ'):
            self._refuse3('%s(parameter=%r)' % (what, parameter), 'the visco wrappers and the chain from (c, Q) to the complex velocity are those of the 2-D '
                                                                   'operators (parameter \'c\' and \'rho\' are served)')
        if not blocks and isinstance(parameter, str) and parameter == 'joint':
            raise ValueError('illumination returns one value per cell: parameter=\'joint\' has a 2 x 2 block per cell, which hessianBlocks(kind=\'pseudoHessian\') returns')
        self._checkParameter(parameter, linearisation, joint=blocks)
        if side == 'receiver':
            self._refuse3('%s(side=\'receiver\', linearisation=%r)' % (what, linearisation),
                          'the exact kinds are the source-side sums over the forward fields; side=\'receiver\' is served by the \'scaler\' kinds \'energy\' and \'pseudoHessian\'')
        self.updateModel(m)                # (a dict may bring the `rho` that decides what is served)
        if blocks and not self._hasDensity():
            raise NotImplementedError('hessianBlocks needs an explicit `rho` in the config: without one the density follows the velocity (Gardner) and is no parameter '
                                      'of its own, so there is no (c, rho) block -- illumination(linearisation=\'full\', parameter=\'c\') is the diagonal of the total '
                                      'derivative (give `rho`, e.g. 310 c^0.25 as an array, for the blocks)')
        if self.fieldsDtype != 'complex128':
            raise NotImplementedError('%s(linearisation=%r) reads a complex128 store: fieldsDtype=%r is not served by the 3-D kernels (leave fieldsDtype at its default)'
                                      % (what, linearisation, self.fieldsDtype))
        if not getattr(self, '_derivatives3D', False) and (parameter != 'c' or not self._hasDensity()):
            raise NotImplementedError('%s(linearisation=%r, parameter=%r)%s needs derivatives3D=True beside hessian3D=True: the density rows and the Gardner total '
                                      'derivative are built on the buoyancy maps that key serves (parameter=\'c\' with an explicit `rho` needs hessian3D alone)'
                                      % (what, linearisation, parameter, '' if self._hasDensity() else ' without `rho` in the config'))
        parameter, gardner = self._requireExact3('%s(linearisation=%r)' % (what, linearisation), parameter, linearisation)
        sv = self.survey
        N = self.nrow
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                from . import device_survey3d
                return device_survey3d.pseudoHessianFromFields3(self, F, parameter, gardner, bool(perFreq), blocks)
            shape = (3, N) if blocks else (N,)
            H = np.zeros(((sv.nfreq,) + shape) if perFreq else shape, dtype=np.float64)
            st = complex(self.system.scaleTerm)
            a2 = st.real * st.real + st.imag * st.imag
            for ifreq in self.ownedFreqs:
                op = self.system.subProblems[ifreq]
                uf = np.asarray(F[ifreq])
                uh = np.conj(uf.reshape((uf.shape[0], -1)) / st)
                if blocks:
                    E = frechet3d.pseudoHessianBlocks3(op, uh)
                else:
                    E = frechet3d.pseudoHessianDiagonal3(op, uh, parameter, frechet3d.gardnerChain3(op) if gardner else None)
                if perFreq:
                    H[ifreq] = a2 * E
                else:
                    H += a2 * E
        if self._sharded:
            H = parallel.allreduce_sum(H)
        return H

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
        if getattr(self, '_derivatives3D', False):
            self.updateModel(m)              # (a dict may bring the `rho` that decides what is served)
            m = None
        parameter, gardner = self._requireExact3('Jtvec(linearisation=%r)' % (linearisation,), parameter, linearisation)
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
                return device_survey3d.gradientFromFields3(self, F, self._deviceBackSources(rd), rd, adj, parameter, gardner)
            N = self.nrow
            wantC, wantB = gardner or parameter in ('c', 'joint'), gardner or parameter in ('rho', 'joint')
            g = np.zeros(2 * N if parameter == 'joint' else N, dtype=np.float64)
            gb = g[N:] if parameter == 'joint' else g
            st = complex(self.system.scaleTerm)
            qb = [q.conj() for q in sv.getResidualSources(np.conj(resid))]        # R_s^H r_s = conj(R_s^T conj(r_s))
            M = None
            for ifreq, uB in self._solveOwned(qb, adj):
                op = self.system.subProblems[ifreq]
                M = frechet3d.massStencil3(op.modelDims) if M is None else M
                uh, lam, w = np.conj(np.asarray(F[ifreq]) / st), np.conj(np.asarray(uB) / st), -np.conj(st) / complex(op.premul)
                if wantC:
                    P = frechet3d.imagingSum3(op, uh, lam, M)
                    g[:N] += (w * frechet3d.velocityChain3(op) * P).real
                if wantB:
                    chain = frechet3d.gardnerChain3(op) if gardner else frechet3d.densityChain3(op)
                    gb += chain * (w * frechet3d.buoyancyImaging3(op, uh, lam, frechet3d.lapStencil3(op), M)).real
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
        if getattr(self, '_derivatives3D', False):
            self.updateModel(m)
            m = None
        parameter, gardner = self._requireExact3('JvecBorn(linearisation=%r)' % (linearisation,), parameter, linearisation)
        self.updateModel(m)
        sv = self.survey
        if parameter == 'joint':
            dc, dbuoy = self._splitJoint(v, 'JvecBorn')
        else:
            dc = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape((self.nrow,)))
            dc, dbuoy = (None, dc) if parameter == 'rho' else (dc, dc if gardner else None)
        with self._forwardFields(u) as F:
            if isinstance(F, DeviceFields):
                from . import device_survey3d
                data = device_survey3d.bornFromFields3(self, F, dc) if dbuoy is None else device_survey3d.bornFromFields3(self, F, dc, dbuoy, gardner)
            else:
                data = np.zeros((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
                st = complex(self.system.scaleTerm)
                subs = self.system.subProblems
                owned = self.ownedFreqs
                M = frechet3d.massStencil3(subs[0].modelDims) if owned else None

                def sources(i):
                    uh = np.conj(np.asarray(F[i]) / st)
                    q = 0.0 if dc is None else frechet3d.bornSources3(subs[i], dc, uh, M)
                    if dbuoy is not None:
                        chain = frechet3d.gardnerChain3(subs[i]) if gardner else frechet3d.densityChain3(subs[i])
                        q = q + frechet3d.buoyancySources3(subs[i], chain * dbuoy, uh, frechet3d.lapStencil3(subs[i]), M)
                    return q / -complex(subs[i].premul)
                qv = [sources(i) if i in owned else None for i in range(sv.nfreq)]
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
