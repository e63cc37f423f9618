"""The data misfit: its value, its adjoint source and its gradient, with the unknown source signature estimated per frequency or per shot.

Symbols: p = dpred(m), (nrec, nsrc, nfreq); d = dobs, the same shape; w2 >= 0 real, data-shaped (0 marks a dead trace, which is selected away and never
evaluated: it may hold NaN in d); s a complex source factor per (source, frequency); q = s p, r = q - d.  Every kind gives a value phi and psi = grad_q phi
under <a, b> = Re sum conj(a) b, the inner product under which Jtvec(adjoint='transpose') is the adjoint of JvecBorn:

    'l2'            phi = 1/2 sum w2 |r|^2                                  psi = w2 r
    'huber'         a = sqrt(w2) |r|;  phi = sum (a <= t ? a^2 / 2 : t a - t^2 / 2)      psi = (a <= t ? w2 r : t sqrt(w2) r / |r|)
    'hybrid'        phi = sum eps^2 (sqrt(1 + w2 |r|^2 / eps^2) - 1)        psi = w2 r / sqrt(1 + w2 |r|^2 / eps^2)
    'logarithmic'   rho = q / d, L = ln |rho|, theta = arg rho;  phi = 1/2 sum w2 (alpha L^2 + beta theta^2)       psi = w2 (alpha L + i beta theta) / conj(q)

The source factor is s = a / b with a = sum w2 conj(p) d and b = sum w2 |p|^2 over the samples of a group (a frequency, or one (source, frequency)): the
weighted least-squares estimate, for every kind.  The adjoint source is the gradient of the functional the user evaluates, the dependence of s on p included.
s is not holomorphic in p:  ds = (sum w2 d conj(dp)) / b - s (2 Re sum w2 conj(p) dp) / b,  and  d phi = Re sum conj(psi) (s dp + p ds), so with
c = sum_group conj(psi) p

    v = conj(s) psi + w2 ((c / b) d - (2 Re(c s) / b) p)

and the second term vanishes for 'l2' (c = conj(s b - a) = 0: variable projection).

The module-level functions (`sourceEstimate`, `terms`, `adjointSource`, `gaussNewtonWeights`) are numpy and take the precision of their arguments: the tests
run them in np.clongdouble.  `DataMisfit` joins them to a problem through `survey.dpred` and `Jtvec(adjoint='transpose')`."""
import numpy as np

KINDS = ('l2', 'huber', 'hybrid', 'logarithmic')
SOURCES = ('given', 'perFrequency', 'perSource')
_PARAMS = {'l2': (), 'huber': ('threshold',), 'hybrid': ('epsilon',), 'logarithmic': ('amplitude', 'phase')}


def _real(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def _checkKind(kind, params):
    if kind not in KINDS:
        raise ValueError('kind is %r: one of %s' % (kind, ', '.join(repr(k) for k in KINDS)))
    for key in params:
        if key not in _PARAMS[kind]:
            raise ValueError('kind=%r takes %s, not %r' % (kind, ', '.join(_PARAMS[kind]) or 'no parameters', key))
    for key in _PARAMS[kind]:
        if key not in params:
            raise ValueError('kind=%r needs %s' % (kind, key))
    if kind == 'huber' and not params['threshold'] > 0:
        raise ValueError('threshold is %r: it must be positive' % (params['threshold'],))
    if kind == 'hybrid' and not params['epsilon'] > 0:
        raise ValueError('epsilon is %r: it must be positive' % (params['epsilon'],))
    if kind == 'logarithmic' and not (params['amplitude'] >= 0 and params['phase'] >= 0):
        raise ValueError('amplitude and phase are %r and %r: neither may be negative' % (params['amplitude'], params['phase']))


def _checkSource(source):
    if source not in SOURCES:
        raise ValueError('source is %r: one of %s' % (source, ', '.join(repr(k) for k in SOURCES)))


def _weights(w2, p):
    'w2 broadcast to the data, in the real type of p; None: ones'
    real = _real(p.dtype)
    if w2 is None:
        return np.ones(p.shape, dtype=real)
    return np.broadcast_to(np.asarray(w2, dtype=real), p.shape)


def _groupSum(x, source):
    'the sums of a group, as (nsrc, nfreq): over receivers and sources of a frequency, or over the receivers of one (source, frequency)'
    if source == 'perFrequency':
        return np.broadcast_to(x.sum(axis=(0, 1))[None, :], x.shape[1:])
    return x.sum(axis=0)


def _groupName(source, isrc, ifreq):
    return 'frequency %d' % ifreq if source == 'perFrequency' else 'source %d of frequency %d' % (isrc, ifreq)


def moments(p, d, w2=None, source='perFrequency'):
    'a = sum w2 conj(p) d and b = sum w2 |p|^2 over the groups of `source`, both (nsrc, nfreq); samples with w2 = 0 are selected away'
    _checkSource(source)
    p = np.asarray(p)
    w = _weights(w2, p)
    live = w > 0
    zero = p.dtype.type(0)
    pd = np.where(live, w * np.conj(p) * np.where(live, np.asarray(d, dtype=p.dtype), zero), zero)
    pp = np.where(live, w * (p.real * p.real + p.imag * p.imag), _real(p.dtype).type(0))
    return _groupSum(pd, source), _groupSum(pp, source)


def sourceEstimate(p, d, w2=None, source='perFrequency', sourceTerms=None):
    """s, (nsrc, nfreq) in the complex type of p: `sourceTerms` (default ones) for 'given', else the weighted least-squares estimate a / b of every group.
    A group with b = 0 (no live sample, or no predicted energy) has no estimate: ValueError naming it."""
    _checkSource(source)
    p = np.asarray(p)
    if source == 'given':
        if sourceTerms is None:
            return np.ones(p.shape[1:], dtype=p.dtype)
        return np.array(np.broadcast_to(np.asarray(sourceTerms, dtype=p.dtype), p.shape[1:]))
    a, b = moments(p, d, w2, source)
    if np.any(b == 0):
        isrc, ifreq = [int(i[0]) for i in np.nonzero(b == 0)]
        raise ValueError('no source estimate for %s: its weighted predicted energy sum w2 |p|^2 is zero' % _groupName(source, isrc, ifreq))
    return a / b


def _psi(p, d, s, w, kind, params):
    'phi per sample, psi, and the live mask; the dead samples hold zeros'
    cplx, real = p.dtype, _real(p.dtype)
    live = w > 0
    one, zero = real.type(1), real.type(0)
    ws = np.where(live, w, one)
    q = np.asarray(s, dtype=cplx)[None, :, :] * p
    ds = np.where(live, np.asarray(d, dtype=cplx), cplx.type(1))
    if kind == 'logarithmic':
        qs = np.where(live, q, cplx.type(1))
        rho = qs / ds
        L = np.log(np.abs(rho))
        th = np.arctan2(rho.imag, rho.real)
        al, be = real.type(params['amplitude']), real.type(params['phase'])
        phi = ws * (al * L * L + be * th * th) / 2
        psi = ws * (al * L + 1j * (be * th)).astype(cplx) / np.conj(qs)
    else:
        r = q - ds
        r2 = r.real * r.real + r.imag * r.imag
        if kind == 'l2':
            phi, psi = ws * r2 / 2, ws * r
        elif kind == 'huber':
            t = real.type(params['threshold'])
            sw = np.sqrt(ws)
            ar = np.sqrt(r2)
            a = sw * ar
            small = a <= t
            phi = np.where(small, a * a / 2, t * a - t * t / 2)
            psi = np.where(small, ws * r, (t * sw / np.where(small, one, ar)) * r)
        else:
            e = real.type(params['epsilon'])
            root = np.sqrt(1 + ws * r2 / (e * e))
            phi, psi = ws * r2 / (1 + root), ws * r / root          # (eps^2 (root - 1) without the cancellation)
    return np.where(live, phi, zero), np.where(live, psi, cplx.type(0)), live


def terms(p, d, s, w2=None, kind='l2', source='given', **params):
    """phi (a scalar), psi (data-shaped) and c = sum_group conj(psi) p (nsrc, nfreq; the groups of 'given' are those of 'perSource') at the source factors
    s (nsrc, nfreq).  Samples with w2 = 0 are selected away."""
    _checkKind(kind, params)
    _checkSource(source)
    p = np.asarray(p)
    phi, psi, live = _psi(p, d, s, _weights(w2, p), kind, params)
    c = _groupSum(np.where(live, np.conj(psi) * p, p.dtype.type(0)), source)
    return phi.sum(), psi, c


def adjointSource(p, d, w2=None, kind='l2', source='given', sourceTerms=None, projection=True, **params):
    """v with d phi = Re sum conj(v) dp, phi the reduced functional (s a function of p unless it is given): conj(s) psi, plus for an estimated source the
    term through the estimate, w2 ((c / b) d - (2 Re(c s) / b) p).  projection=False leaves that term out: the gradient at FIXED s, which is not the gradient
    of the functional evaluated (the tests seed it as the mistake to catch)."""
    p = np.asarray(p)
    s = sourceEstimate(p, d, w2, source, sourceTerms)
    _, psi, c = terms(p, d, s, w2, kind, source, **params)
    v = np.conj(s)[None, :, :] * psi
    if source != 'given' and projection:
        w = _weights(w2, p)
        live = w > 0
        _, b = moments(p, d, w2, source)
        zero = p.dtype.type(0)
        dsafe = np.where(live, np.asarray(d, dtype=p.dtype), zero)
        v = v + np.where(live, w * ((c / b)[None, :, :] * dsafe - (2 * (c * s).real / b)[None, :, :] * p), zero)
    return v


def gaussNewtonWeights(p, d, s, w2=None, kind='l2', **params):
    """The real diagonal W >= 0 with  d psi ~ W' dq  and hence H_GN = J^H diag(|s|^2 W') J at fixed s, as `Hvec(weights=)` takes it:
    |s|^2 w2 ('l2'), |s|^2 (a <= t ? w2 : t sqrt(w2) / |r|) ('huber'), |s|^2 w2 / sqrt(1 + w2 |r|^2 / eps^2) ('hybrid'), alpha w2 / |p|^2 ('logarithmic' with
    alpha = beta; otherwise the curvature is not a real diagonal in the data).  The projection term of the source estimate is left out."""
    _checkKind(kind, params)
    p = np.asarray(p)
    cplx, real = p.dtype, _real(p.dtype)
    w = _weights(w2, p)
    live = w > 0
    one, zero = real.type(1), real.type(0)
    ws = np.where(live, w, one)
    s = np.asarray(s, dtype=cplx)
    s2 = (s.real * s.real + s.imag * s.imag)[None, :, :]
    if kind == 'logarithmic':
        if params['amplitude'] != params['phase']:
            raise NotImplementedError('with amplitude != phase the curvature of the logarithmic misfit is not a real diagonal in the data')
        ps = np.where(live, p, cplx.type(1))
        out = real.type(params['amplitude']) * ws / (ps.real * ps.real + ps.imag * ps.imag)
        return np.where(live, out, zero)
    r = s[None, :, :] * p - np.where(live, np.asarray(d, dtype=cplx), cplx.type(1))
    r2 = r.real * r.real + r.imag * r.imag
    if kind == 'l2':
        out = ws
    elif kind == 'huber':
        t = real.type(params['threshold'])
        sw, ar = np.sqrt(ws), np.sqrt(r2)
        small = sw * ar <= t
        out = np.where(small, ws, t * sw / np.where(small, one, ar))
    else:
        e = real.type(params['epsilon'])
        out = ws / np.sqrt(1 + ws * r2 / (e * e))
    return np.where(live, s2 * out, zero)


class DataMisfit(object):
    """phi = DataMisfit(prob, dobs, kind='l2', weights=None, source='given', sourceTerms=None, **params)

        val    = phi(m)                                        float
        val, g = phi.valueAndGradient(m, u=None, parameter='c', linearisation='full')      g as Jtvec(adjoint='transpose') returns it
        phi.sourceTerms                                        (nsrc, nfreq) complex128, the s of the last evaluation
        phi.adjointSource(m, u=None)                           (nrec, nsrc, nfreq): the v with g = prob.Jtvec(m, v, adjoint='transpose', ...)
        phi.gaussNewtonWeights(m, u=None)                      real >= 0, data-shaped: prob.Hvec(m, x, weights=...) is the Gauss-Newton product at fixed s

    kind: 'l2'; 'huber' (threshold=t > 0); 'hybrid' (epsilon > 0); 'logarithmic' (amplitude >= 0, phase >= 0; dobs != 0 wherever the weight is positive).
    weights: w2 >= 0, data-shaped or broadcastable to (nrec, nsrc, nfreq); a sample with weight 0 is never evaluated and may hold anything in dobs.
    source: 'given' (sourceTerms, default ones), 'perFrequency' or 'perSource': the weighted least-squares estimate of the module's docstring, for every
    kind; the gradient is that of the reduced functional, the dependence of the estimate on the model included.

    Every problem class, parameter and linearisation that the problem's own Jtvec(adjoint='transpose') serves is served: the predicted data come from
    `survey.dpred(m, u=)`, the adjoint source from the numpy functions of this module, and the gradient from `prob.Jtvec(m, v, u=, adjoint='transpose', ...)`,
    which refuses what it refuses with its own sentence.  `u` is whatever those two take (None, a host list, a DeviceFields).  Under sharded frequencies the
    data are all-reduced by `dpred`, so the value and the source terms are the same on every rank, and `Jtvec` all-reduces the gradient.

    `valueAndGradient` on a Helm2DProblem over MiniZephyr / MiniZephyrHD on one grid, with the device path, parameter 'c', 'rho' or 'joint', linearisation
    'operator' or 'full' and u a DeviceFields or None, keeps the data on the device (device_survey.misfitFromFields): the samples are turned into the adjoint
    source where the sampling kernel wrote them, and 3 k doubles per item and pass come down.  With u None and no group of the source estimate spanning two
    work items ('given', 'perSource', or every frequency's columns in one item) it runs in ONE pass without a store (device_survey.misfitOnePass): an item
    solves its forward columns, makes its adjoint source, back-propagates and images, and only its own fields are held -- the factors of A and of A^T are
    resident side by side.  'perFrequency' over several items with u None solves an internal store and releases it.  The route is chosen silently; the config
    key misfitHostData=True keeps to the generic one."""

    def __init__(self, prob, dobs, kind='l2', weights=None, source='given', sourceTerms=None, **params):
        _checkKind(kind, params)
        _checkSource(source)
        prob._requirePaired()
        sv = prob.survey
        self.prob, self.kind, self.source, self.params = prob, kind, source, dict(params)
        self.shape = (sv.nrec, sv.nsrc, sv.nfreq)
        self.dobs = np.array(np.asarray(dobs, dtype=np.complex128).reshape(self.shape))
        if weights is None:
            self.weights = None
        else:
            w = np.asarray(weights, dtype=np.float64)
            if not np.all(w >= 0):                                        # (NaN fails too)
                raise ValueError('weights must be real and >= 0 (0 marks a dead trace)')
            self.weights = np.array(np.broadcast_to(w, self.shape))
        if source == 'given' and sourceTerms is not None:
            self._given = np.array(np.broadcast_to(np.asarray(sourceTerms, dtype=np.complex128), self.shape[1:]))
        elif sourceTerms is not None:
            raise ValueError('sourceTerms are given and source is %r: an estimated source takes none' % (source,))
        else:
            self._given = None
        live = np.ones(self.shape, dtype=bool) if self.weights is None else self.weights > 0
        if kind == 'logarithmic' and np.any(live & ~(np.abs(self.dobs) > 0)):
            raise ValueError("kind='logarithmic' needs dobs != 0 wherever the weight is positive: %d samples are zero or NaN"
                             % int(np.count_nonzero(live & ~(np.abs(self.dobs) > 0))))
        self.sourceTerms = None
        self._devicePanels = {}            # (GPU, ifreq, c0, c1) -> the item's dobs and weight panels there (device_survey._misfitData)

    def _deviceServes(self, u, parameter, linearisation):
        "True where `valueAndGradient` keeps the data on the device"
        from .fieldstore import DeviceFields
        from .minizephyr import MiniZephyr, MiniZephyrHD
        from .problem import Helm2DProblem
        from .survey import HelmMultiGridSurvey
        prob = self.prob
        if getattr(prob, '_misfitHostData', False) or not isinstance(prob, Helm2DProblem) or isinstance(prob.survey, HelmMultiGridSurvey):
            return False
        if parameter not in ('c', 'rho', 'joint') or linearisation not in ('operator', 'full') or not (u is None or isinstance(u, DeviceFields)):
            return False
        if prob._isVisco() or prob._kyServed() or prob._multiscaleServed() or not prob._deviceGradientAvailable():
            return False
        subs = prob.system.subProblems
        return bool(subs) and type(subs[0]) in (MiniZephyr, MiniZephyrHD)

    def _valueAndGradientDevice(self, u, parameter, linearisation):
        "the model is current and the refusals of Jtvec are past: (value, gradient) with the data kept on the device"
        from . import device_survey
        prob = self.prob
        linearisation = prob._resolveLinearisation(linearisation, parameter, 'Jtvec')
        if u is not None:
            val, s, g = device_survey.misfitFromFields(prob, u, self, linearisation, parameter)
        else:
            owned = prob.ownedFreqs
            items = device_survey.deviceItems(prob.system, owned, prob.survey.nsrc)[1] if owned else []
            if device_survey.misfitInOnePass(self, items):
                val, s, g = device_survey.misfitOnePass(prob, self, linearisation, parameter)
            else:
                F = prob.fieldsDevice()
                try:
                    val, s, g = device_survey.misfitFromFields(prob, F, self, linearisation, parameter)
                finally:
                    F.release()
        self.sourceTerms = s
        if parameter == 'rho':
            g = prob._buoyancyChain() * g
        elif parameter == 'joint':
            g[prob.nrow:] *= prob._buoyancyChain()
        return val, g

    def _predict(self, m, u):
        return np.asarray(self.prob.survey.dpred(m, u=u), dtype=np.complex128).reshape(self.shape)

    def _estimate(self, p):
        self.sourceTerms = sourceEstimate(p, self.dobs, self.weights, self.source, self._given)
        return self.sourceTerms

    def value(self, m=None, u=None):
        p = self._predict(m, u)
        phi, _, _ = terms(p, self.dobs, self._estimate(p), self.weights, self.kind, self.source, **self.params)
        return float(phi)

    __call__ = value

    def adjointSource(self, m=None, u=None):
        p = self._predict(m, u)
        self._estimate(p)
        return adjointSource(p, self.dobs, self.weights, self.kind, self.source, self._given, **self.params)

    def gaussNewtonWeights(self, m=None, u=None):
        p = self._predict(m, u)
        return gaussNewtonWeights(p, self.dobs, self._estimate(p), self.weights, self.kind, **self.params)

    def valueAndGradient(self, m=None, u=None, parameter='c', linearisation='full'):
        """(phi(m), its gradient): the adjoint source handed to prob.Jtvec(m, v, u=u, adjoint='transpose', linearisation=, parameter=).  With u None the
        forward fields are solved by `dpred` and again by `Jtvec`; solve them once (`fieldsDevice()` or `fields()`) and pass them to avoid that."""
        prob = self.prob
        prob.updateModel(m)
        if self._deviceServes(u, parameter, linearisation):
            if u is not None:
                u.checkCurrent(prob)
            return self._valueAndGradientDevice(u, parameter, linearisation)
        p = self._predict(m, u)
        s = self._estimate(p)
        phi, _, _ = terms(p, self.dobs, s, self.weights, self.kind, self.source, **self.params)
        v = adjointSource(p, self.dobs, self.weights, self.kind, self.source, self._given, **self.params)
        g = self.prob.Jtvec(m, v, u=u, adjoint='transpose', linearisation=linearisation, parameter=parameter)
        return float(phi), g
