"""CPU: the data misfit of zephyr_amd/misfit.py.  Data space in 80-bit arithmetic: the adjoint source is the gradient of the reduced functional for every kind
and source mode (and the one without the term through the source estimate is not); 'l2' has the variable-projection property.  Model space on the oracle
doubles, through the generic route (dpred, the numpy functions, Jtvec(adjoint='transpose')): central differences of the reduced functional against g . v for
'c' and 'joint', a visco 'cQ' case, a 2.5-D case and a 3-D case; dead traces, refusals, and the Gauss-Newton weights."""
import numpy as np
import pytest

from tests import frechet_cases as fc
from tests import misfit_cases as mc
from zephyr_amd import DataMisfit
from zephyr_amd import misfit as mf

CLD, LD = mc.CLD, mc.LD
ESTIMATED = ('perFrequency', 'perSource')


# ---- data space -------------------------------------------------------------------------------------------------------------------------------------
SHAPE = (7, 5, 3)
STEPS = (4e-3, 2e-3, 1e-3)


def data_case(seed=1):
    'p, d, w2 (7, 5, 3) and a direction dp with |dp| <= 1, in 80-bit; w2 with dead samples that hold NaN in d'
    rng = np.random.default_rng(seed)
    parts = [mc.panel_inputs(SHAPE[0], SHAPE[1], seed + f) for f in range(SHAPE[2])]
    p, d, w2 = (np.stack([q[i] for q in parts], axis=2) for i in range(3))
    s = np.stack([q[3] for q in parts], axis=1)
    dp = rng.uniform(0.2, 1., SHAPE) * np.exp(1j * rng.uniform(-np.pi, np.pi, SHAPE))
    return p.astype(CLD), d.astype(CLD), w2.astype(LD), s.astype(CLD), dp.astype(CLD)


def gap_threshold(a):
    'a threshold in the widest relative gap between the sorted values a (the middle half of them): samples on both sides, none near it'
    a = np.sort(np.asarray(a, dtype=np.float64).ravel())
    lo, hi = len(a) // 4, 3 * len(a) // 4
    i = lo + int(np.argmax(a[lo + 1:hi + 1] / a[lo:hi]))
    return float(np.sqrt(a[i] * a[i + 1])), float(a[i + 1] / a[i])


def huber_levels(p, d, w2, source, given):
    'a = sqrt(w2) |s p - d| of the live samples at the source factors of `source`'
    s = mf.sourceEstimate(p, d, w2, source, given)
    live = np.ones(p.shape, dtype=bool) if w2 is None else np.asarray(w2) > 0
    r = np.where(live, s[None] * p - np.where(live, d, 1), 0)
    return (np.sqrt(np.where(live, 1 if w2 is None else w2, 0)) * np.abs(r))[live]


def reduced(p, d, w2, kind, source, given, params):
    return mf.terms(p, d, mf.sourceEstimate(p, d, w2, source, given), w2, kind, source, **params)[0]


def data_ratios(kind, source, projection=True):
    p, d, w2, s, dp = data_case()
    given = s if source == 'given' else None
    params = dict(mc.PARAMS[kind])
    if kind == 'huber':
        t, gap = gap_threshold(huber_levels(p, d, w2, source, given))
        assert gap > 1.02
        params['threshold'] = t
        below = huber_levels(p, d, w2, source, given) <= t
        assert 0 < np.count_nonzero(below) < below.size
        for h in STEPS:          # the no-crossing condition: the set {a <= t} is the same at every evaluated point
            for sign in (1, -1):
                assert np.array_equal(huber_levels(p + sign * LD(h) * dp, d, w2, source, given) <= t, below)
    v = mf.adjointSource(p, d, w2, kind, source, given, projection=projection, **params)
    lin = (np.conj(v) * dp).real.sum()
    errs = [abs((reduced(p + LD(h) * dp, d, w2, kind, source, given, params) - reduced(p - LD(h) * dp, d, w2, kind, source, given, params)) / (2 * LD(h)) - lin)
            for h in STEPS]
    return [float(e / abs(lin)) for e in errs], [float(errs[i] / errs[i + 1]) for i in range(2)]


@pytest.mark.parametrize('source', mc.SOURCES)
@pytest.mark.parametrize('kind', mc.KINDS)
def test_the_adjoint_source_is_the_gradient_of_the_reduced_functional(kind, source):
    """(phi(p + h dp) - phi(p - h dp)) / 2h approaches Re sum conj(v) dp with the error falling >= 3.5x per halving, in 80-bit arithmetic, s re-estimated at
    every point.  'l2' with a given source is a quadratic: its central difference is exact and the error is rounding (below 1e-15 relative, no ratio)."""
    rel, ratios = data_ratios(kind, source)
    print('%s %s: relative errors %s, ratios %s' % (kind, source, rel, ratios))
    if kind == 'l2' and source == 'given':
        assert max(rel) < 1e-15
    else:
        assert min(ratios) >= mc.TAYLOR


@pytest.mark.parametrize('source', ESTIMATED)
@pytest.mark.parametrize('kind', ['hybrid', 'logarithmic'])
def test_without_the_term_through_the_estimate_it_is_not(kind, source):
    'the seeded mistake: the adjoint source at FIXED s fails the same check (its error does not fall: the ratios stay near 1)'
    rel, ratios = data_ratios(kind, source, projection=False)
    print('%s %s without the second term: relative errors %s, ratios %s' % (kind, source, rel, ratios))
    assert min(ratios) < mc.TAYLOR


@pytest.mark.parametrize('dtype', [np.complex128, CLD])
@pytest.mark.parametrize('source', ESTIMATED)
def test_l2_has_the_variable_projection_property(source, dtype):
    '|c| <= 64 u sum |psi| |p| over the group: the second term of v vanishes for least squares, and v is conj(s) psi'
    p, d, w2, _, _ = data_case(seed=3)
    real = LD if dtype is CLD else np.float64
    p, d, w2 = p.astype(dtype), d.astype(dtype), w2.astype(real)
    u = float(np.finfo(real).eps) / 2
    s = mf.sourceEstimate(p, d, w2, source)
    _, psi, c = mf.terms(p, d, s, w2, 'l2', source)
    bound = 64 * u * mf._groupSum(np.abs(psi) * np.abs(p), source)
    print('worst |c| / bound: %.3g' % float(np.max(np.abs(c) / bound)))
    assert np.all(np.abs(c) <= bound)
    v = mf.adjointSource(p, d, w2, 'l2', source)
    assert np.max(np.abs(v - np.conj(s)[None] * psi)) <= 64 * u * np.max(np.abs(v))


@pytest.mark.parametrize('source', mc.SOURCES)
@pytest.mark.parametrize('kind', mc.KINDS)
def test_dead_samples_change_nothing(kind, source):
    'a sample with w2 = 0 is selected away: NaN, zero or anything else in its dobs gives the same bits of phi, s, psi, c and v'
    p, d, w2, s, _ = data_case(seed=4)
    p, d, w2, s = p.astype(np.complex128), d.astype(np.complex128), w2.astype(np.float64), s.astype(np.complex128)
    dead = w2 == 0
    assert np.count_nonzero(dead) > 5 and np.all(np.isnan(d[dead]))
    given = s if source == 'given' else None
    out = []
    for fill in (np.nan, 0., 3. - 2j):
        dd = np.where(dead, fill, d)
        se = mf.sourceEstimate(p, dd, w2, source, given)
        phi, psi, c = mf.terms(p, dd, se, w2, kind, source, **mc.PARAMS[kind])
        v = mf.adjointSource(p, dd, w2, kind, source, given, **mc.PARAMS[kind])
        assert np.isfinite(phi) and np.all(np.isfinite(v)) and np.all(v[dead] == 0) and np.all(psi[dead] == 0)
        out.append(np.concatenate([[phi], se.ravel(), psi.ravel(), c.ravel(), v.ravel()]))
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize('kind', mc.ALGEBRAIC)
def test_gauss_newton_weights_against_a_finite_difference_of_psi(kind):
    """psi = W(|r|) r with W real, so along a rotation of r, dr = i r h, d psi / dh = i W r exactly: the central difference of psi along dr = +- i h r (dobs
    moved by -+ i h r at fixed s) equals i (weights / |s|^2) r to O(h^2)."""
    p, d, w2, s, _ = data_case(seed=6)
    live = w2 > 0
    d = np.where(live, d, 1)
    params = mc.PARAMS[kind]
    r = np.where(live, s[None] * p - d, 0)
    gn = mf.gaussNewtonWeights(p, d, s, w2, kind, **params)
    assert gn.dtype == LD and np.all(gn >= 0) and np.all(gn[~live] == 0)
    h = LD(1e-5)
    psi = lambda dd: mf.terms(p, dd, s, w2, kind, 'given', **params)[1]
    fd = (psi(d - 1j * h * r) - psi(d + 1j * h * r)) / (2 * h)
    want = 1j * (gn / (np.abs(s) ** 2)[None]) * r
    err = float(np.max(np.abs(fd - want)) / np.max(np.abs(want)))
    print('%s: relative difference %.3g' % (kind, err))
    assert err < 1e-8


def test_gauss_newton_weights_of_the_logarithmic_kind():
    p, d, w2, s, _ = data_case(seed=6)
    gn = mf.gaussNewtonWeights(p, d, s, w2, 'logarithmic', amplitude=0.8, phase=0.8)
    live = w2 > 0
    assert np.allclose(np.asarray(gn[live], dtype=float), np.asarray(0.8 * w2[live] / np.abs(p[live]) ** 2, dtype=float), rtol=1e-15)
    with pytest.raises(NotImplementedError, match='not a real diagonal in the data'):
        mf.gaussNewtonWeights(p, d, s, w2, 'logarithmic', amplitude=1.0, phase=0.7)


# ---- model space: the oracle doubles, the generic route -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pairs():
    'mode -> (prob, survey, c0, dobs, direction): the 37 x 53 case, fixed and moving (the moving one with the HD class and a complex scaleTerm)'
    out = {}
    for mode, hd in (('fixed', False), ('relative', True)):
        prob, sv = fc.host_pair(mode, hd)
        c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
        d1 = sv.dpred(c0 + fc.perturbation(seed=12).reshape(c0.shape))
        dobs = mc.observed(sv, None, d1)
        out[mode] = (prob, sv, c0, dobs, fc.perturbation(seed=13))
    return out


def model_params(kind, prob, sv, c0, dobs, source):
    "the kind's parameters at the scale of the data: epsilon = the median |r| at c0; 'huber': a threshold in the widest gap of a = |r|"
    if kind not in ('huber', 'hybrid'):
        return dict(mc.PARAMS[kind])
    p = sv.dpred(c0).reshape(dobs.shape)
    a = huber_levels(p, dobs, None, source, None)
    if kind == 'hybrid':
        return dict(epsilon=float(np.median(a)))
    return dict(threshold=gap_threshold(a)[0])


def model_ratios(prob, phi, c0, v, **kw):
    val, g = phi.valueAndGradient(c0, **kw)
    assert g.dtype == np.float64 and val == phi(c0)
    errs, ratios, lin = mc.central_ratios(lambda c: phi(c), g, c0, v)
    prob.updateModel(c0)
    return [e / abs(lin) for e in errs], ratios


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
@pytest.mark.parametrize('source', mc.SOURCES)
@pytest.mark.parametrize('kind', ['l2', 'hybrid', 'logarithmic'])
def test_central_differences_of_the_reduced_functional(pairs, kind, source, mode):
    """dobs from a perturbed model, scaled by 1.3 - 0.4i, 2 % noise; g through Jtvec(adjoint='transpose', linearisation='full') on the host route; the central
    differences at h = 0.25, 0.125, 0.0625 approach g . v with error ratios >= 3.5"""
    prob, sv, c0, dobs, v = pairs[mode]
    phi = DataMisfit(prob, dobs, kind=kind, source=source, **model_params(kind, prob, sv, c0, dobs, source))
    rel, ratios = model_ratios(prob, phi, c0, v)
    print('%s %s %s: relative errors %s, ratios %s' % (kind, source, mode, rel, ratios))
    assert min(ratios) >= mc.TAYLOR
    assert phi.sourceTerms.shape == (sv.nsrc, sv.nfreq) and phi.sourceTerms.dtype == np.complex128
    if source != 'given':
        assert np.max(np.abs(phi.sourceTerms - (1.3 - 0.4j))) < 0.5          # (dobs is (1.3 - 0.4i) times the data of a model nearby)


@pytest.mark.parametrize('source', mc.SOURCES)
def test_huber_under_its_no_crossing_condition(pairs, source):
    """'huber' is once differentiable: the threshold sits in the widest gap of a = |r| and the direction is short (a tenth of the others), and the test checks
    that the set {a <= t} is the same at every evaluated point before it asserts the ratios"""
    prob, sv, c0, dobs, v = pairs['fixed']
    v = 0.1 * v
    params = model_params('huber', prob, sv, c0, dobs, source)
    t = params['threshold']
    levels = lambda c: huber_levels(sv.dpred(c).reshape(dobs.shape), dobs, None, source, None) <= t
    below = levels(c0)
    assert 0 < np.count_nonzero(below) < below.size
    for h in (0.25, 0.125, 0.0625):
        for sign in (1, -1):
            assert np.array_equal(levels(c0 + sign * h * v.reshape(c0.shape)), below)
    phi = DataMisfit(prob, dobs, kind='huber', source=source, **params)
    rel, ratios = model_ratios(prob, phi, c0, v)
    print('huber %s: relative errors %s, ratios %s' % (source, rel, ratios))
    assert min(ratios) >= mc.TAYLOR


def test_the_joint_gradient(pairs):
    "parameter='joint': [g_c; g_rho] against central differences along a stacked (c, rho) direction"
    from tests import joint_cases as jc
    prob, sv, c0, dobs, _ = pairs['fixed']
    rho0 = np.array(prob.systemConfig['rho'], dtype=np.float64)
    vc, vr = fc.perturbation(seed=13), fc.perturbation(seed=14, amplitude=40.)
    phi = DataMisfit(prob, dobs, kind='hybrid', source='perFrequency', **model_params('hybrid', prob, sv, c0, dobs, 'perFrequency'))
    val, g = phi.valueAndGradient(jc.both(c0, rho0), parameter='joint', linearisation='full')
    assert g.shape == (2 * c0.size,)
    lin = float(np.dot(g, np.concatenate([vc, vr])))
    at = lambda h: jc.both(c0 + h * vc.reshape(c0.shape), rho0 + h * vr.reshape(c0.shape))
    errs = [abs((phi(at(h)) - phi(at(-h))) / (2 * h) - lin) for h in (0.25, 0.125, 0.0625)]
    prob.updateModel(jc.both(c0, rho0))
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print('joint: relative errors %s, ratios %s' % ([e / abs(lin) for e in errs], ratios))
    assert min(ratios) >= mc.TAYLOR


def test_a_visco_problem_with_cQ():
    "Helm2DViscoProblem, parameter='cQ': the generic route serves what Jtvec serves"
    from tests import visco_cases as vc
    prob, sv = vc.pair(vc.strong_config())
    shape = (fc.NZ, fc.NX)
    c0, Q0 = np.array(prob.systemConfig['c'], dtype=np.float64).reshape(shape), np.array(prob.systemConfig['Q'], dtype=np.float64).reshape(shape)
    dvc, dvQ = vc.perturbations()
    at = lambda h, a=dvc, b=dvQ: {'c': c0 + h * a.reshape(shape), 'Q': Q0 + h * b.reshape(shape)}
    dobs = mc.observed(sv, None, sv.dpred(at(1., fc.perturbation(seed=12), 0. * dvQ)))
    phi = DataMisfit(prob, dobs, kind='logarithmic', source='perSource', **mc.PARAMS['logarithmic'])
    val, g = phi.valueAndGradient(at(0.), parameter='cQ', linearisation='full')
    lin = float(np.dot(g, np.concatenate([dvc, dvQ])))
    errs = [abs((phi(at(h)) - phi(at(-h))) / (2 * h) - lin) for h in (0.25, 0.125, 0.0625)]
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print('visco cQ: relative errors %s, ratios %s' % ([e / abs(lin) for e in errs], ratios))
    assert min(ratios) >= mc.TAYLOR


def test_a_25d_problem():
    'Helm25DProblem with kyDerivatives: u None, the generic route'
    from tests import ky_exact_cases as kc
    prob, sv = kc.host_pair('fixed')
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    v = kc.perturbation(c0.size, seed=9)
    dobs = mc.observed(sv, None, sv.dpred(c0 + kc.perturbation(c0.size, seed=8).reshape(c0.shape)))
    phi = DataMisfit(prob, dobs, kind='l2', source='perFrequency')
    rel, ratios = model_ratios(prob, phi, c0, v)
    print('2.5-D: relative errors %s, ratios %s' % (rel, ratios))
    assert min(ratios) >= mc.TAYLOR


def test_a_3d_problem():
    'Helm3DProblem on the 18 x 16 x 20 oracle'
    from tests import survey3d_cases as s3
    prob, sv = s3.host_pair('18x16x20')
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    rng = np.random.default_rng(17)
    v = 50. * rng.uniform(-1., 1., c0.size)
    dobs = mc.observed(sv, None, sv.dpred(c0 + 50. * rng.uniform(-1., 1., c0.shape)))
    phi = DataMisfit(prob, dobs, kind='hybrid', source='perSource', epsilon=float(np.median(np.abs(dobs))) * 0.1)
    rel, ratios = model_ratios(prob, phi, c0, v)
    print('3-D: relative errors %s, ratios %s' % (rel, ratios))
    assert min(ratios) >= mc.TAYLOR


def test_l2_recovers_a_scaled_source(pairs):
    'dobs = kappa dpred(m): s = kappa, phi and g at rounding level'
    prob, sv, c0, _, _ = pairs['fixed']
    kappa = 0.8 + 1.7j
    p = sv.dpred(c0)
    for source in ESTIMATED:
        phi = DataMisfit(prob, kappa * p, kind='l2', source=source)
        val, g = phi.valueAndGradient(c0)
        assert np.max(np.abs(phi.sourceTerms - kappa)) < 1e-13
        ref = 0.5 * np.sum(np.abs(p) ** 2) * abs(kappa) ** 2
        g1 = DataMisfit(prob, 0 * p, kind='l2').valueAndGradient(c0)[1]          # (the gradient of 1/2 |p|^2: the scale g is small against)
        print('%s: phi / (|kappa|^2 |p|^2 / 2) = %.3g, |g| / |g of |p|^2 / 2| = %.3g' % (source, val / ref, np.linalg.norm(g) / np.linalg.norm(g1)))
        assert val < 1e-26 * ref and np.linalg.norm(g) < 1e-12 * np.linalg.norm(g1)


def test_dead_traces_through_the_problem(pairs):
    'zero-weight samples holding NaN in dobs change nothing: the same value, source terms and gradient as with finite values there'
    prob, sv, c0, dobs, _ = pairs['relative']
    w = np.ones(dobs.shape)
    w[2, :, :] = 0.
    w[:5, 1, 0] = 0.
    w[4, 3, 1] = 0.
    out = []
    for fill in (np.nan, 1.0):
        d = np.where(w > 0, dobs, fill)
        phi = DataMisfit(prob, d, kind='logarithmic', weights=w, source='perSource', **mc.PARAMS['logarithmic'])
        val, g = phi.valueAndGradient(c0)
        assert np.isfinite(val) and np.all(np.isfinite(g)) and np.all(phi.adjointSource(c0)[w == 0] == 0)
        out.append((val, phi.sourceTerms.copy(), g))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    # a weight per receiver broadcasts
    phi = DataMisfit(prob, dobs, weights=np.linspace(0.5, 2., sv.nrec)[:, None, None])
    assert phi.weights.shape == dobs.shape and np.isfinite(phi(c0))


def test_the_adjoint_source_and_the_weights_are_what_jtvec_and_hvec_take(pairs):
    prob, sv, c0, dobs, _ = pairs['fixed']
    phi = DataMisfit(prob, dobs, kind='hybrid', source='perFrequency', **model_params('hybrid', prob, sv, c0, dobs, 'perFrequency'))
    val, g = phi.valueAndGradient(c0, linearisation='operator')
    v = phi.adjointSource(c0)
    assert v.shape == dobs.shape and np.array_equal(g, prob.Jtvec(c0, v, adjoint='transpose', linearisation='operator'))
    w = phi.gaussNewtonWeights(c0)
    assert w.shape == dobs.shape and w.dtype == np.float64 and np.all(w >= 0)
    x = fc.perturbation(seed=15)
    Hx = prob.Hvec(c0, x, weights=w, linearisation='operator')
    assert Hx.shape == x.shape and float(np.dot(x, Hx)) > 0
    u = prob.fields(c0)
    assert phi.valueAndGradient(c0, u=u, linearisation='operator')[0] == val          # (a host list of fields: the generic route too)


def test_refusals(pairs):
    prob, sv, c0, dobs, _ = pairs['fixed']
    with pytest.raises(ValueError, match="kind is 'l1'"):
        DataMisfit(prob, dobs, kind='l1')
    with pytest.raises(ValueError, match="source is 'perShot'"):
        DataMisfit(prob, dobs, source='perShot')
    with pytest.raises(ValueError, match="kind='huber' needs threshold"):
        DataMisfit(prob, dobs, kind='huber')
    with pytest.raises(ValueError, match='it must be positive'):
        DataMisfit(prob, dobs, kind='hybrid', epsilon=0.)
    with pytest.raises(ValueError, match="kind='l2' takes no parameters, not 'epsilon'"):
        DataMisfit(prob, dobs, epsilon=1.)
    with pytest.raises(ValueError, match='neither may be negative'):
        DataMisfit(prob, dobs, kind='logarithmic', amplitude=-1., phase=1.)
    with pytest.raises(ValueError, match='weights must be real and >= 0'):
        DataMisfit(prob, dobs, weights=-np.ones(dobs.shape))
    with pytest.raises(ValueError, match='an estimated source takes none'):
        DataMisfit(prob, dobs, source='perSource', sourceTerms=np.ones((sv.nsrc, sv.nfreq)))
    d0 = dobs.copy()
    d0[1, 2, 0] = 0.
    with pytest.raises(ValueError, match="needs dobs != 0 wherever the weight is positive: 1 samples"):
        DataMisfit(prob, d0, kind='logarithmic', amplitude=1., phase=1.)
    w = np.ones(dobs.shape)
    w[1, 2, 0] = 0.
    DataMisfit(prob, d0, kind='logarithmic', weights=w, amplitude=1., phase=1.)          # (a dead sample may be zero)
    # a group without a live sample has no estimate, and is named
    w = np.ones(dobs.shape)
    w[:, 3, 1] = 0.
    with pytest.raises(ValueError, match='no source estimate for source 3 of frequency 1'):
        DataMisfit(prob, dobs, weights=w, source='perSource')(c0)
    w[:, :, 1] = 0.
    with pytest.raises(ValueError, match='no source estimate for frequency 1'):
        DataMisfit(prob, dobs, weights=w, source='perFrequency')(c0)
    # what Jtvec refuses is refused with its sentence
    phi = DataMisfit(prob, dobs)
    with pytest.raises(ValueError, match="linearisation is 'exact'"):
        phi.valueAndGradient(c0, linearisation='exact')
    with pytest.raises(ValueError, match="parameter is 'vp'"):
        phi.valueAndGradient(c0, parameter='vp')
    with pytest.raises(ValueError, match="MultiFreq has no Q"):
        phi.valueAndGradient(c0, parameter='Q')
    with pytest.raises(ValueError, match="parameter='joint' needs linearisation='operator' or 'full'"):
        phi.valueAndGradient(c0, parameter='joint', linearisation='scaler')
    g = phi.valueAndGradient(c0, linearisation='scaler')[1]          # (the reference's weight is served as Jtvec serves it)
    assert g.shape == (c0.size,)
    import zephyr_amd as za
    assert za.DataMisfit is DataMisfit and 'DataMisfit' in za.__all__
