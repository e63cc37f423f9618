"""CPU: parameter='rho' of JvecBorn / Jtvec / Hvec on the oracle doubles -- the buoyancy map against the oracle's own assembly, its transpose, the Taylor test
that makes it the derivative of dpred in rho (and a mass-terms-only derivative that fails it), the adjoint identities, the refusals, and the 80-bit
evaluations the device kernels are held to, checked against plain fp64 numpy and against wrong evaluations."""
import numpy as np
import pytest

import zephyr_amd as za
from oracle import helm_oracle as ho
from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from zephyr_amd import frechet as fr

CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-mz', 'fixed-hd', 'moving-mz', 'moving-hd']
OP = dict(linearisation='operator')


@pytest.fixture(scope='module')
def solved():
    'per case: the pair, the density of the config, the perturbation, the host fields and the Born data in rho -- made once, left unchanged'
    out = {}
    for key in CASES:
        prob, sv = fc.host_pair(*key)
        rho0 = np.array(prob.systemConfig['rho'], dtype=np.float64)
        v = dc.perturbation()
        uF = prob.fields()
        out[key] = dict(prob=prob, sv=sv, rho0=rho0, v=v, uF=uF, Jrho=prob.JvecBorn(None, v, u=uF, parameter='rho', **OP))
    return out


# ---- 1. the buoyancy map against the oracle's assembly --------------------------------------------------------------------------------------------
def _oracle_planes(sc, rho):
    return ho.minizephyr_coefficients(sc['nz'], sc['nx'], sc['c'], rho, complex(sc['freq']), dx=sc['dx'], dz=sc['dz'], nPML=sc['nPML'], tau=sc.get('tau', np.inf),
                                      ky=sc.get('ky', 0.0), freeSurf=sc['freeSurf'])


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES) + ['survey'])
def test_buoyancy_planes_are_the_difference_of_two_oracle_assemblies(name):
    """interior(C[1 / (b0 + db)]) - interior(C[1 / b0]) = L[db] with db positive and of the size of b0, so that the difference loses no digits.  Per component
    within (C_PLANES + 2) 2^-53 of the magnitudes of the three evaluations: each is the star evaluated once (C_PLANES, counted in density_cases) on a
    buoyancy that the oracle gets from 1 / rho of a rho = 1 / b (two more roundings); the magnitudes of b0 + db and b0 add up to that of 2 b0 + db."""
    if name == 'survey':
        sc = fc.config('fixed', False)
        sc.update(freq=fc.FREQS[2])
    else:
        sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    nz, nx = sc['nz'], sc['nx']
    db = dc.operator_inputs(sc)[0]
    b0 = (1.0 / np.asarray(sc['rho'], dtype=np.float64)).ravel()
    D = _oracle_planes(sc, (1.0 / (b0 + db)).reshape((nz, nx))) - _oracle_planes(sc, (1.0 / b0).reshape((nz, nx)))
    D[:, ~fr._interiorMask(nz, nx)] = 0
    L = fr.buoyancyPlanes(op, db)
    assert np.all(L[:, ~fr._interiorMask(nz, nx)] == 0)
    mag = fr.buoyancyPlanes(op, db, magnitude=True) + fr.buoyancyPlanes(op, 2 * b0 + db, magnitude=True)
    ratio = dc.worst_ratio(L.ravel(), D.ravel().astype(dc.CLD), ((dc.C_PLANES + 2) * dc.U64 * mag).ravel().astype(dc.LD))
    print('%s: worst error / bound %.3f; |L - D| / |D| %.2e' % (name, ratio, np.abs(L - D).max() / np.abs(D).max()))
    assert ratio <= 1.0
    # linear and homogeneous: the map of a sum is the sum of the maps, to rounding
    db2 = dc.operator_inputs(sc, seed=9)[0]
    assert np.abs(fr.buoyancyPlanes(op, db) + fr.buoyancyPlanes(op, db2) - fr.buoyancyPlanes(op, db + db2)).max() <= 16 * dc.U64 * mag.max()


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_buoyancy_adjoint_is_the_plain_transpose(name):
    "<L[db], P> = <db, L^T P> under the bilinear pairing for random complex P, to rounding; the same with the conjugated coefficients"
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    db, P, _ = dc.operator_inputs(sc)
    db = db * np.random.default_rng(2).uniform(-1., 1., db.size)
    L = fr.buoyancyPlanes(op, db).reshape((9, -1))
    for conj in (False, True):
        Lc = np.conj(L) if conj else L
        lhs, rhs = (Lc * P).sum(), (db * fr.buoyancyAdjoint(op, P, conj=conj)).sum()
        scale = (np.abs(L) * np.abs(P)).sum()
        assert abs(lhs - rhs) <= 64 * dc.U64 * scale, (name, conj, abs(lhs - rhs) / scale)
    # the lag products are the other half: sum_s z_s^T (dA) u_s = <L[db], P(z, u)>
    rng = np.random.default_rng(3)
    z, u = ac.randc(rng, (db.size, 3)), ac.randc(rng, (db.size, 3))
    a = (z * fr.applyPlanes(L, u, sc['nz'], sc['nx'])).sum()
    b = (L * fr.lagProducts(z, u, sc['nz'], sc['nx'])).sum()
    assert abs(a - b) <= 64 * dc.U64 * (np.abs(L) * fr.lagProducts(np.abs(z), np.abs(u), sc['nz'], sc['nx'])).sum()


# ---- 2. Taylor -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_taylor_remainder_of_dpred_in_rho_falls_at_second_order(solved, key):
    s = solved[key]
    r = dc.taylor_remainders(s['sv'], s['Jrho'], s['rho0'], s['v'])
    print('%s: remainders %s factors %s' % (key, r, fc.factors(r)))
    assert all(f >= 3.5 for f in fc.factors(r))


def test_taylor_test_rejects_the_mass_terms_alone(solved):
    'the derivative with the stiffness averages left out (K only) is of first order: the test above can fail'
    s = solved[('fixed', False)]
    prob, sv = s['prob'], s['sv']
    db = prob._buoyancyChain() * s['v']
    wrong = dc.born_with_planes(prob, sv, s['uF'], lambda op: dc.mass_only_planes(op, db))
    right = dc.born_with_planes(prob, sv, s['uF'], lambda op: fr.buoyancyPlanes(op, db))
    assert ac.rel(right, s['Jrho']) <= 1e-12
    r = dc.taylor_remainders(sv, wrong, s['rho0'], s['v'])
    print('mass terms alone: remainders %s factors %s' % (r, fc.factors(r)))
    assert all(f <= 2.5 for f in fc.factors(r))


# ---- 3. the adjoint identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_density_pair_is_adjoint_and_hvec_blocks_are_symmetric(solved, key):
    s = solved[key]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    rng = np.random.default_rng(17)
    x, y, r = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow), ac.randc(rng, sv.nD)
    Jx = prob.JvecBorn(None, x, u=uF, parameter='rho', **OP)
    g = prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter='rho', **OP)
    assert g.shape == (prob.nrow,) and g.dtype == np.float64 and Jx.dtype == np.complex128 and Jx.shape == (sv.nD,)
    lhs = ac.inner(Jx, r)
    miss = abs(lhs - ac.inner(x, g)) / abs(lhs)
    print('%s: identity misses by %.2e' % (key, miss))
    assert miss <= 1e-10
    H = lambda p, par: prob.Hvec(None, p, u=uF, parameter=par, **OP)
    a, b = float(x @ H(y, 'rho')), float(y @ H(x, 'rho'))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    assert abs(float(x @ H(x, 'rho')) - ac.inner(Jx, Jx)) <= 1e-10 * ac.inner(Jx, Jx)
    # the off-diagonal blocks are each other's transposes: p a c-perturbation, the result in rho, against q in rho, the result in c
    a, b = float(y @ H(x, ('c', 'rho'))), float(x @ H(y, ('rho', 'c')))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    assert abs(a - ac.inner(prob.JvecBorn(None, x, u=uF, **OP), prob.JvecBorn(None, y, u=uF, parameter='rho', **OP))) <= 1e-10 * abs(a)
    # u = None solves the fields itself and gives the same
    assert ac.rel(prob.JvecBorn(None, x, parameter='rho', **OP), Jx) <= 1e-12
    assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **OP), g) <= 1e-12


# ---- 4. the default and the refusals ---------------------------------------------------------------------------------------------------------------
def test_parameter_c_is_the_call_without_the_keyword_bit_for_bit(solved):
    s = solved[('relative', True)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    rng = np.random.default_rng(5)
    v, r = rng.standard_normal(prob.nrow), ac.randc(rng, sv.nD)
    for lin in ('scaler', 'operator'):
        kw = dict(u=uF, linearisation=lin)
        assert np.array_equal(prob.JvecBorn(None, v, parameter='c', **kw).view(np.float64), prob.JvecBorn(None, v, **kw).view(np.float64))
        assert np.array_equal(prob.Jtvec(None, r, adjoint='transpose', parameter='c', **kw), prob.Jtvec(None, r, adjoint='transpose', **kw))
        assert np.array_equal(prob.Hvec(None, v, parameter='c', **kw), prob.Hvec(None, v, **kw))
        assert np.array_equal(prob.Hvec(None, v, parameter=('c', 'c'), **kw), prob.Hvec(None, v, **kw))
    assert np.array_equal(prob.Jtvec(None, r, u=uF, parameter='c'), prob.Jtvec(None, r, u=uF))


def test_bad_parameters_are_refused(solved):
    s = solved[('fixed', False)]
    prob, sv, uF, v = s['prob'], s['sv'], s['uF'], s['v']
    r = ac.randc(np.random.default_rng(3), sv.nD)
    calls = [lambda: prob.JvecBorn(None, v, u=uF, parameter='rho'),                                      # (linearisation='scaler': the reference has no density scaler)
             lambda: prob.JvecBorn(None, v, u=uF, linearisation='scaler', parameter='rho'),
             lambda: prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter='rho'),
             lambda: prob.Jtvec(None, r, u=uF, parameter='rho', **OP),                                   # (adjoint='reciprocity')
             lambda: prob.Hvec(None, v, u=uF, parameter='rho'),
             lambda: prob.Hvec(None, v, u=uF, parameter=('c', 'rho')),
             lambda: prob.JvecBorn(None, v, u=uF, parameter='density', **OP),
             lambda: prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter=None, **OP),
             lambda: prob.Hvec(None, v, u=uF, parameter=('rho', 'Q'), **OP)]
    for call in calls:
        with pytest.raises(ValueError):
            call()


def _all_three_refuse(prob, sv):
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for call in (lambda: prob.JvecBorn(None, v, parameter='rho', **OP), lambda: prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **OP),
                 lambda: prob.Hvec(None, v, parameter='rho', **OP), lambda: prob.Hvec(None, v, parameter=('c', 'rho'), **OP)):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert len(str(ei.value)) > 20


def test_what_the_density_derivative_does_not_serve_is_refused_with_the_reason():
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    sc = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True)
    del sc['rho']
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    _all_three_refuse(prob, sv)
    with pytest.raises(NotImplementedError, match='rho'):
        prob.JvecBorn(None, np.ones(prob.nrow), parameter='rho', **OP)
    prob25, sv25 = ac.host_pair('25d-fixed', rho=2000.)
    _all_three_refuse(prob25, sv25)
    scv = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True, Q=50.)
    probv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    probv.pair(svv)
    _all_three_refuse(probv, svv)
    sce = fc.config('fixed', False, Disc=za.Eurus, hostGradient=True)
    probe, sve = Helm2DProblem(sce), Helm2DSurvey(sce)
    probe.pair(sve)
    _all_three_refuse(probe, sve)
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq, rho=2000.)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    _all_three_refuse(probm, svm)


# ---- 5. the reference evaluations of the four kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(3, 3, 1), (5, 61, 5), (4, 63, 4), (33, 64, 3)])
def test_the_80_bit_evaluations_bound_plain_fp64_and_reject_wrong_ones(case):
    nz, nx, nsrc = case
    U, B, C, P0 = dc.kernel_inputs(nz, nx, nsrc, seed=nz)
    coef = 0.3 - 1.1j
    shifted = list(dc.LAGS)
    shifted[5], shifted[3] = shifted[3], shifted[5]                   # (one pair of lags mis-shifted: left for right)
    for conj in (False, True):
        ref, mag = dc.stencil_sources_reference(U, C, coef, nz, nx, conj)
        bound = dc.C_STENCIL * dc.U64 * mag
        X = np.conj(U) if conj else U
        plain = np.stack([coef * fr.applyPlanes(C.reshape((9, nz, nx)), X[s], nz, nx) for s in range(nsrc)])         # the host route's own fp64 numpy
        assert dc.worst_ratio(plain, ref, bound) <= 1.0
        assert dc.worst_ratio(dc.stencil_sources_reference(U, C, coef, nz, nx, conj, dtype=np.complex128)[0], ref, bound) <= 1.0
        if nx > 3:
            assert dc.worst_ratio(dc.stencil_sources_reference(U, C, coef, nz, nx, conj, dtype=np.complex128, lags=shifted)[0], ref, bound) > 1e6
    ref, mag = dc.lag_imaging_reference(P0, U, B, nz, nx)
    bound = dc.c_lag(nsrc) * dc.U64 * mag
    plain = P0 + fr.lagProducts(B.T, U.T, nz, nx)
    assert dc.worst_ratio(plain, ref, bound) <= 1.0
    assert dc.worst_ratio(dc.lag_imaging_reference(P0, U, B, nz, nx, dtype=np.complex128)[0], ref, bound) <= 1.0
    assert dc.worst_ratio(dc.lag_imaging_reference(P0, U, B, nz, nx, dtype=np.complex128, mask=False)[0], ref, bound) > 1e6
    if nx > 3:
        assert dc.worst_ratio(dc.lag_imaging_reference(P0, U, B, nz, nx, dtype=np.complex128, lags=shifted)[0], ref, bound) > 1e6


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_the_80_bit_buoyancy_map_and_transpose_bound_plain_fp64_and_reject_wrong_ones(name):
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    db, P, G0 = dc.operator_inputs(sc)
    N = db.size
    ref, mag = dc.planes_reference(op, db)
    bound = dc.C_PLANES * dc.U64 * mag
    plain = fr.buoyancyPlanes(op, db).reshape((9, N))
    ratio = dc.worst_ratio(plain, ref, bound)
    assert ratio <= 1.0
    assert dc.worst_ratio(plain[::-1], ref, bound) > 1e6                        # (the planes in the wrong slots)
    w = -0.7 + 0.4j
    worst = [ratio]
    for conj in (False, True):
        ref, mag = dc.adjoint_reference(op, G0, P, w, conj)
        bound = dc.C_ADJOINT * dc.U64 * mag
        worst.append(dc.worst_ratio(G0 + w * fr.buoyancyAdjoint(op, P, conj=conj), ref, bound))
        assert worst[-1] <= 1.0
        assert dc.worst_ratio(G0 + w * fr.buoyancyAdjoint(op, P, conj=not conj), ref, bound) > 1e6
    print('%s: fp64 numpy at %s of the bounds' % (name, ['%.3f' % x for x in worst]))
