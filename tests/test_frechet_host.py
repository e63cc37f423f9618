"""CPU: linearisation='operator' of JvecBorn / Jtvec / Hvec on the oracle doubles -- the Taylor test that makes it the derivative of dpred (and shows that
the default 'scaler' is not), Richardson checks of Jv and of g . v, the adjoint identity, the refusals, and the 80-bit evaluation the device kernels are
held to, checked against plain fp64 numpy and against two wrong stencils."""
import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
from zephyr_amd.frechet import MZ_MASS, massStencil, maskInterior

CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-mz', 'fixed-hd', 'moving-mz', 'moving-hd']


@pytest.fixture(scope='module')
def solved():
    'per case: the pair, the model, the perturbation, the host fields at the model and both Born data -- made once, left unchanged'
    out = {}
    for key in CASES:
        prob, sv = fc.host_pair(*key)
        c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
        v = fc.perturbation()
        uF = prob.fields(c0)
        out[key] = dict(prob=prob, sv=sv, c0=c0, v=v, uF=uF, Jop=prob.JvecBorn(None, v, u=uF, linearisation='operator'),
                        Jsc=prob.JvecBorn(None, v, u=uF, linearisation='scaler'))
    return out


def _dpred(s):
    return lambda c: s['sv'].dpred(c)


# ---- 1. Taylor ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_taylor_remainder_of_dpred_falls_at_second_order_with_operator_and_at_first_with_scaler(solved, key):
    s = solved[key]
    r_op = fc.taylor_remainders(_dpred(s), s['Jop'], s['c0'], s['v'])
    r_sc = fc.taylor_remainders(_dpred(s), s['Jsc'], s['c0'], s['v'])
    s['prob'].updateModel(s['c0'])
    print('%s: operator remainders %s factors %s; scaler factors %s' % (key, r_op, fc.factors(r_op), fc.factors(r_sc)))
    assert all(f >= 3.5 for f in fc.factors(r_op))
    assert all(f <= 2.5 for f in fc.factors(r_sc))


# ---- 2. Richardson -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', [('fixed', False), ('relative', True)], ids=['fixed-mz', 'moving-hd'])
def test_central_differences_of_dpred_and_of_the_misfit_converge_to_jvec_and_to_the_gradient(solved, key):
    s = solved[key]
    prob, sv, c0, v = s['prob'], s['sv'], s['c0'], s['v']
    rng = np.random.default_rng(41)
    d0 = sv.dpred(c0)
    dobs = d0 + 0.3 * fc.norm(d0) / np.sqrt(d0.size) * ac.randc(rng, d0.size)
    misfit = lambda c: 0.5 * fc.norm(sv.dpred(c) - dobs) ** 2
    ej, eg = [], []
    prob.updateModel(c0)
    g = prob.Jtvec(None, d0 - dobs, u=s['uF'], adjoint='transpose', linearisation='operator')
    gv = float(g @ v)
    for h in (0.25, 0.125):
        ej.append(fc.norm(s['Jop'] - fc.central(_dpred(s), c0, v, h)))
        eg.append(abs(gv - fc.central(misfit, c0, v, h)))
    prob.updateModel(c0)
    print('%s: |Jv - central| %s (|Jv| %.3e); |g.v - central| %s (|g.v| %.3e)' % (key, ej, fc.norm(s['Jop']), eg, abs(gv)))
    assert ej[0] / ej[1] >= 3.5
    assert eg[0] / eg[1] >= 3.5


# ---- 3. the adjoint identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_operator_pair_is_adjoint(solved, key):
    s = solved[key]
    prob, sv = s['prob'], s['sv']
    rng = np.random.default_rng(17)
    x, r = rng.standard_normal(prob.nrow), ac.randc(rng, sv.nD)
    Jx = prob.JvecBorn(None, x, u=s['uF'], linearisation='operator')
    g = prob.Jtvec(None, r, u=s['uF'], adjoint='transpose', linearisation='operator')
    assert g.shape == (prob.nrow,) and g.dtype == np.float64 and Jx.dtype == np.complex128
    lhs = ac.inner(Jx, r)
    miss = abs(lhs - ac.inner(x, g)) / abs(lhs)
    print('%s: identity misses by %.2e' % (key, miss))
    assert miss <= 1e-10
    # Hvec is the composition, symmetric
    y = rng.standard_normal(prob.nrow)
    a, b = float(x @ prob.Hvec(None, y, u=s['uF'], linearisation='operator')), float(y @ prob.Hvec(None, x, u=s['uF'], linearisation='operator'))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    assert abs(float(x @ prob.Hvec(None, x, u=s['uF'], linearisation='operator')) - ac.inner(Jx, Jx)) <= 1e-10 * ac.inner(Jx, Jx)
    # u = None solves the fields itself and gives the same
    assert ac.rel(prob.JvecBorn(None, x, linearisation='operator'), Jx) <= 1e-12
    assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', linearisation='operator'), g) <= 1e-12


# ---- 4. refusals and the untouched default -------------------------------------------------------------------------------------------------------
def test_scaler_is_the_default_bit_for_bit_and_bad_values_are_refused(solved):
    s = solved[('fixed', False)]
    prob, sv, uF, v = s['prob'], s['sv'], s['uF'], s['v']
    r = ac.randc(np.random.default_rng(3), sv.nD)
    assert np.array_equal(prob.JvecBorn(None, v, u=uF).view(np.float64), s['Jsc'].view(np.float64))
    assert np.array_equal(prob.Jtvec(None, r, u=uF, adjoint='transpose', linearisation='scaler'), prob.Jtvec(None, r, u=uF, adjoint='transpose'))
    assert np.array_equal(prob.Jtvec(None, r, u=uF, linearisation='scaler'), prob.Jtvec(None, r, u=uF))
    assert np.array_equal(prob.Hvec(None, v, u=uF, linearisation='scaler'), prob.Hvec(None, v, u=uF))
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=uF, linearisation='operator')                           # (adjoint='reciprocity')
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=uF, adjoint='reciprocity', linearisation='operator')
    for call in (lambda: prob.JvecBorn(None, v, u=uF, linearisation='exact'), lambda: prob.Hvec(None, v, u=uF, linearisation=None),
                 lambda: prob.Jtvec(None, r, u=uF, adjoint='transpose', linearisation='Operator')):
        with pytest.raises(ValueError):
            call()


def _all_three_refuse(prob, sv):
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for call in (lambda: prob.JvecBorn(None, v, linearisation='operator'), lambda: prob.Jtvec(None, r, adjoint='transpose', linearisation='operator'),
                 lambda: prob.Hvec(None, v, linearisation='operator')):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert len(str(ei.value)) > 20


def test_what_the_operator_linearisation_does_not_serve_is_refused_with_the_reason():
    import zephyr_amd as za
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    # no rho in the config
    sc = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True)
    del sc['rho']
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    _all_three_refuse(prob, sv)
    with pytest.raises(NotImplementedError, match='rho'):
        prob.JvecBorn(None, np.ones(prob.nrow), linearisation='operator')
    # the 2.5-D composite
    prob25, sv25 = ac.host_pair('25d-fixed', rho=2000.)
    _all_three_refuse(prob25, sv25)
    # visco
    scv = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True, Q=50.)
    probv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    probv.pair(svv)
    _all_three_refuse(probv, svv)
    # Eurus
    sce = fc.config('fixed', False, Disc=za.Eurus, hostGradient=True)
    probe, sve = Helm2DProblem(sce), Helm2DSurvey(sce)
    probe.pair(sve)
    _all_three_refuse(probe, sve)
    # multiscale
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq, rho=2000.)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    _all_three_refuse(probm, svm)


# ---- 5. the reference evaluation of the two kernels ----------------------------------------------------------------------------------------------
SHAPES = [(12, 9), (3, 70), (5, 300), (37, 53)]


@pytest.mark.parametrize('shape', SHAPES)
def test_the_80_bit_evaluation_bounds_plain_fp64_and_rejects_wrong_stencils(shape):
    nz, nx = shape
    nsrc = 3
    U, B, W, G0 = fc.kernel_inputs(nz, nx, nsrc, seed=nz)
    coef = 0.3 - 1.1j
    swapped = (MZ_MASS[1], MZ_MASS[0], MZ_MASS[2])
    for conj in (False, True):
        ref, mag = fc.virtual_sources_reference(U, W, coef, nz, nx, conj)
        bound = fc.C_VIRTUAL * fc.U64 * mag
        X = np.conj(U) if conj else U
        plain = np.stack([coef * massStencil(W * X[s], nz, nx, mask=True) for s in range(nsrc)])        # the host route's own fp64 numpy
        assert fc.worst_ratio(plain, ref, bound) <= 1.0
        assert fc.worst_ratio(fc.virtual_sources_reference(U, W, coef, nz, nx, conj, dtype=np.complex128)[0], ref, bound) <= 1.0
        assert fc.worst_ratio(fc.virtual_sources_reference(U, W, coef, nz, nx, conj, weights=swapped, dtype=np.complex128)[0], ref, bound) > 1e6
        assert fc.worst_ratio(fc.virtual_sources_reference(U, W, coef, nz, nx, conj, mask=False, dtype=np.complex128)[0], ref, bound) > 1e6
    ref, mag = fc.imaging_reference(G0, U, B, W, nz, nx)
    bound = fc.c_imaging(nsrc) * fc.U64 * mag
    plain = G0 + W * sum(U[s] * massStencil(maskInterior(B[s], nz, nx), nz, nx) for s in range(nsrc))
    assert fc.worst_ratio(plain, ref, bound) <= 1.0
    assert fc.worst_ratio(fc.imaging_reference(G0, U, B, W, nz, nx, dtype=np.complex128)[0], ref, bound) <= 1.0
    assert fc.worst_ratio(fc.imaging_reference(G0, U, B, W, nz, nx, weights=swapped, dtype=np.complex128)[0], ref, bound) > 1e6
    assert fc.worst_ratio(fc.imaging_reference(G0, U, B, W, nz, nx, mask=False, dtype=np.complex128)[0], ref, bound) > 1e6
