"""CPU: the full Newton Hessian-vector product, Hvec(resid=), on the oracle doubles -- the second derivative of the planes by a Taylor test that the mass term alone
fails, the product against central differences of the exact gradient (which the Gauss-Newton product fails), the zero residual, the symmetry, the 80-bit
evaluations the two device kernels are held to, and the refusals."""
import numpy as np
import pytest

import zephyr_amd as za
from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import newton_cases as nc
from zephyr_amd import frechet as fr

CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-mz', 'fixed-hd', 'moving-mz', 'moving-hd']
FULL = dict(linearisation='full')
OP = dict(linearisation='operator')


@pytest.fixture(scope='module')
def solved():
    'per case: the pair, the model, dobs of the shifted model, the host fields and the residual at the model -- made once'
    out = {}
    for key in CASES:
        prob, sv = nc.pair(*key)
        c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
        dobs = nc.observed(prob, sv, c0)
        uF = prob.fields()
        out[key] = dict(prob=prob, sv=sv, c0=c0, dobs=dobs, uF=uF, r=sv.dpred(None, u=uF) - dobs)
    return out


def _restore(s):
    s['prob'].updateModel({'c': np.array(s['c0']), 'rho': np.array(fc.model()[1])})


# ---- 1. the second derivative of the planes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_second_derivative_of_the_planes_by_central_differences_and_the_mass_term_alone_fails(name):
    """||(V_(c+hp)[p] - V_(c-hp)[p]) / 2h - d2A[p, p]||_inf with V = frechet.velocityPlanes and p non-zero in every cell: second order with velocityPlanes2 (from
    rowFactorsD2c and d2 kappa / dc2), no convergence with its stretch part left out -- every one of these grids has cells in the absorbing layers"""
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    p = nc.curvature_inputs(sc)[0]
    c0 = np.asarray(sc['c'], dtype=np.float64)
    V = lambda c: fr.velocityPlanes(za.MiniZephyr(dict(sc, c=c)), p)
    cand = {'full': fr.velocityPlanes2(op, p), 'mass': fr.velocityPlanes2(op, p, stretch=False)}
    rem = {k: [] for k in cand}
    for h in fc.TAYLOR_H:
        D = fc.central(V, c0, p, h)
        for k, d2 in cand.items():
            rem[k].append(float(np.abs(D - d2).max()))
    print('%s: %s' % (name, {k: ['%.2f' % f for f in fc.factors(r)] for k, r in rem.items()}))
    assert all(f >= nc.SECOND for f in fc.factors(rem['full']))
    assert all(f <= nc.STALL for f in fc.factors(rem['mass']))
    # symmetric and bilinear in the two directions
    q = np.random.default_rng(3).standard_normal(p.size)
    assert np.array_equal(fr.velocityPlanes2(op, p, q), fr.velocityPlanes2(op, q, p))


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_curvature_contracts_the_second_derivative_and_the_transposed_planes_are_the_transpose(name):
    "<d2A[p, q], P> = <q, velocityCurvature(P, p)> and <C^T v, u> = <v, C u> under the bilinear pairing, to rounding; conjugated and without the stretch too"
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    nz, nx = sc['nz'], sc['nx']
    p, P, _ = nc.curvature_inputs(sc)
    rng = np.random.default_rng(2)
    q = rng.standard_normal(p.size)
    for conj in (False, True):
        for stretch in (True, False):
            D = fr.velocityPlanes2(op, p, q, stretch=stretch).reshape((9, -1))
            Dc = np.conj(D) if conj else D
            lhs, rhs = (Dc * P).sum(), (q * fr.velocityCurvature(op, P, p, conj=conj, stretch=stretch)).sum()
            assert abs(lhs - rhs) <= 64 * dc.U64 * (np.abs(D) * np.abs(P)).sum(), (name, conj, stretch)
    C = fr.velocityPlanes(op, p)
    u, v = ac.randc(rng, (p.size, 3)), ac.randc(rng, (p.size, 3))
    lhs, rhs = (fr.applyPlanesTransposed(C, v) * u).sum(), (v * fr.applyPlanes(C, u, nz, nx)).sum()
    assert abs(lhs - rhs) <= 64 * dc.U64 * (np.abs(v) * fr.applyPlanes(np.abs(C), np.abs(u), nz, nx)).sum()
    assert np.array_equal(fr.applyPlanesTransposed(C.reshape((9, -1)), v, nz, nx), fr.applyPlanesTransposed(C, v))


# ---- 2. the Hessian against the gradient ------------------------------------------------------------------------------------------------------------
# (case, linearisation, parameter): 'full' with p in every cell on all four cases; 'operator' with p zero in the layers, compared outside them, and the density on
# two cases each, which between them have both arrays and both classes
TAYLOR = [(k, 'full', 'c') for k in CASES] + [(CASES[0], 'operator', 'c'), (CASES[3], 'operator', 'c'), (CASES[1], 'operator', 'rho'), (CASES[2], 'full', 'rho')]


@pytest.mark.parametrize('key,lin,par', TAYLOR, ids=['%s-%s-%s' % (IDS[CASES.index(k)], l, p) for k, l, p in TAYLOR])
def test_central_differences_of_the_gradient_converge_to_hvec_with_resid_and_not_to_gauss_newton(solved, key, lin, par):
    """||(g(m + h p) - g(m - h p)) / 2h - H p|| over fc.TAYLOR_H falls at second order with H p = Hvec(resid=r), g the exact gradient at fixed dobs; against the
    Gauss-Newton product the same remainder keeps its size.  dobs is the data of the model shifted by 40 m/s: measured ||H p - J^T J p|| / ||H p|| = 0.72 for
    ('fixed', MiniZephyr, 'full', 'c') and between 0.4 and 0.9 on the other cases (printed)."""
    s = solved[key]
    prob, sv = s['prob'], s['sv']
    kw = dict(linearisation=lin, parameter=par)
    layers = lin == 'operator' and par == 'c'
    p = nc.outside_layers() if layers else (dc.perturbation() if par == 'rho' else nc.everywhere())
    keep = (p != 0) if layers else None
    _restore(s)
    Hp = prob.Hvec(None, p, u=s['uF'], resid=s['r'], **kw)
    Hgn = prob.Hvec(None, p, u=s['uF'], **kw)
    assert Hp.shape == (prob.nrow,) and Hp.dtype == np.float64
    m0 = fc.model()[1] if par == 'rho' else s['c0']
    g = nc.gradient_of(prob, sv, s['dobs'], **kw)
    try:
        rn = nc.central_remainders(g, m0, p, Hp, keep)
        rg = [fc.norm((fc.central(g, m0, p, h) - Hgn)[slice(None) if keep is None else keep]) for h in fc.TAYLOR_H[-2:]]
    finally:
        _restore(s)
    sl = slice(None) if keep is None else keep
    ratio = fc.norm((Hp - Hgn)[sl]) / fc.norm(Hp[sl])
    print('%s %s %s: remainders %s factors %s; ||Hp - JtJp|| / ||Hp|| = %.3f, Gauss-Newton remainders %s' % (key, lin, par, rn, fc.factors(rn), ratio, rg))
    assert all(f >= nc.SECOND for f in fc.factors(rn))
    assert ratio >= 0.1
    assert rg[0] / rg[1] <= nc.STALL and rg[1] >= 0.5 * fc.norm((Hp - Hgn)[sl])          # (it stalls at the part it leaves out)


# ---- 3. the zero residual -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('par', ['c', 'rho'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_zero_residual_gives_the_gauss_newton_product(solved, key, par):
    "1e-12 is the bound of test_full_host.py between two host routes of one product (u given against u = None)"
    s = solved[key]
    prob, sv = s['prob'], s['sv']
    p = np.random.default_rng(5).standard_normal(prob.nrow)
    for lin in ('full', 'operator'):
        kw = dict(u=s['uF'], linearisation=lin, parameter=par)
        assert ac.rel(prob.Hvec(None, p, resid=np.zeros(sv.nD), **kw), prob.Hvec(None, p, **kw)) <= 1e-12
    # resid=None is the call as it was; u = None solves the fields itself and gives the same
    kw = dict(linearisation='full', parameter=par)
    assert np.array_equal(prob.Hvec(None, p, u=s['uF'], resid=None, **kw), prob.Hvec(None, p, u=s['uF'], **kw))
    assert ac.rel(prob.Hvec(None, p, resid=s['r'], **kw), prob.Hvec(None, p, u=s['uF'], resid=s['r'], **kw)) <= 1e-12


# ---- 4. symmetry -----------------------------------------------------------------------------------------------------------------------------------------
def symmetry_defects(prob, uF, r, seed=17, **kw):
    '(|<q, H p> - <p, H q>| / max of the two) of the Newton product and of the Gauss-Newton product on the same random p, q'
    rng = np.random.default_rng(seed)
    p, q = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow)
    out = []
    for extra in (dict(resid=r), dict()):
        a, b = float(q @ prob.Hvec(None, p, u=uF, **kw, **extra)), float(p @ prob.Hvec(None, q, u=uF, **kw, **extra))
        out.append(abs(a - b) / max(abs(a), abs(b)))
    return out


@pytest.mark.parametrize('par', ['c', 'rho'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_newton_product_is_symmetric_to_ten_times_the_defect_of_gauss_newton(solved, key, par):
    "the two extra solves and the cancellation between the terms are allowed one decimal over what the Gauss-Newton product shows on the same inputs"
    s = solved[key]
    newton, gn = symmetry_defects(s['prob'], s['uF'], s['r'], linearisation='full', parameter=par)
    print('%s %s: symmetry defect %.2e, of the Gauss-Newton product %.2e' % (key, par, newton, gn))
    assert newton <= 10 * gn


# ---- 5. the reference evaluations of the two kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_the_80_bit_curvature_bounds_plain_fp64_and_rejects_wrong_ones(name):
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    p, P, G0 = nc.curvature_inputs(sc)
    w = -0.7 + 0.4j
    worst = []
    for conj in (False, True):
        for stretch in (True, False):
            ref, mag = nc.curvature_reference(op, G0, P, p, w, conj, stretch)
            bound = nc.C_CURVATURE * nc.U64 * mag
            worst.append(nc.worst_ratio(G0 + w * fr.velocityCurvature(op, P, p, conj=conj, stretch=stretch), ref, bound))
            assert worst[-1] <= 1.0
            if stretch:          # (the mass term alone has the real coefficient 6 omega^2 b / c^4 at a real frequency: nothing to conjugate)
                assert nc.worst_ratio(G0 + w * fr.velocityCurvature(op, P, p, conj=not conj, stretch=stretch), ref, bound) > 1e6
            assert nc.worst_ratio(G0 + w * fr.velocityCurvature(op, P, p, conj=conj, stretch=not stretch), ref, bound) > 1e6      # (a missing term)
    print('%s: fp64 numpy at %s of the bound' % (name, ['%.3f' % x for x in worst]))


@pytest.mark.parametrize('case', nc.KERNEL_CASES[::3], ids=['%dx%dx%d' % c for c in nc.KERNEL_CASES[::3]])
def test_the_80_bit_transposed_stencil_bounds_plain_fp64_and_rejects_a_missing_term(case):
    nz, nx, nsrc = case
    U, _, C, _ = nc.kernel_inputs(nz, nx, nsrc, seed=100 * nz + nx + nsrc)
    coef = 0.3 - 1.1j
    for conj in (False, True):
        ref, mag = nc.stencil_t_reference(U, C, coef, nz, nx, conj)
        bound = nc.C_STENCIL_T * nc.U64 * mag
        plain = nc.stencil_t_reference(U, C, coef, nz, nx, conj, dtype=np.complex128)[0]
        assert nc.worst_ratio(plain, ref, bound) <= 1.0
        assert nc.worst_ratio(nc.stencil_t_without_a_lag(U, C, coef, nz, nx, conj), ref, bound) > 1e6
        assert nc.worst_ratio(nc.stencil_t_reference(U, C, coef, nz, nx, not conj, dtype=np.complex128)[0], ref, bound) > 1e6
        # not the untransposed stencil
        assert nc.worst_ratio(dc.stencil_sources_reference(U, np.conj(C) if conj else C, coef, nz, nx, False, dtype=np.complex128)[0], ref, bound) > 1e6


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_what_hvec_with_resid_does_not_serve_is_refused(solved):
    s = solved[('fixed', False)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    p, r = np.ones(prob.nrow), s['r']
    with pytest.raises(ValueError, match='no Hessian'):
        prob.Hvec(None, p, u=uF, resid=r)                                        # ('scaler')
    with pytest.raises(ValueError, match='weights'):
        prob.Hvec(None, p, u=uF, resid=r, weights=np.ones(sv.nD), **FULL)
    with pytest.raises(ValueError, match='size of the data'):
        prob.Hvec(None, p, u=uF, resid=r[:-1], **FULL)
    for pair in (('c', 'rho'), ('rho', 'c')):
        with pytest.raises(NotImplementedError, match='not local'):
            prob.Hvec(None, p, u=uF, resid=r, parameter=pair, **FULL)
    with pytest.raises(ValueError):
        prob.Hvec(None, p, u=uF, resid=r, parameter='Q', **FULL)
    # without `rho` the density follows c: 'full' says why it has no second derivative here, 'operator' refuses the config as it always did
    probg, svg = nc.pair('fixed', False, density=False)
    with pytest.raises(NotImplementedError, match='not local'):
        probg.Hvec(None, p, resid=r, **FULL)
    with pytest.raises(NotImplementedError) as ei:
        probg.Hvec(None, p, resid=r, **OP)
    with pytest.raises(NotImplementedError) as ej:
        probg.Hvec(None, p, **OP)
    assert str(ei.value) == str(ej.value)


def test_the_other_operators_are_refused_with_the_sentences_they_carry():
    "the 2.5-D composite, visco, Eurus and multiscale: Hvec(resid=) refuses with the sentence Hvec() refuses with, which is JvecBorn's under the name of the caller"
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    prob25, sv25 = ac.host_pair('25d-fixed', rho=2000.)
    scv = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True, Q=50.)
    probv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    probv.pair(svv)
    sce = fc.config('fixed', False, Disc=za.Eurus, hostGradient=True)
    probe, sve = Helm2DProblem(sce), Helm2DSurvey(sce)
    probe.pair(sve)
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq, rho=2000.)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    # the same operators without `rho` in the config: still the sentence of the operator, not the one about the density
    norho = []
    for Problem, extra in ((Helm2DViscoProblem, dict(Disc=ac.OracleMiniZephyrT, Q=50.)), (Helm2DProblem, dict(Disc=za.Eurus))):
        sc = fc.config('fixed', False, hostGradient=True, **extra)
        del sc['rho']
        probn, svn = Problem(sc), Helm2DSurvey(sc)
        probn.pair(svn)
        norho.append((probn, svn))
    for prob, sv in [(prob25, sv25), (probv, svv), (probe, sve), (probm, svm)] + norho:
        v, r = np.ones(prob.nrow), np.ones(sv.nD, dtype=complex)
        for kw in (FULL, OP):
            said = []
            for call in (lambda: prob.Hvec(None, v, resid=r, **kw), lambda: prob.Hvec(None, v, **kw), lambda: prob.JvecBorn(None, v, **kw)):
                with pytest.raises(NotImplementedError) as ei:
                    call()
                said.append(str(ei.value))
            assert said[0] == said[1] and said[0].replace('Hvec', 'JvecBorn') == said[2]
