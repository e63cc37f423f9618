"""CPU: the stacked (c, rho) routes, parameter='joint', on the oracle doubles -- the mixed second derivative of the planes by a Taylor test that the mass term alone
fails, its two transposes, the joint gradient, Born data and Hessian products against the single-parameter calls they replace, the joint Newton product against
central differences of the joint gradient (which the Gauss-Newton product and the product without the mixed terms fail), the symmetry, the 80-bit evaluations the two
device kernels are held to, and the refusals."""
import numpy as np
import pytest

import zephyr_amd as za
from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import joint_cases as jc
from tests import newton_cases as nc
from zephyr_amd import frechet as fr
from zephyr_amd import problem as problem_module

CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-mz', 'fixed-hd', 'moving-mz', 'moving-hd']
FULL = dict(linearisation='full', parameter='joint')
OP = dict(linearisation='operator', parameter='joint')


@pytest.fixture(scope='module')
def solved():
    'per case: the pair, dobs of the shifted model, the host fields and the residual at the model -- made once'
    out = {}
    for key in CASES:
        prob, sv = jc.pair(*key)
        dobs = jc.observed(prob, sv)
        uF = prob.fields()
        out[key] = dict(prob=prob, sv=sv, dobs=dobs, uF=uF, r=sv.dpred(None, u=uF) - dobs, N=prob.nrow)
    return out


# ---- 1. the mixed derivative of the planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_mixed_derivative_of_the_planes_by_central_differences_and_the_mass_term_alone_fails(name):
    """||(L_(c+hp)[beta] - L_(c-hp)[beta]) / 2h - mixedPlanes(p, beta)||_inf with L = frechet.buoyancyPlanes, p non-zero in every cell and beta of mixed sign: second
    order with the stretch part, no convergence without it -- every one of these grids has cells in the absorbing layers; linear in beta to 1e-13"""
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    p = nc.curvature_inputs(sc)[0]
    rng = np.random.default_rng(4)
    beta, gamma = rng.standard_normal(p.size) / 2000., rng.standard_normal(p.size) / 2000.
    assert beta.min() < 0 < beta.max()
    c0 = np.asarray(sc['c'], dtype=np.float64)
    L = lambda c: fr.buoyancyPlanes(za.MiniZephyr(dict(sc, c=c)), beta)
    cand = {'full': fr.mixedPlanes(op, p, beta), 'mass': fr.mixedPlanes(op, p, beta, stretch=False)}
    rem = {k: [] for k in cand}
    for h in fc.TAYLOR_H:
        D = fc.central(L, c0, p, h)
        for k, M in cand.items():
            rem[k].append(float(np.abs(D - M).max()))
    print('%s: %s' % (name, {k: ['%.3f' % f for f in fc.factors(r)] for k, r in rem.items()}))
    assert all(f >= jc.SECOND for f in fc.factors(rem['full']))
    assert all(f <= jc.STALL for f in fc.factors(rem['mass']))
    for stretch in (True, False):
        lhs = fr.mixedPlanes(op, p, 0.3 * beta - 1.7 * gamma, stretch=stretch)
        rhs = 0.3 * fr.mixedPlanes(op, p, beta, stretch=stretch) - 1.7 * fr.mixedPlanes(op, p, gamma, stretch=stretch)
        assert np.abs(lhs - rhs).max() <= 1e-13 * np.abs(rhs).max()
    # V at the buoyancy b + beta minus V at b: the mixed derivative is velocityPlanes with beta in the place of the buoyancy
    shifted = za.MiniZephyr(dict(sc, rho=1. / (1. / np.asarray(sc['rho'], dtype=np.float64) + beta.reshape(np.shape(sc['rho'])))))
    diff = fr.velocityPlanes(shifted, p) - fr.velocityPlanes(op, p)
    assert np.abs(diff - cand['full']).max() <= 1e-12 * np.abs(fr.velocityPlanes(op, p)).max()


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_the_two_transposes_of_the_mixed_planes(name):
    "<mixedPlanes(p, beta), P> = <p, mixedAdjointC(P, beta)> = <beta, mixedAdjointB(P, p)> under the bilinear pairing, to rounding; conjugated and without the stretch too"
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    p, B, P, _ = jc.mixed_inputs(sc)
    for conj in (False, True):
        for stretch in (True, False):
            D = fr.mixedPlanes(op, p, B, stretch=stretch).reshape((9, -1))
            Dc = np.conj(D) if conj else D
            lhs = (Dc * P).sum()
            in_c = (p * fr.mixedAdjointC(op, P, B, conj=conj, stretch=stretch)).sum()
            in_b = (B * fr.mixedAdjointB(op, P, p, conj=conj, stretch=stretch)).sum()
            tol = 64 * dc.U64 * (fr.mixedPlanes(op, p, B, stretch=stretch, magnitude=True).reshape((9, -1)) * np.abs(P)).sum()
            assert abs(lhs - in_c) <= tol and abs(lhs - in_b) <= tol, (name, conj, stretch)
            assert abs(lhs) > 1e3 * tol


# ---- 2. one route of a product against another ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_joint_routes_against_the_single_parameter_calls(solved, key):
    "1e-12 is the project's bound between two host routes of one product (test_full_host.py, test_newton_host.py)"
    s = solved[key]
    prob, sv, uF, r, N = s['prob'], s['sv'], s['uF'], s['r'], s['N']
    vc, vr = jc.directions()
    v, z = jc.stack(vc, vr), np.zeros(N)
    for lin in ('full', 'operator'):
        one = dict(u=uF, linearisation=lin)
        kw = dict(one, parameter='joint')
        g = prob.Jtvec(None, r, adjoint='transpose', **kw)
        assert g.shape == (2 * N,) and g.dtype == np.float64
        assert ac.rel(g[:N], prob.Jtvec(None, r, adjoint='transpose', parameter='c', **one)) <= 1e-12
        assert ac.rel(g[N:], prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **one)) <= 1e-12
        d = prob.JvecBorn(None, v, **kw)
        assert d.shape == (sv.nD,)
        assert ac.rel(d, prob.JvecBorn(None, vc, parameter='c', **one) + prob.JvecBorn(None, vr, parameter='rho', **one)) <= 1e-12
        H = prob.Hvec(None, v, **kw)
        blocks = np.concatenate((prob.Hvec(None, vc, parameter='c', **one) + prob.Hvec(None, vr, parameter=('rho', 'c'), **one),
                                 prob.Hvec(None, vc, parameter=('c', 'rho'), **one) + prob.Hvec(None, vr, parameter='rho', **one)))
        assert H.shape == (2 * N,) and H.dtype == np.float64
        assert ac.rel(H, blocks) <= 1e-12
        Hn = prob.Hvec(None, v, resid=r, **kw)
        assert Hn.shape == (2 * N,) and Hn.dtype == np.float64
        assert ac.rel(prob.Hvec(None, jc.stack(vc, z), resid=r, **kw)[:N], prob.Hvec(None, vc, resid=r, parameter='c', **one)) <= 1e-12
        assert ac.rel(prob.Hvec(None, jc.stack(z, vr), resid=r, **kw)[N:], prob.Hvec(None, vr, resid=r, parameter='rho', **one)) <= 1e-12
        assert ac.rel(prob.Hvec(None, v, resid=np.zeros(sv.nD), **kw), H) <= 1e-12
        w = np.random.default_rng(8).uniform(0., 2., sv.nD)
        assert ac.rel(prob.Hvec(None, v, weights=w, **kw), prob.Jtvec(None, w * d, adjoint='transpose', **kw)) <= 1e-12
    # u = None solves the fields itself and gives the same
    assert ac.rel(prob.Hvec(None, v, resid=r, **FULL), prob.Hvec(None, v, u=uF, resid=r, **FULL)) <= 1e-12
    assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', **FULL), prob.Jtvec(None, r, u=uF, adjoint='transpose', **FULL)) <= 1e-12


# ---- 3. the Hessian against the gradient ---------------------------------------------------------------------------------------------------------------
# (case, linearisation, which halves of v are non-zero): 'full' with v_c in every cell on all four cases; 'operator' with v_c zero in the layers, compared outside
# them in the c half, on two cases that have both arrays and both classes; [p; 0] and [0; p] on two cases
TAYLOR = [(k, 'full', 'both') for k in CASES] + [(CASES[0], 'operator', 'both'), (CASES[3], 'operator', 'both')] + \
         [(CASES[1], 'full', 'c'), (CASES[1], 'full', 'rho'), (CASES[2], 'full', 'c'), (CASES[2], 'full', 'rho')]


def _without_the_mixed_terms(monkeypatch, call):
    'the joint Newton product of the host route with M_c^T and M_b^T left out: a wrong Hessian'
    with monkeypatch.context() as mp:
        mp.setattr(problem_module, 'mixedAdjointC', lambda op, P, db, **kw: np.zeros(int(op.nz) * int(op.nx), dtype=np.complex128))
        mp.setattr(problem_module, 'mixedAdjointB', lambda op, P, dc_, **kw: np.zeros(int(op.nz) * int(op.nx), dtype=np.complex128))
        return call()


@pytest.mark.parametrize('key,lin,halves', TAYLOR, ids=['%s-%s-%s' % (IDS[CASES.index(k)], l, h) for k, l, h in TAYLOR])
def test_central_differences_of_the_joint_gradient_converge_to_the_joint_newton_product(solved, monkeypatch, key, lin, halves):
    """||(g(m + h v) - g(m - h v)) / 2h - H v|| over fc.TAYLOR_H, in the c half and in the rho half, falls at second order with H v = Hvec(resid=r), g the joint gradient
    at fixed dobs, m = (c, rho) and v = [v_c; v_rho] (or [p; 0], [0; p]).  Against the Gauss-Newton product, and against the Newton product without the two mixed
    transposes, the remainders keep their size.  dobs is the data of (c + 40 m/s, rho x 1.03).  Conditions: the residual part is >= 0.1 of ||H v||, and the mixed
    terms -- measured directly, as the stacked product minus the one with M_c^T and M_b^T left out -- are >= 0.05 of it.  (The difference to what the
    single-parameter calls could assemble, the two Newton diagonal blocks plus the two Gauss-Newton off-diagonal blocks, is printed beside it.)"""
    s = solved[key]
    prob, sv, uF, r, N = s['prob'], s['sv'], s['uF'], s['r'], s['N']
    kw = dict(linearisation=lin, parameter='joint')
    layers = lin == 'operator'
    vc, vr = jc.directions(layers)
    keep = (vc != 0) if layers else slice(None)
    z = np.zeros(N)
    v = jc.stack(vc if halves in ('both', 'c') else z, vr if halves in ('both', 'rho') else z)
    jc.restore(prob)
    Hv = prob.Hvec(None, v, u=uF, resid=r, **kw)
    Hgn = prob.Hvec(None, v, u=uF, **kw)
    Hnomix = _without_the_mixed_terms(monkeypatch, lambda: prob.Hvec(None, v, u=uF, resid=r, **kw))
    g = jc.gradient_of(prob, sv, s['dobs'], linearisation=lin)
    try:
        rn = jc.central_remainders(g, v, Hv, N, keep)
        rg = jc.central_remainders(g, v, Hgn, N, keep, hs=fc.TAYLOR_H[-2:])
        rm = jc.central_remainders(g, v, Hnomix, N, keep, hs=fc.TAYLOR_H[-2:])
    finally:
        jc.restore(prob)
    pick = lambda a: np.concatenate((a[:N][keep], a[N:]))
    size = fc.norm(pick(Hv))
    resid_share, mixed_share = fc.norm(pick(Hv - Hgn)) / size, fc.norm(pick(Hv - Hnomix)) / size
    one = dict(u=uF, linearisation=lin)
    today = np.concatenate((prob.Hvec(None, v[:N], resid=r, parameter='c', **one) + prob.Hvec(None, v[N:], parameter=('rho', 'c'), **one),
                            prob.Hvec(None, v[:N], parameter=('c', 'rho'), **one) + prob.Hvec(None, v[N:], resid=r, parameter='rho', **one)))
    for half, name in ((0, 'c'), (1, 'rho')):
        print('%s %s %s, %s half: remainders %s factors %s; Gauss-Newton %s; without the mixed terms %s' % (
            key, lin, halves, name, [x[half] for x in rn], fc.factors([x[half] for x in rn]), [x[half] for x in rg], [x[half] for x in rm]))
    print('%s %s %s: residual share %.3f, mixed share %.3f (halves %.3f / %.3f), off-diagonal residual part against the diagonal Newton + Gauss-Newton blocks %.3f' % (
        key, lin, halves, resid_share, mixed_share, fc.norm((Hv - Hnomix)[:N][keep]) / fc.norm(Hv[:N][keep]), fc.norm((Hv - Hnomix)[N:]) / fc.norm(Hv[N:]),
        fc.norm(pick(Hv - today)) / size))
    for half in (0, 1):
        assert all(f >= jc.SECOND for f in fc.factors([x[half] for x in rn])), (half, rn)
    assert resid_share >= 0.1 and mixed_share >= 0.05
    for half in (0, 1):
        assert rg[0][half] / rg[1][half] <= jc.STALL                                    # (the last two remainders stall)
    # the stacked remainder without the mixed terms stalls at the part that is left out
    tot = [np.hypot(*x) for x in rm]
    assert tot[0] / tot[1] <= jc.STALL and tot[1] >= 0.5 * fc.norm(pick(Hv - Hnomix))


# ---- 4. symmetry -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_joint_newton_product_is_symmetric_to_ten_times_the_defect_of_gauss_newton(solved, key):
    "the criterion of test_newton_host.py on the stacked vectors: |<q, H v> - <v, H q>| / max of the two, Newton against Gauss-Newton on the same inputs"
    s = solved[key]
    prob, uF, r, N = s['prob'], s['uF'], s['r'], s['N']
    rng = np.random.default_rng(17)
    v, q = rng.standard_normal(2 * N), rng.standard_normal(2 * N)
    defect = []
    for extra in (dict(resid=r), dict()):
        a, b = float(q @ prob.Hvec(None, v, u=uF, **FULL, **extra)), float(v @ prob.Hvec(None, q, u=uF, **FULL, **extra))
        defect.append(abs(a - b) / max(abs(a), abs(b)))
    print('%s: joint symmetry defect %.2e, of the joint Gauss-Newton product %.2e' % (key, defect[0], defect[1]))
    assert defect[0] <= 10 * defect[1]


# ---- 5. the reference evaluations of the two kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_the_80_bit_mixed_transposes_bound_plain_fp64_and_reject_wrong_ones(name):
    sc = dc.operator_config(name)
    op = za.MiniZephyr(sc)
    p, B, P, G0 = jc.mixed_inputs(sc)
    w = -0.7 + 0.4j
    worst = {'b': [], 'c': []}
    for conj in (False, True):
        for stretch in (True, False):
            ref, mag = jc.mixed_b_reference(op, G0, P, p, w, conj, stretch)
            bound = jc.C_MIXED * jc.U64 * mag
            worst['b'].append(jc.worst_ratio(G0 + w * fr.mixedAdjointB(op, P, p, conj=conj, stretch=stretch), ref, bound))
            assert jc.worst_ratio(G0 + w * fr.mixedAdjointB(op, P, p, conj=conj, stretch=not stretch), ref, bound) > 1e6          # (the stretch part missing)
            if stretch:          # (the mass term alone has a real coefficient at a real frequency: nothing to conjugate; it has no stiffness part either)
                assert jc.worst_ratio(G0 + w * fr.mixedAdjointB(op, P, p, conj=not conj, stretch=True), ref, bound) > 1e6
                assert jc.worst_ratio(G0 + w * jc.mixed_b_with_p_of_the_cell(op, P, p, conj), ref, bound) > 1e6
                assert jc.worst_ratio(G0 + w * jc.mixed_b_without_the_centre_row(op, P, p, conj), ref, bound) > 1e6
            ref, mag = jc.mixed_c_reference(op, G0, P, B, w, conj, stretch)
            bound = jc.C_VADJOINT_B * jc.U64 * mag
            worst['c'].append(jc.worst_ratio(G0 + w * fr.mixedAdjointC(op, P, B, conj=conj, stretch=stretch), ref, bound))
            assert jc.worst_ratio(G0 + w * fr.mixedAdjointC(op, P, B, conj=conj, stretch=not stretch), ref, bound) > 1e6
            if stretch:
                assert jc.worst_ratio(G0 + w * fr.mixedAdjointC(op, P, B, conj=not conj, stretch=True), ref, bound) > 1e6
    print('%s: fp64 numpy at %s (mixedAdjointB) and %s (mixedAdjointC) of the bound' % (name, ['%.3f' % x for x in worst['b']], ['%.3f' % x for x in worst['c']]))
    assert max(worst['b']) <= 1.0 and max(worst['c']) <= 1.0
    # the helpers are what they say: with the missing pieces put back they are the transpose again
    assert ac.rel(jc.mixed_b_with_p_of_the_cell(op, P, np.full(p.size, 3.), False), fr.mixedAdjointB(op, P, np.full(p.size, 3.))) <= 1e-13


# ---- 6. the refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_joint_routes_do_not_serve_is_refused(solved):
    s = solved[('fixed', False)]
    prob, sv, uF, r, N = s['prob'], s['sv'], s['uF'], s['r'], s['N']
    v = np.ones(2 * N)
    for call in (lambda **kw: prob.Jtvec(None, r, u=uF, adjoint='transpose', **kw), lambda **kw: prob.JvecBorn(None, v, u=uF, **kw),
                 lambda **kw: prob.Hvec(None, v, u=uF, **kw), lambda **kw: prob.Hvec(None, v, u=uF, resid=r, **kw)):
        with pytest.raises(ValueError):
            call(parameter='joint')                                                  # ('scaler')
        with pytest.raises(ValueError):
            call(parameter='joint', linearisation='scaler')
    for bad in (np.ones(N), np.ones(2 * N + 1)):
        with pytest.raises(ValueError, match='stacked'):
            prob.JvecBorn(None, bad, u=uF, **FULL)
        with pytest.raises(ValueError, match='stacked'):
            prob.Hvec(None, bad, u=uF, **FULL)
        with pytest.raises(ValueError, match='stacked'):
            prob.Hvec(None, bad, u=uF, resid=r, **FULL)
    with pytest.raises(ValueError, match='weights'):
        prob.Hvec(None, v, u=uF, resid=r, weights=np.ones(sv.nD), **FULL)
    for pair in (('joint', 'c'), ('c', 'joint'), ('joint', 'joint'), ('rho', 'joint')):
        with pytest.raises(ValueError):
            prob.Hvec(None, v, u=uF, linearisation='full', parameter=pair)
        with pytest.raises(ValueError):
            prob.Hvec(None, v, u=uF, linearisation='full', parameter=pair, resid=r)
    for kind in ('pseudoHessian', 'gaussNewton', 'energy'):
        with pytest.raises(ValueError):
            prob.illumination(None, kind=kind, **FULL)
    with pytest.raises(ValueError, match='transpose'):
        prob.Jtvec(None, r, u=uF, **FULL)                                            # (adjoint='reciprocity')
    # the existing refusals of a pair and of a Gardner config with resid stay as they are
    for pair in (('c', 'rho'), ('rho', 'c')):
        with pytest.raises(NotImplementedError, match='not local'):
            prob.Hvec(None, np.ones(N), u=uF, resid=r, parameter=pair, linearisation='full')
    probg, svg = jc.pair('fixed', False, density=False)
    with pytest.raises(NotImplementedError, match='not local'):
        probg.Hvec(None, np.ones(N), resid=r, linearisation='full')
    for lin in ('full', 'operator'):
        for call in (lambda **kw: probg.Jtvec(None, r, adjoint='transpose', **kw), lambda **kw: probg.JvecBorn(None, v, **kw),
                     lambda **kw: probg.Hvec(None, v, **kw), lambda **kw: probg.Hvec(None, v, resid=r, **kw)):
            with pytest.raises(NotImplementedError, match='free parameter'):
                call(parameter='joint', linearisation=lin)


def test_the_other_operators_are_refused_with_the_sentences_they_carry():
    "the 2.5-D composite, visco, Eurus and multiscale: parameter='joint' refuses with the sentence the single-parameter call refuses with"
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
    for prob, sv in [(prob25, sv25), (probv, svv), (probe, sve), (probm, svm)]:
        v, v2, r = np.ones(prob.nrow), np.ones(2 * prob.nrow), np.ones(sv.nD, dtype=complex)
        for lin in ('full', 'operator'):
            said = []
            for call in (lambda: prob.Hvec(None, v2, resid=r, linearisation=lin, parameter='joint'), lambda: prob.Hvec(None, v2, linearisation=lin, parameter='joint'),
                         lambda: prob.Hvec(None, v, linearisation=lin), lambda: prob.JvecBorn(None, v2, linearisation=lin, parameter='joint'),
                         lambda: prob.Jtvec(None, r, adjoint='transpose', linearisation=lin, parameter='joint')):
                with pytest.raises(NotImplementedError) as ei:
                    call()
                said.append(str(ei.value))
            assert said[0] == said[1] == said[2] and said[0].replace('Hvec', 'JvecBorn') == said[3]
            assert said[0].split(' ', 1)[1] == said[4].split(' ', 1)[1]                # (Jtvec names itself with its adjoint: the sentence after the name)
