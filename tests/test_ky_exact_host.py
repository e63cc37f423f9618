"""CPU: the exact derivatives of a 2.5-D problem (kyDerivatives=True) on the oracle doubles -- the Taylor test of dpred that the per-ky sum passes and the 'scaler'
fails, the adjoint identities, Hvec against its two halves, the joint calls against the single ones, nky = 1 against the 2-D problem, the gradient of the
ky-summed fields as a negative control, the refusals, and two gloo ranks."""
import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
from tests import ky_exact_cases as kc

CASES = [('fixed', False), ('relative', False), ('fixed', True)]
IDS = ['fixed-mz', 'moving-mz', 'fixed-hd']
T = dict(adjoint='transpose')
PARS = [('operator', 'c'), ('operator', 'rho'), ('operator', 'joint'), ('full', 'c'), ('full', 'rho'), ('full', 'joint')]


@pytest.fixture(scope='module')
def solved():
    'per case and density (explicit, Gardner): the pair, the model, the per-ky host fields and the data -- made once'
    out = {}
    for key in CASES:
        for density in (True, False):
            if not density and key != ('fixed', False):
                continue
            prob, sv = kc.host_pair(*key, density=density)
            c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
            out[key + (density,)] = dict(prob=prob, sv=sv, c0=c0, FK=prob.fields(perKy=True), d0=sv.dpred(c0))
    return out


def _vector(prob, par, seed):
    return np.random.default_rng(seed).standard_normal(2 * prob.nrow if par == 'joint' else prob.nrow)


# ---- 1. Taylor ---------------------------------------------------------------------------------------------------------------------------------------------
def _dpred_stepped(s, par, v):
    'h -> dpred at the model stepped by h along v (the velocity, the density of the config, or both); the caller puts the model back'
    prob, sv, c0 = s['prob'], s['sv'], s['c0']
    N = prob.nrow
    rho0 = None if prob.systemConfig.get('rho') is None else np.array(prob.systemConfig['rho'], dtype=np.float64)
    vc = v[:N].reshape(c0.shape) if par in ('c', 'joint') else None
    vr = (v[N:] if par == 'joint' else v).reshape(c0.shape) if par in ('rho', 'joint') else None

    def dpred(h):
        m = {'c': c0 + h * vc if vc is not None else c0}
        if vr is not None:
            m['rho'] = rho0 + h * vr
        prob.updateModel(m)
        return sv.dpred()
    return dpred, (lambda: prob.updateModel({'c': c0, 'rho': rho0} if rho0 is not None else {'c': c0}))


@pytest.mark.parametrize('name,key,par', [('full-rho', ('fixed', False, True), 'c'), ('full-gardner', ('fixed', False, False), 'c'), ('rho', ('relative', False, True), 'rho'),
                                          ('joint', ('fixed', True, True), 'joint')], ids=['full-rho', 'full-gardner', 'rho', 'joint'])
def test_taylor_remainder_of_dpred_falls_at_second_order(solved, name, key, par):
    'the perturbation is non-zero in every cell, +-50 as in test_full_host.py; five halvings, every factor in the second-order window'
    s = solved[key]
    prob = s['prob']
    v = np.concatenate((kc.perturbation(prob.nrow, 8), kc.perturbation(prob.nrow, 9))) if par == 'joint' else kc.perturbation(prob.nrow)
    Jv = prob.JvecBorn(None, v, u=s['FK'], linearisation='full', parameter=par)
    dpred, restore = _dpred_stepped(s, par, v)
    try:
        r = kc.taylor_remainders(dpred, s['d0'], Jv)
    finally:
        restore()
    f = fc.factors(r)
    print('%s: remainders %s factors %s' % (name, r, f))
    assert len(f) == 5 and all(x >= kc.SECOND for x in f)


def test_scaler_is_of_first_order_on_the_same_perturbation(solved):
    "negative control: the reference's gradientScaler on the ky SUM is not the derivative of dpred -- every factor stays in the first-order window (2.00 measured)"
    s = solved[('fixed', False, True)]
    prob = s['prob']
    v = kc.perturbation(prob.nrow)
    Jv = prob.JvecBorn(None, v, u=prob.fields(), linearisation='scaler')
    dpred, restore = _dpred_stepped(s, 'c', v)
    try:
        f = fc.factors(kc.taylor_remainders(dpred, s['d0'], Jv))
    finally:
        restore()
    print('scaler factors %s' % (f,))
    assert all(x <= kc.FIRST for x in f)


# ---- 2. the adjoint identities, Hvec, joint ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin,par', PARS, ids=['%s-%s' % p for p in PARS])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_born_data_and_gradient_are_adjoint(solved, key, lin, par):
    s = solved[key + (True,)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    x, r = _vector(prob, par, 17), ac.randc(np.random.default_rng(18), sv.nD)
    Jx = prob.JvecBorn(None, x, u=FK, linearisation=lin, parameter=par)
    g = prob.Jtvec(None, r, u=FK, linearisation=lin, parameter=par, **T)
    assert g.shape == x.shape and g.dtype == np.float64 and Jx.dtype == np.complex128 and Jx.shape == (sv.nD,)
    lhs = ac.inner(Jx, r)
    miss = abs(lhs - ac.inner(x, g)) / abs(lhs)
    print('%s %s %s: identity misses by %.2e' % (key, lin, par, miss))
    assert miss <= 1e-10


def test_gardner_pair_is_adjoint_and_u_none_gives_the_same(solved):
    s = solved[('fixed', False, False)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    x, r = _vector(prob, 'c', 3), ac.randc(np.random.default_rng(4), sv.nD)
    kw = dict(linearisation='full')
    Jx, g = prob.JvecBorn(None, x, u=FK, **kw), prob.Jtvec(None, r, u=FK, **kw, **T)
    lhs = ac.inner(Jx, r)
    assert abs(lhs - ac.inner(x, g)) <= 1e-10 * abs(lhs)
    assert ac.rel(prob.JvecBorn(None, x, **kw), Jx) <= 1e-12 and ac.rel(prob.Jtvec(None, r, **kw, **T), g) <= 1e-12
    assert ac.rel(prob.Hvec(None, x, **kw), prob.Hvec(None, x, u=FK, **kw)) <= 1e-12


@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_hvec_is_its_two_halves_symmetric_and_the_pairs_are_transposes(solved, key):
    s = solved[key + (True,)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    rng = np.random.default_rng(23)
    x, y = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow)
    w = rng.uniform(0.5, 1.5, sv.nD)
    for lin in ('operator', 'full'):
        for par in ('c', 'rho'):
            kw = dict(u=FK, linearisation=lin, parameter=par)
            H = lambda p: prob.Hvec(None, p, weights=w, **kw)
            assert ac.rel(H(x), prob.Jtvec(None, prob.JvecBorn(None, x, **kw) * w, **kw, **T)) <= 1e-12
            a, b = float(y @ H(x)), float(x @ H(y))
            assert abs(a - b) <= 1e-10 * max(abs(a), abs(b)), (lin, par)
        kw = dict(u=FK, linearisation=lin)
        a, b = float(y @ prob.Hvec(None, x, parameter=('c', 'rho'), **kw)), float(x @ prob.Hvec(None, y, parameter=('rho', 'c'), **kw))
        assert abs(a - b) <= 1e-10 * max(abs(a), abs(b)), lin
        xy = np.concatenate((x, y))
        Hj = prob.Hvec(None, xy, parameter='joint', **kw)
        a, b = float(xy @ Hj), ac.inner(prob.JvecBorn(None, xy, parameter='joint', **kw), prob.JvecBorn(None, xy, parameter='joint', **kw))
        assert abs(a - b) <= 1e-10 * b


@pytest.mark.parametrize('lin', ['operator', 'full'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_joint_is_the_two_single_parameter_calls(solved, key, lin):
    s = solved[key + (True,)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    N = prob.nrow
    xy, r = _vector(prob, 'joint', 31), ac.randc(np.random.default_rng(32), sv.nD)
    kw = dict(u=FK, linearisation=lin)
    g = prob.Jtvec(None, r, parameter='joint', **kw, **T)
    assert ac.rel(g[:N], prob.Jtvec(None, r, parameter='c', **kw, **T)) <= 1e-12 and ac.rel(g[N:], prob.Jtvec(None, r, parameter='rho', **kw, **T)) <= 1e-12
    both = prob.JvecBorn(None, xy[:N], parameter='c', **kw) + prob.JvecBorn(None, xy[N:], parameter='rho', **kw)
    assert ac.rel(prob.JvecBorn(None, xy, parameter='joint', **kw), both) <= 1e-12


# ---- 3. nky = 1 is the 2-D problem, and the summed fields are not enough --------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', [('fixed', False), ('relative', True)], ids=['fixed-mz', 'moving-hd'])
def test_one_ky_is_the_2d_problem_times_the_scale_term_of_the_composite(key):
    p25, s25 = kc.host_pair(*key, nky=1)
    p2, s2 = kc.host_pair_2d(*key)
    x, r = _vector(p25, 'c', 5), ac.randc(np.random.default_rng(6), s25.nD)
    st = np.exp(1j * np.pi) / (4 * np.pi)
    for lin, par in PARS:
        xx = _vector(p25, par, 5)
        assert ac.rel(p25.JvecBorn(None, xx, linearisation=lin, parameter=par), st * p2.JvecBorn(None, xx, linearisation=lin, parameter=par)) <= 1e-12, (lin, par)
    # the gradient pairs with the data: <st J v, r> = <v, J^T conj(st) r>
    assert ac.rel(p25.Jtvec(None, r, linearisation='full', **T), p2.Jtvec(None, np.conj(st) * r, linearisation='full', **T)) <= 1e-12


def test_gradient_from_the_summed_fields_misses_the_adjoint_identity(solved):
    'negative control: the maps applied to the product of the two ky SUMS -- a helper of the cases file, not a route -- are not the adjoint of the Born data'
    s = solved[('fixed', False, True)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    x, r = _vector(prob, 'c', 41), ac.randc(np.random.default_rng(42), sv.nD)
    lhs = ac.inner(prob.JvecBorn(None, x, u=FK, linearisation='full'), r)
    miss = abs(lhs - ac.inner(x, kc.summed_field_gradient(prob, r))) / abs(lhs)
    print('summed fields miss the identity by %.2e' % miss)
    assert miss > 1e-3


def test_per_ky_host_fields_sum_to_the_fields(solved):
    s = solved[('fixed', True, True)]
    prob = s['prob']
    F = prob.fields()
    for i, Fk in enumerate(s['FK']):
        assert Fk.shape == (kc.NKY, prob.nrow, s['sv'].nsrc) and ac.rel(Fk.sum(axis=0), F[i]) <= 1e-12
    premuls = [complex(sub.premul) for sub in prob.system.subProblems[0].subProblems]
    assert np.allclose(premuls, [1 / 5., 2 / 5., 2 / 5.]) and len({float(sub.ky) for sub in prob.system.subProblems[0].subProblems}) == kc.NKY


# ---- 4. the refusals -------------------------------------------------------------------------------------------------------------------------------------------
OLD = 'does not serve the 2.5-D composite: the stored fields are the ky SUM, the exact derivative needs the fields per ky'


def _calls(prob, sv, **kw):
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    return (lambda: prob.JvecBorn(None, v, **kw), lambda: prob.Jtvec(None, r, **kw, **T), lambda: prob.Hvec(None, v, **kw))


def test_without_the_key_the_old_sentence_still_comes():
    sc = kc.host_config()
    del sc['kyDerivatives']
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    for lin in ('operator', 'full'):
        for call in _calls(prob, sv, linearisation=lin):
            with pytest.raises(NotImplementedError) as ei:
                call()
            assert OLD in str(ei.value)
    with pytest.raises(NotImplementedError, match='ky SUM'):
        prob.Jtvec(None, np.ones(sv.nD, dtype=complex), linearisation='operator', parameter='rho', **T)
    assert prob.Jtvec(None, np.ones(sv.nD, dtype=complex), **T).shape == (prob.nrow,)          # ('scaler' is served as it always was)


def test_what_the_key_does_not_serve_is_refused_with_the_reason(solved):
    from zephyr_amd.problem import Helm25DViscoProblem
    from zephyr_amd.survey import Helm25DSurvey
    s = solved[('fixed', False, True)]
    prob, sv, FK = s['prob'], s['sv'], s['FK']
    v, r = np.ones(prob.nrow), np.ones(sv.nD, dtype=complex)
    # no explicit cmin: the quadrature nodes would move with the model
    sc = kc.host_config()
    del sc['cmin']
    p2, s2 = Helm25DProblem_pair(sc)
    for call in _calls(p2, s2, linearisation='full'):
        with pytest.raises(NotImplementedError, match='cmin'):
            call()
    # the ky-SUM fields with an exact linearisation
    for call in _calls(prob, sv, linearisation='full', u=prob.fields()):
        with pytest.raises(ValueError, match='perKy=True'):
            call()
    with pytest.raises(NotImplementedError, match=r'Hvec\(resid=\) does not serve the 2.5-D composite'):
        prob.Hvec(None, v, u=FK, linearisation='full', resid=r)
    for kw in (dict(kind='gaussNewton'), dict(kind='gaussNewton', linearisation='full'), dict(kind='pseudoHessian', linearisation='operator'),
               dict(kind='pseudoHessian', linearisation='full', parameter='rho')):
        with pytest.raises(NotImplementedError, match='not built per ky'):
            prob.illumination(**kw)
    assert prob.illumination(kind='pseudoHessian').shape == (prob.nrow,)          # (the 'scaler' kinds stay)
    for kind in ('pseudoHessian', 'gaussNewton'):
        with pytest.raises(NotImplementedError, match='not built per ky'):
            prob.hessianBlocks(kind=kind)
    # visco composites
    scv = kc.host_config(Q=50.)
    pv, sv_ = Helm25DViscoProblem(scv), Helm25DSurvey(scv)
    pv.pair(sv_)
    for call in _calls(pv, sv_, linearisation='full'):
        with pytest.raises(NotImplementedError, match='visco'):
            call()
    scv['viscoDerivatives'] = True
    pv, sv_ = Helm25DViscoProblem(scv), Helm25DSurvey(scv)
    pv.pair(sv_)
    for call in _calls(pv, sv_, linearisation='full'):
        with pytest.raises(NotImplementedError, match='Helm25DViscoProblem'):
            call()
    # perKy on a problem that has no ky axis
    p2d, _ = kc.host_pair_2d()
    with pytest.raises(ValueError, match='perKy=True'):
        p2d.fields(perKy=True)
    with pytest.raises(ValueError, match='perKy=True'):
        p2d.fieldsDevice(perKy=True)


def Helm25DProblem_pair(sc):
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def test_multiscale_pairings_are_refused():
    from zephyr_amd import MiniZephyr25D, MultiGridMultiFreq
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    from zephyr_amd.problem import Helm2DProblem
    from tests.test_moving_plan import multigrid_config
    scm = dict(multigrid_config(), Disc=MiniZephyr25D, nky=2, cmin=1500., SystemWrapper=MultiGridMultiFreq, rho=2000., kyDerivatives=True)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    for call in _calls(probm, svm, linearisation='full'):
        with pytest.raises(NotImplementedError, match='single-grid'):
            call()


def test_scaler_is_unchanged_by_the_key(solved):
    "'scaler' with the key is 'scaler' without it, bit for bit"
    s = solved[('fixed', False, True)]
    prob, sv = s['prob'], s['sv']
    sc = kc.host_config()
    del sc['kyDerivatives']
    ref, sref = Helm25DProblem_pair(sc)
    x, r = _vector(prob, 'c', 7), ac.randc(np.random.default_rng(8), sv.nD)
    F, Fr = prob.fields(), ref.fields()
    assert np.array_equal(prob.Jtvec(None, r, u=F, **T), ref.Jtvec(None, r, u=Fr, **T))
    assert np.array_equal(prob.JvecBorn(None, x, u=F), ref.JvecBorn(None, x, u=Fr))
    assert np.array_equal(sv.dpred(), sref.dpred())


# ---- 5. two ranks ----------------------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests import ky_exact_cases as kc
ok = True
ref, sref = kc.host_pair('relative', True, shardFreqs=False)
prob, sv = kc.host_pair('relative', True)
assert prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
rng = np.random.default_rng(5)
v, r = rng.standard_normal(2 * prob.nrow), ac.randc(rng, sv.nD)
kw = dict(linearisation='full', parameter='joint')
ok = ok and ac.rel(prob.Jtvec(None, r, adjoint='transpose', **kw), ref.Jtvec(None, r, adjoint='transpose', **kw)) < 1e-12
ok = ok and ac.rel(prob.JvecBorn(None, v, **kw), ref.JvecBorn(None, v, **kw)) < 1e-12
ok = ok and ac.rel(prob.Hvec(None, v[:prob.nrow], linearisation='full'), ref.Hvec(None, v[:prob.nrow], linearisation='full')) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'frequencies sharded over two ranks: gradient, Born data and the Gauss-Newton product end in one all-reduce each and every rank holds the single-rank result'
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29671', WORLD_SIZE='2', PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
