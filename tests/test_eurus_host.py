"""CPU: what the config key eurusDerivatives serves on Eurus problems with eps == delta, on the oracle doubles of tests/eurus_cases.py -- the planes of
frechet.eurusPlanes against the oracle's assembly by Taylor remainders (edge rows included), the transposes of frechet.eurusAdjoint, Taylor tests of dpred
in c, in rho and jointly, the dot-product identities of every linearisation and parameter, and the refusals with and without the key."""
import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac
from tests import eurus_cases as ec
from tests import frechet_cases as fc
import zephyr_amd as za
from zephyr_amd import frechet as fr
from zephyr_amd.problem import Helm2DProblem
from zephyr_amd.survey import Helm2DSurvey

T = dict(adjoint='transpose')


# ---- 1. the planes against the oracle's assembly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aniso', ec.ANISO)
@pytest.mark.parametrize('grid', ['20x24', '37x53'])
def test_taylor_remainder_of_the_planes_on_every_row_and_not_without_the_edge_rows(grid, aniso):
    """||M1(c + h dc, b + h db) - M1(c, b) - h dM1||_inf over ALL rows of the oracle's block 0, dc and db non-zero in every cell: second order along dc and along
    both; along db alone M1 is linear and the remainder is rounding.  With the edge rows' centre entry left out every remainder is of first order."""
    sc = ec.operator_config(grid, aniso)
    op = za.Eurus(sc)
    nz, nx = sc['nz'], sc['nx']
    dc, db, _, _, _ = ec.kernel_inputs(sc)
    c0, b0 = np.asarray(sc['c']), 1.0 / np.asarray(sc['rho'])
    A0 = ec.oracle_c4(op)[0]
    assert np.abs(fr.eurusPlanes(op, db=b0.ravel()) - A0).max() <= 64 * ec.U64 * np.abs(A0).max()          # (homogeneous of degree one in b: L[b] is M1 itself)
    for name, vc, vb in (('dc', dc, None), ('db', None, db), ('both', dc, db)):
        full, noedge = fr.eurusPlanes(op, vc, vb), fr.eurusPlanes(op, vc, vb, edges=False)
        edge = ~fr._interiorMask(nz, nx)
        assert np.all(full[4][edge] != 0) and np.all(noedge[:, edge] == 0) and np.array_equal(full[:, ~edge], noedge[:, ~edge])
        rem = {'full': [], 'noedge': []}
        for h in fc.TAYLOR_H:
            c1 = c0 if vc is None else c0 + h * vc.reshape((nz, nx))
            b1 = b0 if vb is None else b0 + h * vb.reshape((nz, nx))
            D = ec.oracle_c4(op, c=c1, rho=1.0 / b1)[0] - A0
            rem['full'].append(float(np.abs(D - h * full).max()))
            rem['noedge'].append(float(np.abs(D - h * noedge).max()))
        print('%s %s %s: %s' % (grid, aniso, name, {k: ['%.2f' % f for f in fc.factors(r)] for k, r in rem.items()}))
        if name == 'db':
            assert max(rem['full']) <= 64 * ec.U64 * np.abs(A0).max()
        else:
            assert all(f >= ec.SECOND for f in fc.factors(rem['full']))
        assert all(f <= ec.FIRST for f in fc.factors(rem['noedge']))


# ---- 2. the transposes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aniso', ec.ANISO)
@pytest.mark.parametrize('grid', ['20x24', '37x53'])
def test_adjoint_is_the_plain_transpose_of_both_maps(grid, aniso):
    "<V[dc] + L[db], P> = <dc, V^T P> + <db, L^T P> under the bilinear pairing for random complex P, non-zero on the boundary rows, to rounding; the same conjugated"
    sc = ec.operator_config(grid, aniso)
    op = za.Eurus(sc)
    dc, db, P, _, _ = ec.kernel_inputs(sc)
    edge = ~fr._interiorMask(sc['nz'], sc['nx']).ravel()
    assert np.all(P[:, edge] != 0)
    D = fr.eurusPlanes(op, dc, db).reshape((9, -1))
    scale = (fr.eurusPlanes(op, dc, db, magnitude=True).reshape((9, -1)) * np.abs(P)).sum()
    for conj in (False, True):
        gc, gb = fr.eurusAdjoint(op, P, conj=conj)
        lhs, rhs = ((np.conj(D) if conj else D) * P).sum(), (dc * gc).sum() + (db * gb).sum()
        assert abs(lhs - rhs) <= 64 * ec.U64 * scale, (grid, aniso, conj, abs(lhs - rhs) / scale)
        assert abs(lhs) > 1e3 * 64 * ec.U64 * scale
    # each map alone, and the part that only the edge rows carry
    gc, gb = fr.eurusAdjoint(op, P)
    assert abs((fr.eurusPlanes(op, dc).reshape((9, -1)) * P).sum() - (dc * gc).sum()) <= 64 * ec.U64 * scale
    assert abs((fr.eurusPlanes(op, None, db).reshape((9, -1)) * P).sum() - (db * gb).sum()) <= 64 * ec.U64 * scale
    gc0, gb0 = fr.eurusAdjoint(op, P, edges=False)
    assert np.abs(gb - gb0).max() > 0 and np.abs(gc - gc0).max() > 0
    # the lag products with the centre plane on the boundary lines
    z, u = ac.randc(np.random.default_rng(3), (op.nrow, 2)), ac.randc(np.random.default_rng(4), (op.nrow, 2))
    P0, P1 = fr.lagProducts(z, u, op.nz, op.nx), fr.lagProducts(z, u, op.nz, op.nx, edges=True)
    assert np.all(P0[:, edge] == 0) and np.array_equal(P0[:, ~edge], P1[:, ~edge])
    assert np.allclose(P1[4, edge], (z * u).sum(axis=1)[edge], rtol=1e-14, atol=0) and np.all(P1[:4, edge] == 0) and np.all(P1[5:, edge] == 0)


# ---- 3. Taylor at the level of dpred -------------------------------------------------------------------------------------------------------------------
CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-eu', 'fixed-hd', 'moving-eu', 'moving-hd']


@pytest.fixture(scope='module')
def solved():
    'per case and density: the pair, its model, the host fields and the perturbations -- made once, left unchanged'
    out = {}
    for key in CASES:
        for density in (True, False):
            prob, sv = ec.host_pair(*key, density=density)
            vc, vr = ec.perturbations(prob.nrow)
            out[key + (density,)] = dict(prob=prob, sv=sv, c0=np.array(prob.systemConfig['c']), rho0=np.array(prob.systemConfig['rho']) if density else None,
                                         vc=vc, vr=vr, uF=prob.fields())
    return out


def _remainders(s, Jv, vc, vr):
    '||d(c0 + h vc, rho0 + h vr) - d(c0, rho0) - h Jv|| over fc.TAYLOR_H; the model is put back'
    prob, sv, c0, rho0 = s['prob'], s['sv'], s['c0'], s['rho0']
    shape = c0.shape

    def dpred(h):
        m = {}
        if vc is not None:
            m['c'] = c0 + h * vc.reshape(shape)
        if vr is not None:
            m['rho'] = rho0 + h * vr.reshape(shape)
        return sv.dpred(m)
    d0 = sv.dpred({'c': np.array(c0)} if rho0 is None else {'c': np.array(c0), 'rho': np.array(rho0)})
    r = [fc.norm(dpred(h) - d0 - h * Jv) for h in fc.TAYLOR_H]
    prob.updateModel({'c': np.array(c0)} if rho0 is None else {'c': np.array(c0), 'rho': np.array(rho0)})
    return r


@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_taylor_remainder_of_dpred_in_c_is_second_order_with_full_and_first_with_scaler(solved, key, density):
    s = solved[key + (density,)]
    prob, uF, vc = s['prob'], s['uF'], s['vc']
    r = _remainders(s, prob.JvecBorn(None, vc, u=uF, linearisation='full'), vc, None)
    rs = _remainders(s, prob.JvecBorn(None, vc, u=uF, linearisation='scaler'), vc, None)
    print('%s %s: full %s scaler %s' % (key, density, fc.factors(r), fc.factors(rs)))
    assert all(f >= ec.SECOND for f in fc.factors(r))
    assert all(f <= ec.FIRST for f in fc.factors(rs))
    if density:          # the C-PML does not depend on c: 'operator' is the same derivative
        assert ac.rel(prob.JvecBorn(None, vc, u=uF, linearisation='operator'), prob.JvecBorn(None, vc, u=uF, linearisation='full')) == 0.0


@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_taylor_remainder_of_dpred_in_rho_and_jointly_is_second_order(solved, key):
    s = solved[key + (True,)]
    prob, uF, vc, vr = s['prob'], s['uF'], s['vc'], s['vr']
    r = _remainders(s, prob.JvecBorn(None, vr, u=uF, linearisation='full', parameter='rho'), None, vr)
    rj = _remainders(s, prob.JvecBorn(None, np.concatenate((vc, vr)), u=uF, linearisation='full', parameter='joint'), vc, vr)
    print('%s: rho %s joint %s' % (key, fc.factors(r), fc.factors(rj)))
    assert all(f >= ec.SECOND for f in fc.factors(r))
    assert all(f >= ec.SECOND for f in fc.factors(rj))


def test_a_source_on_the_top_grid_line_needs_the_edge_rows(solved):
    "the sources sit on edge rows, whose centre entry depends on the model: second order as it is, first order with the edge terms of the host route off"
    prob, sv = ec.host_pair('fixed', False, top_source=True)
    s = dict(prob=prob, sv=sv, c0=np.array(prob.systemConfig['c']), rho0=np.array(prob.systemConfig['rho']))
    vc, vr = ec.perturbations(prob.nrow)
    v = np.concatenate((vc, vr))
    uF = prob.fields()
    kw = dict(u=uF, linearisation='full', parameter='joint')
    r = _remainders(s, prob.JvecBorn(None, v, **kw), vc, vr)
    prob._eurusEdgeTerms = False
    try:
        Jwrong = prob.JvecBorn(None, v, **kw)
        rng = np.random.default_rng(5)
        res = ac.randc(rng, sv.nD)
        lhs = ac.inner(Jwrong, res)
        assert abs(lhs - ac.inner(v, prob.Jtvec(None, res, **T, **kw))) <= 1e-10 * abs(lhs)          # (the flag reaches both halves: still adjoint)
    finally:
        prob._eurusEdgeTerms = True
    rw = _remainders(s, Jwrong, vc, vr)
    print('top source: factors %s, without the edge terms %s' % (fc.factors(r), fc.factors(rw)))
    assert all(f >= ec.SECOND for f in fc.factors(r))
    # (the statement of tests/test_full_host.py for a derivative that misses a term: the factors fall from step to step, leave the second-order window and end inside
    # the first-order one -- at h = 1 the common h^2 term still weighs in)
    f = fc.factors(rw)
    assert f[0] > f[1] > f[2] and f[2] <= ec.FIRST and min(f) < ec.SECOND


# ---- 4. dot products ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_jvecborn_and_jtvec_are_adjoint_for_every_linearisation_and_parameter(solved, key, density):
    """<JvecBorn v, r> = <v, Jtvec r> to 1e-10 (tests/test_adjoint_host.py) for 'scaler', 'operator', 'full', 'rho', 'joint'; the reciprocity Jtvec misses it;
    joint equals the two single-parameter calls to 1e-12 (tests/test_joint_host.py); Hvec is symmetric"""
    s = solved[key + (density,)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    N = prob.nrow
    rng = np.random.default_rng(17)
    r = ac.randc(rng, sv.nD)
    combos = [('scaler', 'c'), ('full', 'c')] + ([('operator', 'c'), ('operator', 'rho'), ('full', 'rho'), ('operator', 'joint'), ('full', 'joint')] if density else [])
    for lin, par in combos:
        v = rng.standard_normal(2 * N if par == 'joint' else N)
        kw = dict(u=uF, linearisation=lin, parameter=par)
        Jv, g = prob.JvecBorn(None, v, **kw), prob.Jtvec(None, r, **T, **kw)
        assert Jv.shape == (sv.nD,) and g.shape == v.shape and g.dtype == np.float64
        lhs = ac.inner(Jv, r)
        miss = abs(lhs - ac.inner(v, g)) / abs(lhs)
        print('%s %s %s %s: identity misses by %.2e' % (key, density, lin, par, miss))
        assert miss <= 1e-10
        if (lin, par) in (('scaler', 'c'), ('full', 'joint' if density else 'c')):          # (Hvec is the composition of the two: its symmetry once per kind)
            x, y = rng.standard_normal(v.size), rng.standard_normal(v.size)
            a, b = float(x @ prob.Hvec(None, y, **kw)), float(prob.Hvec(None, x, **kw) @ y)
            assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    gR = prob.Jtvec(None, r, u=uF)
    v = rng.standard_normal(N)
    lhs = ac.inner(prob.JvecBorn(None, v, u=uF), r)
    assert abs(lhs - ac.inner(v, gR)) / abs(lhs) > 1e-3          # (M1 is not symmetric: the default back-propagation is not the adjoint)
    if density:
        one = dict(u=uF, linearisation='full')
        gj = prob.Jtvec(None, r, parameter='joint', **T, **one)
        assert ac.rel(gj[:N], prob.Jtvec(None, r, parameter='c', **T, **one)) <= 1e-12
        assert ac.rel(gj[N:], prob.Jtvec(None, r, parameter='rho', **T, **one)) <= 1e-12
        vc, vr = rng.standard_normal(N), rng.standard_normal(N)
        dj = prob.JvecBorn(None, np.concatenate((vc, vr)), parameter='joint', **one)
        assert ac.rel(dj, prob.JvecBorn(None, vc, parameter='c', **one) + prob.JvecBorn(None, vr, parameter='rho', **one)) <= 1e-12
        Hc = prob.Hvec(None, vc, parameter=('c', 'rho'), **one)
        assert ac.rel(Hc, prob.Jtvec(None, prob.JvecBorn(None, vc, **one), parameter='rho', **T, **one)) <= 1e-12
        # u = None solves the fields itself and gives the same
        assert ac.rel(prob.Jtvec(None, r, parameter='joint', linearisation='full', **T), gj) <= 1e-12


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_the_key_set(solved):
    s = solved[CASES[0] + (True,)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    N = prob.nrow
    v, r = np.ones(N), np.ones(sv.nD, dtype=complex)
    with pytest.raises(NotImplementedError, match='Eurus'):
        prob.Hvec(None, v, u=uF, linearisation='full', resid=r)
    for kw in (dict(kind='gaussNewton'), dict(kind='gaussNewton', linearisation='full'), dict(kind='pseudoHessian', linearisation='full'),
               dict(kind='pseudoHessian', linearisation='operator', parameter='rho')):
        with pytest.raises(NotImplementedError, match='Eurus'):
            prob.illumination(None, u=uF, **kw)
    assert np.all(prob.illumination(None, u=uF, kind='energy') >= 0) and np.all(prob.illumination(None, u=uF, kind='pseudoHessian') >= 0)
    with pytest.raises(NotImplementedError, match='Eurus'):
        prob.hessianBlocks(None, u=uF)
    # without `rho`: the sentences 'operator', 'rho' and 'joint' carry for MiniZephyr
    g = solved[CASES[0] + (False,)]
    for kw in (dict(linearisation='operator'), dict(linearisation='full', parameter='rho'), dict(linearisation='full', parameter='joint')):
        with pytest.raises(NotImplementedError, match='explicit `rho`'):
            g['prob'].Jtvec(None, r, u=g['uF'], **T, **kw)
    # eps != delta anywhere
    sc = ec.survey_config('fixed', False, aniso='vti')
    e2 = np.array(sc['eps'])
    e2[10, 10] += 0.01
    sc.update(eps=e2, Disc=ec.OracleEurus, hostGradient=True)
    pc, svc = Helm2DProblem(sc), Helm2DSurvey(sc)
    pc.pair(svc)
    for call in (lambda: pc.Jtvec(None, r, **T), lambda: pc.Jtvec(None, r, linearisation='full', **T), lambda: pc.JvecBorn(None, v, linearisation='full'),
                 lambda: pc.Hvec(None, v, linearisation='full'), lambda: pc.adjointSystem):
        with pytest.raises(NotImplementedError, match='coupled'):
            call()
    for cls in (za.Eurus, za.EurusHD):
        with pytest.raises(NotImplementedError, match='coupled'):
            cls(dict(ec.operator_config('20x24', 'vti'), eps=0.1, delta=0.05, transposed=True))
        assert cls(dict(ec.operator_config('20x24', 'tilted'), transposed=True)).transposed is True
    # visco, 2.5-D and multiscale problems keep the sentences they carry
    from zephyr_amd.problem import Helm2DViscoProblem, Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    scv = ec.survey_config('fixed', False)
    scv.update(Disc=ec.OracleEurus, hostGradient=True, Q=80.)
    pv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    pv.pair(svv)
    with pytest.raises(NotImplementedError, match='visco'):
        pv.Jtvec(None, r, linearisation='full', **T)
    sc25 = ac.survey_config(24, 20, 3, 5, ac.HOST_FREQS, 'fixed')
    sc25.update(Disc=ac.OracleMiniZephyr25DT, nky=2, kyOnDevice=False, hostGradient=True, eurusDerivatives=True, rho=2000.)
    p25, s25 = Helm25DProblem(sc25), Helm25DSurvey(sc25)
    p25.pair(s25)
    with pytest.raises(NotImplementedError, match='2.5-D'):
        p25.Jtvec(None, np.ones(s25.nD, dtype=complex), linearisation='full', **T)
    # a multiscale pairing of Eurus operators with the key: the single-grid sentence of every route and of adjointSystem, before anything Eurus is looked at
    from zephyr_amd import MultiGridMultiFreq
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    for cls in (za.Eurus, za.EurusHD):
        scm = dict(multigrid_config(), Disc=cls, SystemWrapper=MultiGridMultiFreq, eurusDerivatives=True, rho=2000.)
        pm, sm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
        pm.pair(sm)
        assert pm._eurusDerivatives is True
        rm, vm = np.ones(sm.nD, dtype=complex), np.ones(pm.nrow)
        for lin, par, x in (('scaler', 'c', vm), ('operator', 'c', vm), ('full', 'c', vm), ('full', 'rho', vm), ('full', 'joint', np.ones(2 * pm.nrow))):
            kw = dict(linearisation=lin, parameter=par)
            for call in (lambda: pm.Jtvec(None, rm, **T, **kw), lambda: pm.JvecBorn(None, x, **kw), lambda: pm.Hvec(None, x, **kw)):
                with pytest.raises(NotImplementedError, match='serves single-grid surveys: the transposed operator and the stored forward fields live on one grid'):
                    call()
        with pytest.raises(NotImplementedError, match='the transposed operator serves single-grid problems: a multiscale pairing has no exact-adjoint route'):
            pm.adjointSystem


def test_without_the_key_every_eurus_call_raises_what_it_raised():
    "the sentences of the parent commit, word for word"
    base = dict(nx=20, nz=24, dx=10., c=2500., freq=10., nPML=5)
    for cls in (za.Eurus, za.EurusHD):
        with pytest.raises(NotImplementedError) as ei:
            cls(dict(base, transposed=True))
        assert str(ei.value) == '%s has no transposed operator: helm_set_transposed serves 2-D MiniZephyr handles (not Eurus, not the 3-D operator)' % cls.__name__
        assert cls(base).TRANSPOSABLE is False and cls(dict(base, eurusDerivatives=True)).TRANSPOSABLE is True
        assert cls(dict(base, eurusDerivatives=True, eps=0.1, delta=0.2)).TRANSPOSABLE is False
    sc = ec.survey_config('fixed', False)
    del sc['eurusDerivatives']
    sc.update(Disc=ec.OracleEurus, hostGradient=True)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    v, r = np.ones(prob.nrow), np.ones(sv.nD, dtype=complex)
    with pytest.raises(NotImplementedError, match='has no transposed operator: helm_set_transposed serves 2-D MiniZephyr handles'):
        prob.adjointSystem
    with pytest.raises(NotImplementedError, match='has no transposed operator'):
        prob.Jtvec(None, r, **T)
    for lin, par in (('operator', 'c'), ('full', 'c'), ('operator', 'rho'), ('full', 'joint')):
        for call in (lambda: prob.Jtvec(None, r, linearisation=lin, parameter=par, **T), lambda: prob.JvecBorn(None, v, linearisation=lin, parameter=par),
                     lambda: prob.Hvec(None, v, linearisation=lin, parameter=par)):
            with pytest.raises(NotImplementedError) as ei:
                call()
            assert 'serves the 2-D MiniZephyr operators: OracleEurus assembles its mass term differently' in str(ei.value)
    assert np.iscomplexobj(prob.Jtvec(None, r))          # (the reciprocity gradient is served as it always was)


# ---- 6. two ranks --------------------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests import eurus_cases as ec
ok = True
ref, sref = ec.host_pair('relative', True, shardFreqs=False)
prob, sv = ec.host_pair('relative', True)
assert prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
rng = np.random.default_rng(5)
v, r = rng.standard_normal(2 * prob.nrow), ac.randc(rng, sv.nD)
kw = dict(linearisation='full', parameter='joint')
ok = ok and ac.rel(prob.Jtvec(None, r, adjoint='transpose', **kw), ref.Jtvec(None, r, adjoint='transpose', **kw)) < 1e-12
ok = ok and ac.rel(prob.JvecBorn(None, v, **kw), ref.JvecBorn(None, v, **kw)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'frequencies sharded over two ranks: the joint gradient and the joint Born data end in one all-reduce and every rank holds the single-rank result'
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29659', WORLD_SIZE='2', PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
