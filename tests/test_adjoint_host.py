"""CPU: the transposed 9-point operator and what stands on it -- the plane formula against the oracle's matrix, the adjoint identity between JvecBorn
and Jtvec(adjoint='transpose') on the oracle doubles (and that the default Jtvec misses it), Hvec as a symmetric positive semi-definite operator, routing
and refusals, and two gloo ranks against one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the plane formula ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(12, 9), (37, 53), (5, 300)])
@pytest.mark.parametrize('free', [False, True])
def test_transpose_planes_is_the_transposed_matrix_exactly(shape, free):
    nz, nx = shape
    c = ac.rough_model(nz, nx, 3)
    C = ho.minizephyr_coefficients(nz, nx, c, ho.gardner_rho(c), 20., dx=10., dz=8., nPML=4, ky=0.002, freeSurf=(free, False, False, False))
    A, AT = ho.coefficients_to_csr(C), ho.coefficients_to_csr(ac.transpose_planes(C))
    assert abs(A - A.T).max() > 0                                   # (the operator is not symmetric: the test tells the two apart)
    assert abs(AT - A.T).max() == 0.0
    # twice is the identity on every entry that is part of the matrix (entries pointing outside the grid are dropped by both)
    assert abs(ho.coefficients_to_csr(ac.transpose_planes(ac.transpose_planes(C))) - A).max() == 0.0


# ---- 2. the adjoint identity ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def solved():
    'per case: the pair, its host fields, a random model vector, a random residual, JvecBorn v and the two gradients -- made once, left unchanged'
    out = {}
    for case in ac.HOST_CASES:
        prob, sv = ac.host_pair(case)
        rng = np.random.default_rng(17)
        v = rng.standard_normal(prob.nrow)
        r = ac.randc(rng, sv.nD)
        uF = prob.fields()
        out[case] = dict(prob=prob, sv=sv, v=v, r=r, uF=uF, Jv=prob.JvecBorn(None, v, u=uF), gT=prob.Jtvec(None, r, u=uF, adjoint='transpose'),
                         gR=prob.Jtvec(None, r, u=uF))
    return out


@pytest.mark.parametrize('case', ac.HOST_CASES)
def test_jvecborn_and_the_transposed_jtvec_are_adjoint_and_the_default_jtvec_is_not(solved, case):
    s = solved[case]
    Jv, gT, gR = s['Jv'], s['gT'], s['gR']
    assert Jv.shape == (s['sv'].nD,) and Jv.dtype == np.complex128
    assert gT.shape == (s['prob'].nrow,) and gT.dtype == np.float64
    lhs = ac.inner(Jv, s['r'])
    miss = abs(lhs - ac.inner(s['v'], gT)) / abs(lhs)
    miss_default = abs(lhs - ac.inner(s['v'], gR)) / abs(lhs)
    print('%s: identity misses by %.2e with the transposed solve, by %.2e with the default Jtvec' % (case, miss, miss_default))
    assert miss <= 1e-10
    assert miss_default > 1e-2
    # u = None solves the fields itself and gives the same
    prob = s['prob']
    assert ac.rel(prob.Jtvec(None, s['r'], adjoint='transpose'), gT) <= 1e-12
    assert ac.rel(prob.JvecBorn(None, s['v']), Jv) <= 1e-12


# ---- 3. Hvec -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ac.HOST_CASES)
def test_hvec_is_symmetric_and_positive_semidefinite_with_and_without_weights(solved, case):
    s = solved[case]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    rng = np.random.default_rng(23)
    x, y = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow)
    for weights in (None, rng.uniform(0., 2., (sv.nrec, sv.nsrc, sv.nfreq))):
        Hx, Hy = prob.Hvec(None, x, u=uF, weights=weights), prob.Hvec(None, y, u=uF, weights=weights)
        assert Hx.shape == (prob.nrow,) and Hx.dtype == np.float64
        a, b = float(x @ Hy), float(Hx @ y)
        assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
        assert float(x @ Hx) >= 0 and float(y @ Hy) >= 0
        if weights is None:
            Jx = prob.JvecBorn(None, x, u=uF)
            assert abs(float(x @ Hx) - ac.inner(Jx, Jx)) <= 1e-10 * ac.inner(Jx, Jx)          # x^T H x = |J x|^2
    assert ac.rel(prob.Hvec(None, x), prob.Hvec(None, x, u=uF)) <= 1e-12
    with pytest.raises(ValueError):
        prob.Hvec(None, x, u=uF, weights=-np.ones(sv.nD))
    with pytest.raises(ValueError):
        prob.Hvec(None, x, u=uF, weights=np.ones(sv.nD - 1))


# ---- 4. routing and refusals ---------------------------------------------------------------------------------------------------------------
def test_the_default_jtvec_is_untouched_and_bad_values_are_refused(solved):
    s = solved['2d-fixed-freesurf']
    prob, r, uF = s['prob'], s['r'], s['uF']
    assert np.array_equal(prob.Jtvec(None, r, u=uF, adjoint='reciprocity'), prob.Jtvec(None, r, u=uF))
    gm = prob.Jtvec(None, r)
    assert np.iscomplexobj(gm) and np.array_equal(prob.Jtvec(None, r, adjoint='reciprocity').view(np.float64), gm.view(np.float64))
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=uF, adjoint='transposed')
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, adjoint=None)


def test_adjoint_system_follows_the_model_and_the_factors():
    prob, sv = ac.host_pair('2d-fixed-freesurf')
    c = prob.systemConfig['c']
    adj = prob.adjointSystem
    assert type(adj) is type(prob.system) and adj is not prob.system and prob.adjointSystem is adj
    assert [sub.transposed for sub in adj.subProblems] == [True] * 3 and [sub.transposed for sub in prob.system.subProblems] == [False] * 3
    assert [complex(a.freq) for a in adj.subProblems] == [complex(a.freq) for a in prob.system.subProblems]
    prob.updateModel(c)                                     # the same model: kept
    assert prob.adjointSystem is adj
    prob.updateModel(c * 1.01)
    assert prob.adjointSystem is not adj
    assert np.allclose(prob.adjointSystem.subProblems[0].c, c * 1.01)
    del prob.factors                                        # (reaches the transposed wrapper too; with the doubles there is nothing to free)
    # the composite hands the key to its ky sub-problems
    prob25, _ = ac.host_pair('25d-fixed')
    assert all(sub.transposed for comp in prob25.adjointSystem.subProblems for sub in comp.subProblems)
    assert not any(sub.transposed for comp in prob25.system.subProblems for sub in comp.subProblems)


def test_eurus_3d_and_multiscale_are_refused():
    import zephyr_amd as za
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    base = dict(nx=20, nz=24, dx=10., c=2500., freq=10., nPML=5)
    for cls in (za.Eurus, za.EurusHD):
        with pytest.raises(NotImplementedError):
            cls(dict(base, transposed=True))
        assert cls(dict(base, transposed=False)).transposed is False
    with pytest.raises(NotImplementedError):
        za.Helm3D(dict(base, ny=16, transposed=True))
    assert za.MiniZephyr(dict(base, transposed=True)).transposed is True and za.MiniZephyr(base).transposed is False
    # a problem whose discretisation is Eurus has no transposed wrapper
    sc = ac.survey_config(24, 20, 3, 5, ac.HOST_FREQS, 'fixed')
    sc.update(Disc=za.Eurus, hostGradient=True)
    prob, sv = ac.Helm2DProblem(sc), ac.Helm2DSurvey(sc)
    prob.pair(sv)
    with pytest.raises(NotImplementedError):
        prob.adjointSystem
    # multiscale surveys: all three routes
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    r, v = np.ones(svm.nD, dtype=complex), np.ones(probm.nrow)
    with pytest.raises(NotImplementedError):
        probm.Jtvec(None, r, adjoint='transpose')
    with pytest.raises(NotImplementedError):
        probm.JvecBorn(None, v)
    with pytest.raises(NotImplementedError):
        probm.Hvec(None, v)


WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
ok = True
for case in ('2d-fixed-freesurf', '2d-moving-hd'):
    ref, sref = ac.host_pair(case, shardFreqs=False)
    prob, sv = ac.host_pair(case)
    assert prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
    rng = np.random.default_rng(5)
    v, r = rng.standard_normal(prob.nrow), ac.randc(rng, sv.nD)
    ok = ok and ac.rel(prob.Jtvec(None, r, adjoint='transpose'), ref.Jtvec(None, r, adjoint='transpose')) < 1e-12
    ok = ok and ac.rel(prob.JvecBorn(None, v), ref.JvecBorn(None, v)) < 1e-12
    ok = ok and ac.rel(prob.Hvec(None, v), ref.Hvec(None, v)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'frequencies sharded over two ranks: every route ends in one all-reduce and every rank holds the single-rank result'
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29631', WORLD_SIZE='2', PYTHONPATH=ROOT)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
