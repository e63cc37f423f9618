"""CPU: HelmBaseProblem.illumination on the host path (arithmetic by the oracle double) -- the shared extended-precision helper against plain fp64 and
against deliberately wrong evaluations, then the g6 survey: both kinds from solved and from given fields, the per-frequency rows, the receiver side,
what is refused, a multiscale problem, and two gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.doubles import OracleMiniZephyrHD
from tests.illumination_cases import NPATTERN, energy_columns, energy_exact, energy_check, energy_fp64, energy_wrong, energy_entry
from zephyr_amd.problem import Helm2DProblem
from zephyr_amd.survey import Helm2DSurvey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def make(g, Disc=OracleMiniZephyrHD, mode='fixed', **extra):
    'the pairing of tests/test_survey_gradient.py'
    nz, nx = g['c'].shape
    rec = g['rec'] if mode == 'fixed' else g['rec_relative']
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=Disc, parallel=False,
              sterms=g['sterms'], geom=dict(src=g['src'], rec=rec, mode=mode))
    sc.update(extra)
    prob, surv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(surv)
    return prob, surv


def formula(prob, fields, kind, perFreq=False):
    'section 1 of the definition, evaluated directly: sum_f |gradientScaler(f)|^2 sum_s |uF[f][:, s]|^2 (no weight for kind energy)'
    rows = []
    for ifreq, uf in enumerate(fields):
        E = (np.abs(np.asarray(uf)) ** 2).sum(axis=1)
        rows.append(E * np.abs(prob.gradientScaler(ifreq)) ** 2 if kind == 'pseudoHessian' else E)
    rows = np.stack(rows)
    return rows if perFreq else rows.sum(axis=0)


def close(a, b, tol=1e-13):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


# ---- the helper itself ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nsrc', [1, 5, 13, 67])
def test_helper_accepts_plain_fp64_and_rejects_wrong_evaluations(nsrc):
    """the longdouble evaluation and its bound hold a plain fp64 evaluation in the kernels' order, with and without weights and a non-zero E on entry, and
    throw out an evaluation that squares only the real part of one column or skips the last one"""
    N = 257
    rng = np.random.default_rng(nsrc)
    for start in range(NPATTERN):
        cols = range(start, start + nsrc)
        U = energy_columns(N, cols, seed=start)
        for alpha, W in ((1.0, None), (0.37, 10.0 ** rng.uniform(-3, 3, N))):
            E0 = energy_entry(rng, energy_exact(U, alpha, W))
            exact = energy_exact(U, alpha, W, E0)
            assert exact.dtype == np.longdouble and np.all(exact >= 0)
            bad, worst = energy_check(energy_fp64(U, alpha, W, E0), exact, nsrc)
            assert bad == 0 and worst <= 1.0, (start, worst)
            norms = np.abs(U).max(axis=0)
            big = int(np.argmax(norms))
            if norms[big] > 0:              # the column that decides the sum somewhere: its imaginary part is missed
                assert energy_check(energy_wrong(U, 'real_only', alpha, W, E0, col=big), exact, nsrc)[0] > 0, start
            if nsrc > 1 and norms[-1] > 0 and norms[-1] >= 1e-3 * norms[:-1].max():
                assert energy_check(energy_wrong(U, 'skip_last', alpha, W, E0), exact, nsrc)[0] > 0, start
    # two launches onto the same E: the bounds add
    U1, U2 = energy_columns(N, [0, 8, 12], seed=1), energy_columns(N, [9, 10], seed=2)
    exact = energy_exact(U2, 2.0, None, energy_exact(U1))
    assert energy_check(energy_fp64(U2, 2.0, None, energy_fp64(U1)), exact, (3, 2))[0] == 0


# ---- g6 with the oracle double -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g6():
    g = np.load(os.path.join(GOLD, 'g6_survey.npz'))
    prob, surv = make(g)
    return g, prob, surv, prob.fields()


@pytest.mark.parametrize('kind', ['energy', 'pseudoHessian'])
def test_g6_both_kinds_from_solved_and_from_given_fields(g6, kind):
    g, prob, surv, uF = g6
    assert not prob._deviceGradientAvailable()                 # (the oracle double has no device path: this is the host branch)
    ref = formula(prob, uF, kind)
    H = prob.illumination(kind=kind)
    assert H.shape == (prob.nrow,) and H.dtype == np.float64 and np.all(H >= 0) and H.max() > 0
    assert close(H, ref)
    assert close(prob.illumination(u=uF, kind=kind), ref)
    rows = prob.illumination(kind=kind, perFreq=True)
    assert rows.shape == (surv.nfreq, prob.nrow) and rows.dtype == np.float64
    assert close(rows, formula(prob, uF, kind, perFreq=True))
    assert close(rows.sum(axis=0), H)
    assert close(prob.illumination(u=uF, kind=kind, perFreq=True), rows)


def test_pseudo_hessian_is_the_default_and_scalers_can_be_complex():
    g = np.load(os.path.join(GOLD, 'g6_survey.npz'))
    prob, surv = make(g, c=g['c'] * (1.0 + 0.02j))
    uF = prob.fields()
    assert np.iscomplexobj(prob.gradientScaler(0))
    assert close(prob.illumination(u=uF), formula(prob, uF, 'pseudoHessian'))
    assert close(prob.illumination(), prob.illumination(kind='pseudoHessian'), 0.0)


@pytest.mark.parametrize('kind', ['energy', 'pseudoHessian'])
def test_receiver_side_uses_the_receiver_array_as_sources(g6, kind):
    g, prob, surv, _ = g6
    cols = surv.rVec(0).T
    assert cols.shape == (prob.nrow, surv.nrec)
    uR = list(prob.system * ([cols] * surv.nfreq))                    # scaleTerm * (sub_f * columns): srTerms inside rVec, no tsTerms
    HR = prob.illumination(kind=kind, side='receiver')
    assert HR.shape == (prob.nrow,) and close(HR, formula(prob, uR, kind))
    assert close(prob.illumination(kind=kind, side='receiver', perFreq=True), formula(prob, uR, kind, perFreq=True))
    assert not close(HR, prob.illumination(kind=kind), 1e-3)


def test_what_is_refused(g6):
    g, prob, surv, uF = g6
    with pytest.raises(ValueError):
        prob.illumination(kind='hessian')
    with pytest.raises(ValueError):
        prob.illumination(side='both')
    with pytest.raises(ValueError):
        prob.illumination(u=uF, side='receiver')
    probr, _ = make(g, mode='relative')
    with pytest.raises(ValueError):
        probr.illumination(side='receiver')
    assert probr.illumination().shape == (probr.nrow,)          # the source side does not look at the receivers


def test_multiscale_problem_goes_through_the_host_path(helm_lib):
    'every frequency on its own grid: the fields pass through the post-processors as fields() does, the scaler through gradientScaler'
    from tests.test_regrid_host import ScipyGridInterpolator
    from zephyr_amd.distributors import ViscoMultiGridMultiFreq
    from zephyr_amd.problem import Helm2DViscoMultiGridProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    rng = np.random.default_rng(5)
    nz, nx = 40, 48
    c = 2000. + 300. * rng.random((nz, nx))
    src = np.array([[100., 60.], [250., 80.]])
    rec = np.stack([np.linspace(40., 380., 7), np.full(7, 300.)], axis=1)
    sc = dict(nx=nx, nz=nz, dx=9., dz=9., c=c, rho=1000. + 200. * rng.random((nz, nx)), Q=40. + 60. * rng.random((nz, nx)), freqBase=5., nPML=5,
              freqs=[6., 25.], cMin=1500., targetGPW=12., Disc=OracleMiniZephyrHD, parallel=False, SystemWrapper=ViscoMultiGridMultiFreq,
              GridInterpolator=ScipyGridInterpolator, geom=dict(src=src, rec=rec, mode='fixed'), hostGradient=True)
    prob, sv = Helm2DViscoMultiGridProblem(sc), Helm2DMultiGridSurvey(sc)
    prob.pair(sv)
    assert sv.mgHelper.scales[0] > 1. and prob.system.subProblems[0].nrow < prob.nrow
    uF = prob.fields()
    for kind in ('energy', 'pseudoHessian'):
        H = prob.illumination(kind=kind)
        assert H.shape == (nz * nx,) and close(H, formula(prob, uF, kind), 1e-12)
        assert close(prob.illumination(u=uF, kind=kind, perFreq=True), formula(prob, uF, kind, perFreq=True))
    uR = [pp(u) for u, pp in zip(prob.system * [sv.rVec(0, i).T for i in range(sv.nfreq)], sv.postProcessors)]
    assert close(prob.illumination(side='receiver'), formula(prob, uR, 'pseudoHessian'), 1e-12)


# ---- two ranks -----------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests.test_illumination_host import make, close, GOLD
g = dict(np.load(os.path.join(GOLD, 'g6_survey.npz')))
one = %(one)r
kw = dict(freqs=[float(g['freqs'][1])], sterms=g['sterms'][1:2]) if one else {}
ref_prob, _ = make(g, shardFreqs=False, **kw)
prob, surv = make(g, **kw)
nf = surv.nfreq
assert prob.ownedFreqs == list(range(dist.get_rank(), nf, 2))          # (one frequency: rank 1 owns nothing and must still enter the all-reduce)
rows = prob.illumination(perFreq=True)                                 # (rows of the other rank's frequencies arrive through the all-reduce)
ok = rows.shape == (nf, prob.nrow) and close(rows, ref_prob.illumination(perFreq=True), 1e-13)
ok = ok and close(prob.illumination(kind='energy', side='receiver'), ref_prob.illumination(kind='energy', side='receiver'), 1e-13)
ok = ok and close(prob.illumination(u=ref_prob.fields()), rows.sum(axis=0), 1e-13)
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


@pytest.mark.parametrize('one,port', [(False, '29627'), (True, '29629')])
def test_two_gloo_ranks_return_the_single_process_result(tmp_path, one, port):
    """world size 2 with the frequencies sharded: ONE all-reduce gives both ranks the single-process result, per-frequency rows included; with a single
    frequency rank 1 owns none and still enters the collective (no hang)"""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT, one=one))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=port, WORLD_SIZE='2', PYTHONPATH=ROOT, OMP_NUM_THREADS='1')       # (two ranks with a thread pool each only get in each other's way)
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
