"""GPU: DataMisfit.valueAndGradient with the data kept on the device (device_survey.misfitFromFields and, with u None, the route it picks) against the generic
route of the same problem (misfitHostData: dpred down, the numpy functions, the adjoint source up through Jtvec) on the 37 x 53 device pair -- every kind, source
mode and parameter, fixed and moving arrays, HD and not, both store formats, the default density, two workers, two gloo ranks --, the Taylor test of the reduced
functional through the device route, and the bits of dpred and Jtvec before and after a misfit call."""
import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import misfit_cases as mc
from zephyr_amd import DataMisfit

pytestmark = pytest.mark.gpu

rel = ac.rel
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm
TOL = 1e-6                                        # device against host-map comparisons of tests/test_gpu_full.py and tests/test_gpu_joint.py (solves at rtol 1e-11)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def observed(prob, sv):
    'dobs of tests/test_misfit_host.py on the device pair: the data of c + perturbation, scaled by 1.3 - 0.4i, 2 % noise; the model is put back'
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    dobs = mc.observed(sv, None, sv.dpred(c0 + fc.perturbation(seed=12).reshape(c0.shape)))
    prob.updateModel(c0)
    return c0, dobs


def params(kind, sv, dobs):
    "the kind's parameters at the scale of the data: 'hybrid' epsilon and 'huber' threshold = the median of |dpred - dobs / (1.3 - 0.4i)|-like residuals"
    if kind not in ('huber', 'hybrid'):
        return dict(mc.PARAMS[kind])
    a = float(np.median(np.abs(sv.dpred().reshape(dobs.shape) * (1.3 - 0.4j) - dobs)))
    return dict(epsilon=a) if kind == 'hybrid' else dict(threshold=a)


def both_routes(prob, phi, u, **kw):
    'valueAndGradient through the device route and through the generic one, and their source terms'
    assert phi._deviceServes(u, kw.get('parameter', 'c'), kw.get('linearisation', 'full'))
    val, g = phi.valueAndGradient(None, u=u, **kw)
    s = phi.sourceTerms.copy()
    prob._misfitHostData = True
    try:
        assert not phi._deviceServes(u, kw.get('parameter', 'c'), kw.get('linearisation', 'full'))
        hval, hg = phi.valueAndGradient(None, u=u, **kw)
        hs = phi.sourceTerms.copy()
    finally:
        prob._misfitHostData = False
    return (val, s, g), (hval, hs, hg)


def errors(dev, host):
    return dict(val=abs(dev[0] - host[0]) / abs(host[0]), s=rel(dev[1], host[1]), g=rel(dev[2], host[2]))


@pytest.mark.parametrize('kind', mc.KINDS)
@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_the_device_route_against_the_host_data_route(helm_lib, monkeypatch, mode, kind):
    """value, source terms and gradient of every source mode and of 'c' / 'rho' / 'joint' within 1e-6 of the generic route on the same store (complex128), weights
    with dead traces that hold NaN; u = None agrees with u = F; the measured differences are printed"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair(mode, E2E[mode], device=True, rtol=1e-11)
    assert prob._deviceGradientAvailable()
    c0, dobs = observed(prob, sv)
    w = np.random.default_rng(2).uniform(0.5, 2., dobs.shape)
    w[3, :, 1] = 0.
    w[1, 2, :] = 0.
    dobs = np.where(w > 0, dobs, np.nan)
    pr = params(kind, sv, np.where(w > 0, dobs, 0))
    F = prob.fieldsDevice()
    worst = {}
    for source in mc.SOURCES:
        given = ac.randc(np.random.default_rng(4), (sv.nsrc, sv.nfreq)) if source == 'given' else None
        phi = DataMisfit(prob, dobs, kind=kind, weights=w, source=source, sourceTerms=given, **pr)
        for parameter, lin in (('c', 'full'), ('rho', 'operator'), ('joint', 'full'), ('c', 'operator')):
            kw = dict(parameter=parameter, linearisation=lin)
            dev, host = both_routes(prob, phi, F, **kw)
            e = errors(dev, host)
            assert dev[2].dtype == np.float64 and dev[2].shape == host[2].shape and dev[1].shape == (sv.nsrc, sv.nfreq)
            for k, x in e.items():
                worst[k] = max(worst.get(k, 0.), x)
            assert max(e.values()) <= TOL, (source, parameter, lin, e)
            if parameter == 'joint':
                joint = dev
        none = phi.valueAndGradient(None, parameter='joint', linearisation='full')
        e = errors((none[0], phi.sourceTerms, none[1]), joint)
        worst['u=None'] = max(worst.get('u=None', 0.), max(e.values()))
        assert max(e.values()) <= TOL, (source, 'u=None', e)
    print('%s %s: device against host data, worst relative differences %s' % (mode, kind, {k: '%.1e' % x for k, x in worst.items()}))
    F.release()
    del prob.factors


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_the_complex64_store_and_the_default_density(helm_lib, monkeypatch, mode):
    "the same comparison on a complex64 store (both routes read the same store), and linearisation='full' without `rho`, where Gardner's chain joins"
    monkeypatch.setenv('HELM_DEVICES', '0')
    for extra, density in ((dict(fieldsDtype='complex64'), True), ({}, False)):
        prob, sv = xc.pair(mode, E2E[mode], density=density, device=True, rtol=1e-11, **extra)
        c0, dobs = observed(prob, sv)
        F = prob.fieldsDevice()
        assert F.dtype == extra.get('fieldsDtype', 'complex128')
        for kind, source in (('hybrid', 'perFrequency'), ('logarithmic', 'perSource'), ('huber', 'given')):
            phi = DataMisfit(prob, dobs, kind=kind, source=source, **params(kind, sv, dobs))
            for parameter in (('c', 'rho', 'joint') if density else ('c',)):
                dev, host = both_routes(prob, phi, F, parameter=parameter, linearisation='full')
                e = errors(dev, host)
                print('%s %s %s %s %s: %s' % (mode, F.dtype, 'rho' if density else 'Gardner', kind, parameter, {k: '%.1e' % x for k, x in e.items()}))
                assert max(e.values()) <= TOL, e
        F.release()
        del prob.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: a per-frequency group spans both items, so the three passes run apart; u = None solves a store of its own"
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    c0, dobs = observed(prob, sv)
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    for kind, source in (('logarithmic', 'perFrequency'), ('hybrid', 'perSource'), ('l2', 'given')):
        phi = DataMisfit(prob, dobs, kind=kind, source=source, **params(kind, sv, dobs))
        for parameter in ('c', 'joint'):
            dev, host = both_routes(prob, phi, F, parameter=parameter, linearisation='full')
            e = errors(dev, host)
            none = phi.valueAndGradient(None, parameter=parameter, linearisation='full')
            e['u=None'] = max(errors((none[0], phi.sourceTerms, none[1]), dev).values())
            print('two workers %s %s %s: %s' % (kind, source, parameter, {k: '%.1e' % x for k, x in e.items()}))
            assert max(e.values()) <= TOL, e
    F.release()
    del prob.factors


@pytest.mark.parametrize('source', mc.SOURCES)
@pytest.mark.parametrize('kind', ['l2', 'hybrid', 'logarithmic'])
def test_taylor_test_of_the_reduced_functional_through_the_device_route(helm_lib, monkeypatch, kind, source):
    "central differences of the device route's value at h = 0.25, 0.125, 0.0625 approach g . v of the device route's gradient: error ratios >= 3.5"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('relative', True, device=True, rtol=1e-11)
    c0, dobs = observed(prob, sv)
    phi = DataMisfit(prob, dobs, kind=kind, source=source, **params(kind, sv, dobs))
    assert phi._deviceServes(None, 'c', 'full')
    value = lambda c: phi.valueAndGradient(c)[0]
    g = phi.valueAndGradient(c0)[1]
    errs, ratios, lin = mc.central_ratios(value, g, c0, fc.perturbation(seed=13))
    print('%s %s: relative errors %s, ratios %s' % (kind, source, [e / abs(lin) for e in errs], ratios))
    assert min(ratios) >= mc.TAYLOR
    del prob.factors


def test_a_misfit_call_leaves_dpred_and_jtvec_as_they_were(helm_lib, monkeypatch):
    "dpred and Jtvec with a host residual give the bits they gave before a misfit call (the pipelines take a host `resid` on the path it took)"
    monkeypatch.setenv('HELM_DEVICES', '0')
    for mode in ('fixed', 'relative'):
        prob, sv = xc.pair(mode, E2E[mode], device=True, rtol=1e-11)
        c0, dobs = observed(prob, sv)
        r = ac.randc(np.random.default_rng(6), dobs.shape)
        F = prob.fieldsDevice()
        calls = [lambda: sv.dpred(u=F), lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full'),
                 lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='operator', parameter='joint'), lambda: prob.Jtvec(None, r, u=F)]
        before = [call() for call in calls]
        for source in mc.SOURCES:
            phi = DataMisfit(prob, dobs, kind='hybrid', source=source, **params('hybrid', sv, dobs))
            phi.valueAndGradient(None, u=F, parameter='joint')
            phi.valueAndGradient(None)
        for call, b in zip(calls, before):
            assert np.array_equal(bits(call()), bits(b))
        F.release()
        del prob.factors


def test_what_the_device_route_leaves_to_the_generic_one(helm_lib, monkeypatch):
    "a host list of fields, the reference's scaler, hostGradient and the config key go through the generic route, silently; a stale store is refused as Jtvec refuses it"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', False, device=True, rtol=1e-11)
    c0, dobs = observed(prob, sv)
    phi = DataMisfit(prob, dobs)
    F = prob.fieldsDevice()
    assert phi._deviceServes(F, 'c', 'full') and phi._deviceServes(None, 'joint', 'operator')
    assert not phi._deviceServes(list(F), 'c', 'full') and not phi._deviceServes(F, 'c', 'scaler') and not phi._deviceServes(F, 'Q', 'full')
    val, g = phi.valueAndGradient(None, u=F)
    hval, hg = phi.valueAndGradient(None, u=list(F))
    assert abs(val - hval) <= TOL * abs(hval) and rel(g, hg) <= TOL
    prob.updateModel(c0 + 1.)
    with pytest.raises(ValueError, match='belong to an earlier model'):
        phi.valueAndGradient(None, u=F)
    F.release()
    off, _ = xc.pair('fixed', False, device=True, rtol=1e-11, misfitHostData=True)
    assert not DataMisfit(off, dobs)._deviceServes(None, 'c', 'full')
    del prob.factors


RANKS = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
os.environ['HELM_DEVICES'] = '0'
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac, full_cases as xc, misfit_cases as mc
from tests.test_gpu_misfit_routes import observed, params
from zephyr_amd import DataMisfit
ref, sref = xc.pair('relative', True, device=True, rtol=1e-11, shardFreqs=False)
prob, sv = xc.pair('relative', True, device=True, rtol=1e-11)
assert prob._deviceGradientAvailable() and prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
c0, dobs = observed(ref, sref)
ok = True
for kind, source, par in (('hybrid', 'perFrequency', 'joint'), ('logarithmic', 'perSource', 'c'), ('l2', 'given', 'rho')):
    pr = params(kind, sref, dobs)
    one, many = DataMisfit(ref, dobs, kind=kind, source=source, **pr), DataMisfit(prob, dobs, kind=kind, source=source, **pr)
    assert many._deviceServes(None, par, 'full')
    want = one.valueAndGradient(None, parameter=par)
    F = prob.fieldsDevice()
    assert F.ownedFreqs == prob.ownedFreqs
    e = []
    for u in (F, None):
        val, g = many.valueAndGradient(None, u=u, parameter=par)
        e += [abs(val - want[0]) / abs(want[0]), ac.rel(many.sourceTerms, one.sourceTerms), ac.rel(g, want[1])]
    F.release()
    print('RANK', dist.get_rank(), kind, source, par, ['%%.2e' %% x for x in e], flush=True)
    ok = ok and max(e) <= 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(helm_lib, tmp_path):
    """the three frequencies sharded over two ranks on one GPU: the sums of a group are local to the rank that owns the frequency, the value and the source
    terms are all-reduced, and the gradient's all-reduce gives every rank the single-rank result"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'ranks.py'
    script.write_text(RANKS % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29671', WORLD_SIZE='2', PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        print(o)
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
