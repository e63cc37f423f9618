"""GPU: the exact derivatives of a 2.5-D problem (kyDerivatives=True) through the per-ky store -- the device routes of Jtvec / JvecBorn / Hvec against the host
route on the oracle doubles fed the downloaded per-ky blocks (both stores, fixed and moving arrays, every parameter), u = None, a repeated call and kyRelease
against u = FK bit for bit, dpred(u=FK), two workers, the adjoint identity, the Taylor test of dpred through the device routes, and the routes that must stay
what they were.  37 x 53 (several separator levels), nky = 3, two frequencies, 3 sources, 5 receivers."""
import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
from tests import ky_exact_cases as kc
from zephyr_amd import device_survey

pytestmark = pytest.mark.gpu

rel, randc, inner = ac.rel, ac.randc, ac.inner
T = dict(adjoint='transpose')
E2E = {'fixed': False, 'relative': True}          # mode -> a complex scaleTerm
PARS = [('full', 'c'), ('full', 'rho'), ('full', 'joint'), ('operator', 'c'), ('operator', 'joint')]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _inputs(prob, sv, par, seed=31):
    rng = np.random.default_rng(seed)
    n = 2 * prob.nrow if par == 'joint' else prob.nrow
    return rng.standard_normal(n), rng.standard_normal(n), randc(rng, sv.nD)


def _no_store(*args, **kwargs):
    raise AssertionError('u = None of the exact 2.5-D routes allocates no store')


def _blocks(F, nfreq):
    return [F.kyBlocks(i) for i in range(nfreq)]


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_route_fed_the_downloaded_blocks(helm_lib, monkeypatch, mode):
    """complex128 store: 1e-6 against the oracle doubles and the identity at 1e-7, the tolerances of test_gpu_full.py (the solver runs at rtol 1e-11 against the
    oracle's LU); u = None and a second call give the bits of u = FK; the store counts its nky blocks and still downloads the ky sum"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = kc.device_pair(mode, E2E[mode])
    probh, svh = kc.host_of(mode, E2E[mode])
    assert prob._deviceGradientAvailable() and not probh._deviceGradientAvailable()
    FK = prob.fieldsDevice(perKy=True)
    assert FK.nky == kc.NKY and sum(FK.nbytes.values()) == kc.NKY * sv.nfreq * sv.nsrc * prob.nrow * 16
    blocks = _blocks(FK, sv.nfreq)
    F, Fh = prob.fields(), probh.fields(perKy=True)
    for i in range(sv.nfreq):
        assert blocks[i].shape == (kc.NKY, prob.nrow, sv.nsrc)
        assert rel(FK[i], F[i]) <= 1e-12 and rel(blocks[i].sum(axis=0), F[i]) <= 1e-12
        assert rel(blocks[i], Fh[i]) <= 1e-6
    for lin, par in PARS:
        v, p, r = _inputs(prob, sv, par)
        kw = dict(u=FK, linearisation=lin, parameter=par)
        kh = dict(u=blocks, linearisation=lin, parameter=par)
        gT, Jv, Hp = prob.Jtvec(None, r, **kw, **T), prob.JvecBorn(None, v, **kw), prob.Hvec(None, p, **kw)
        assert gT.shape == v.shape and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128 and Hp.dtype == np.float64
        eg, ej, eh = rel(gT, probh.Jtvec(None, r, **kh, **T)), rel(Jv, probh.JvecBorn(None, v, **kh)), rel(Hp, probh.Hvec(None, p, **kh))
        lhs = inner(Jv, r)
        miss = abs(lhs - inner(v, gT)) / abs(lhs)
        print('%s %s %s: Jtvec against the host route %.2e, JvecBorn %.2e, Hvec %.2e; identity misses by %.2e' % (mode, lin, par, eg, ej, eh, miss))
        assert eg <= 1e-6 and ej <= 1e-6 and eh <= 1e-6
        assert miss <= 1e-7
        assert np.array_equal(bits(prob.Jtvec(None, r, **kw, **T)), bits(gT)) and np.array_equal(bits(prob.JvecBorn(None, v, **kw)), bits(Jv))      # (twice)
        kn = dict(linearisation=lin, parameter=par)
        with monkeypatch.context() as mp:          # (u = None: the same bits, and no store is solved -- the fields of a ky live in the workspace)
            mp.setattr(device_survey, 'fields', _no_store)
            assert np.array_equal(bits(prob.Jtvec(None, r, **kn, **T)), bits(gT)) and np.array_equal(bits(prob.JvecBorn(None, v, **kn)), bits(Jv))
            assert np.array_equal(bits(prob.Hvec(None, p, **kn)), bits(Hp))
    # the pairs of Hvec, with data weights
    v, p, r = _inputs(prob, sv, 'c', 5)
    w = np.random.default_rng(6).uniform(0.5, 1.5, sv.nD)
    kw = dict(linearisation='full', weights=w)
    a = prob.Hvec(None, v, u=FK, parameter=('c', 'rho'), **kw)
    assert rel(a, probh.Hvec(None, v, u=blocks, parameter=('c', 'rho'), **kw)) <= 1e-6
    x, y = float(p @ a), float(v @ prob.Hvec(None, p, u=FK, parameter=('rho', 'c'), **kw))
    assert abs(x - y) <= 1e-7 * max(abs(x), abs(y))
    FK.release()
    del prob.factors


def test_gardner_density_through_the_device_route(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = kc.device_pair('fixed', False, density=False)
    probh, _ = kc.host_of('fixed', False, density=False)
    FK = prob.fieldsDevice(perKy=True)
    blocks = _blocks(FK, sv.nfreq)
    v, p, r = _inputs(prob, sv, 'c')
    kw, kh = dict(u=FK, linearisation='full'), dict(u=blocks, linearisation='full')
    gT, Jv = prob.Jtvec(None, r, **kw, **T), prob.JvecBorn(None, v, **kw)
    assert rel(gT, probh.Jtvec(None, r, **kh, **T)) <= 1e-6 and rel(Jv, probh.JvecBorn(None, v, **kh)) <= 1e-6
    lhs = inner(Jv, r)
    assert abs(lhs - inner(v, gT)) <= 1e-7 * abs(lhs)
    with pytest.raises(NotImplementedError, match='rho'):
        prob.JvecBorn(None, v, u=FK, linearisation='operator')
    FK.release()
    del prob.factors


def test_complex64_store_against_the_host_route_on_the_unpacked_blocks(helm_lib, monkeypatch):
    "the format bound of test_gpu_full.py's complex64 test: the device on the packed store against the host route on the same, unpacked blocks; one exponent per column and ky"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = kc.device_pair('relative', True)
    prob64, sv64 = kc.device_pair('relative', True, fieldsDtype='complex64')
    probh, _ = kc.host_of('relative', True)
    FK, FK64 = prob.fieldsDevice(perKy=True), prob64.fieldsDevice(perKy=True)
    assert FK64.dtype == 'complex64' and FK64.nky == kc.NKY
    assert sum(FK64.nbytes.values()) == kc.NKY * sv.nfreq * sv.nsrc * (prob.nrow * 8 + 4)
    unpacked = _blocks(FK64, sv.nfreq)
    # a component is off by at most 2^-24 of its column's largest, so a block by sqrt(2 N) 2^-24 of its norm at the most
    assert 0 < rel(unpacked[0], FK.kyBlocks(0)) <= np.sqrt(2 * prob.nrow) * 2.0 ** -24
    for lin, par in (('full', 'c'), ('full', 'joint')):
        v, p, r = _inputs(prob, sv, par)
        kw, kh = dict(u=FK64, linearisation=lin, parameter=par), dict(u=unpacked, linearisation=lin, parameter=par)
        d64, g64 = prob64.JvecBorn(None, v, **kw), prob64.Jtvec(None, r, **kw, **T)
        ed, eg = rel(d64, probh.JvecBorn(None, v, **kh)), rel(g64, probh.Jtvec(None, r, **kh, **T))
        print('%s %s complex64: JvecBorn against the host route on the unpacked blocks %.2e, Jtvec %.2e' % (lin, par, ed, eg))
        assert ed <= 1e-6 and eg <= 1e-6
        assert rel(d64, prob.JvecBorn(None, v, u=FK, linearisation=lin, parameter=par)) > 0           # (the packed store was read)
        lhs = inner(d64, r)
        assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    FK.release()
    FK64.release()
    del prob.factors, prob64.factors


def test_dpred_from_the_per_ky_store_and_ky_release(helm_lib, monkeypatch):
    "dpred(u=FK) forms the ky sum while sampling: dpred() to 1e-12; kyRelease=True gives the bits of False"
    monkeypatch.setenv('HELM_DEVICES', '0')
    out = {}
    for release in (False, True):
        prob, sv = kc.device_pair('fixed', True, kyRelease=release)
        FK = prob.fieldsDevice(perKy=True)
        d = sv.dpred(u=FK)
        assert rel(d, sv.dpred()) <= 1e-12
        v, p, r = _inputs(prob, sv, 'joint')
        kw = dict(u=FK, linearisation='full', parameter='joint')
        out[release] = (d, prob.Jtvec(None, r, **kw, **T), prob.JvecBorn(None, v, **kw), prob.Hvec(None, p, **kw), prob.Jtvec(None, r, linearisation='full', **T))
        if release:
            assert not prob.factors and not prob.adjointSystem.factors          # (every ky operator of either system went after its last use)
        FK.release()
        del prob.factors
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(bits(a), bits(b))


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with a batch of the sources each: per-ky blocks per item, the partials added on the host"
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = kc.device_config('relative', True, freqs=[kc.GPU_FREQS[1]], sterms=np.array([0.8 - 0.3j]))
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    FK = prob.fieldsDevice(perKy=True)
    assert len(FK.items) == 2
    blocks = _blocks(FK, 1)
    probh, _ = kc.host_of('relative', True, freqs=[kc.GPU_FREQS[1]], sterms=np.array([0.8 - 0.3j]))
    assert rel(sv.dpred(u=FK), sv.dpred()) <= 1e-12
    v, p, r = _inputs(prob, sv, 'joint')
    kw, kh = dict(u=FK, linearisation='full', parameter='joint'), dict(u=blocks, linearisation='full', parameter='joint')
    assert rel(prob.Jtvec(None, r, **kw, **T), probh.Jtvec(None, r, **kh, **T)) <= 1e-6
    assert rel(prob.JvecBorn(None, v, **kw), probh.JvecBorn(None, v, **kh)) <= 1e-6
    assert rel(prob.Hvec(None, p, **kw), probh.Hvec(None, p, **kh)) <= 1e-6
    assert rel(prob.Hvec(None, p, linearisation='full', parameter='joint'), probh.Hvec(None, p, **kh)) <= 1e-6
    FK.release()
    del prob.factors


@pytest.mark.parametrize('par', ['c', 'joint'])
def test_taylor_remainder_of_the_device_dpred_falls_at_second_order(helm_lib, monkeypatch, par):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = kc.device_pair('fixed', False)
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    rho0 = np.array(prob.systemConfig['rho'], dtype=np.float64)
    N = prob.nrow
    v = np.concatenate((kc.perturbation(N, 8), kc.perturbation(N, 9))) if par == 'joint' else kc.perturbation(N)
    FK = prob.fieldsDevice(perKy=True)
    Jv = prob.JvecBorn(None, v, u=FK, linearisation='full', parameter=par)
    d0 = sv.dpred(u=FK)
    FK.release()

    def dpred(h):
        prob.updateModel({'c': c0 + h * v[:N].reshape(c0.shape), 'rho': rho0 + (h * v[N:].reshape(c0.shape) if par == 'joint' else 0.)})
        return sv.dpred()
    r = kc.taylor_remainders(dpred, d0, Jv, hs=fc.TAYLOR_H)
    print('device %s: remainders %s factors %s' % (par, r, fc.factors(r)))
    assert all(f >= kc.SECOND for f in fc.factors(r))
    del prob.factors


def test_existing_routes_give_the_same_bits_before_and_after_and_the_sum_store_is_refused(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = kc.device_pair('fixed', True)
    v, p, r = _inputs(prob, sv, 'c')

    def existing():
        F = prob.fieldsDevice()
        assert F.nky is None
        out = (sv.dpred(), sv.dpred(u=F), prob.Jtvec(None, r, u=F, **T), prob.JvecBorn(None, v, u=F), prob.Jtvec(None, r), F[0], F[1])
        return F, out
    F, before = existing()
    for call in (lambda: prob.Jtvec(None, r, u=F, linearisation='full', **T), lambda: prob.JvecBorn(None, v, u=F, linearisation='operator'),
                 lambda: prob.Hvec(None, v, u=F, linearisation='full', parameter='c')):
        with pytest.raises(ValueError, match='perKy=True'):
            call()
    F.release()
    FK = prob.fieldsDevice(perKy=True)
    prob.Jtvec(None, r, u=FK, linearisation='full', **T)
    prob.Hvec(None, v, u=FK, linearisation='full')
    with pytest.raises(ValueError, match='per ky'):
        prob.Jtvec(None, r, u=FK, **T)                                   # ('scaler' reads the ky sum)
    FK.release()
    F, after = existing()
    F.release()
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    # without the key the device problem refuses as it always did
    sc = kc.device_config('fixed', True)
    del sc['kyDerivatives']
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    old, sold = Helm25DProblem(sc), Helm25DSurvey(sc)
    old.pair(sold)
    with pytest.raises(NotImplementedError, match='the stored fields are the ky SUM'):
        old.Jtvec(None, r, linearisation='full', **T)
    assert np.array_equal(bits(old.Jtvec(None, r, **T)), bits(prob.Jtvec(None, r, **T)))
    del prob.factors, old.factors
