"""GPU: DataMisfit.valueAndGradient(u=None) in one pass without a store (device_survey.misfitOnePass) against the route over a complex128 store
(device_survey.misfitFromFields): the same bits of the value, the source terms and the gradient where the items coincide -- every kind, source mode and
pipeline ('c' with 'operator' and 'full', the default density, 'rho', 'joint') --, which route u = None takes, and that no store is made."""
import numpy as np
import pytest

from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import misfit_cases as mc
from tests.test_gpu_misfit_routes import E2E, bits, observed, params
from zephyr_amd import DataMisfit
from zephyr_amd import device_survey

pytestmark = pytest.mark.gpu

PIPELINES = (('c', 'full'), ('c', 'operator'), ('rho', 'operator'), ('joint', 'full'), ('joint', 'operator'))


@pytest.mark.parametrize('kind', mc.KINDS)
@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_one_pass_gives_the_bits_of_the_store_route(helm_lib, monkeypatch, mode, kind):
    """u = None against u = F on a complex128 store: the items coincide (one worker, a frequency per item), the kernels, their inputs and the order in which the
    worker adds to its partial are the same, and so are the bits -- for every source mode ('perFrequency': every frequency's columns fit one item) and pipeline;
    fieldsDevice is not called"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair(mode, E2E[mode], device=True, rtol=1e-11)
    c0, dobs = observed(prob, sv)
    w = np.random.default_rng(2).uniform(0.5, 2., dobs.shape)
    w[3, :, 1] = 0.
    pr = params(kind, sv, dobs)
    F = prob.fieldsDevice()
    stores = []
    monkeypatch.setattr(type(prob), 'fieldsDevice', lambda self, *a, **k: stores.append(1))
    for source in mc.SOURCES:
        phi = DataMisfit(prob, dobs, kind=kind, weights=w, source=source, **pr)
        items = device_survey.deviceItems(prob.system, prob.ownedFreqs, sv.nsrc)[1]
        assert device_survey.misfitInOnePass(phi, items) and [it[2:] for it in items] == [it[2:] for it in F.items]
        for parameter, lin in PIPELINES:
            kw = dict(parameter=parameter, linearisation=lin)
            val, g = phi.valueAndGradient(None, u=F, **kw)
            s = phi.sourceTerms.copy()
            val1, g1 = phi.valueAndGradient(None, **kw)
            assert val1 == val and np.array_equal(bits(phi.sourceTerms), bits(s)) and np.array_equal(bits(g1), bits(g)), (source, parameter, lin)
            assert np.array_equal(bits(phi.valueAndGradient(None, **kw)[1]), bits(g1))          # (and on a second call)
    assert not stores
    F.release()
    del prob.factors


def test_one_pass_with_the_default_density(helm_lib, monkeypatch):
    "linearisation='full' without `rho`: the buoyancy partial and Gardner's chain, the same bits as over the store"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('relative', True, density=False, device=True, rtol=1e-11)
    c0, dobs = observed(prob, sv)
    F = prob.fieldsDevice()
    for kind, source in (('hybrid', 'perSource'), ('logarithmic', 'perFrequency')):
        phi = DataMisfit(prob, dobs, kind=kind, source=source, **params(kind, sv, dobs))
        val, g = phi.valueAndGradient(None, u=F)
        val1, g1 = phi.valueAndGradient(None)
        assert val1 == val and np.array_equal(bits(g1), bits(g))
    F.release()
    del prob.factors


def test_two_workers(helm_lib, monkeypatch):
    """two workers on GPU 0 with half the sources of one frequency each: 'given' and 'perSource' run in one pass (the bits of the store route, whose items are
    the same deal); a per-frequency group spans both items, so u = None solves a store and releases it"""
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    c0, dobs = observed(prob, sv)
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    made = []
    real = type(prob).fieldsDevice
    monkeypatch.setattr(type(prob), 'fieldsDevice', lambda self, *a, **k: (made.append(1), real(self, *a, **k))[1])
    for source in mc.SOURCES:
        phi = DataMisfit(prob, dobs, kind='hybrid', source=source, **params('hybrid', sv, dobs))
        val, g = phi.valueAndGradient(None, u=F, parameter='joint')
        del made[:]
        val1, g1 = phi.valueAndGradient(None, parameter='joint')
        assert len(made) == (1 if source == 'perFrequency' else 0)
        assert val1 == val and np.array_equal(bits(g1), bits(g)), source
    F.release()
    del prob.factors
