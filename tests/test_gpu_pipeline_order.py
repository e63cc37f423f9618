"""GPU: the order of library calls inside a work item of every device pipeline of zephyr_amd.device_survey.

The library runs on its own streams, so a torch operation whose result a library call reads has to be followed by `_lib.wait_torch_stream` before that
call.  A pipeline that drops one of those waits still computes the right numbers most of the time, so no test of results sees where they sit.  Here
every work item's calls are recorded in order -- the `*Device` methods of the operators entered (those a composite hands on to its ky operators
included), the grid transfers (`apply_device`) of a multiscale survey, and every `_lib.wait_torch_stream`, those made inside the methods as well -- and
compared with the sequences written out below.

The surveys are those of tests/test_gpu_adjoint.py (96 x 80, 3 frequencies, 13 sources, 7 receivers; fixed and moving array; both store formats), its
2.5-D composite with nky = 2, and the multiscale pair of tests/test_gpu_multiscale.py.  HELM_DEVICES=0,0 deals the three frequencies to the worker of
GPU 0 all the same (a frequency stays with the GPU its operator lives on); with ONE frequency the two workers take its sources 0-6 and 6-13 on two
threads, so that layout is recorded as well."""
import threading

import numpy as np
import pytest

from tests import test_gpu_adjoint as ta
from tests import test_gpu_multiscale as tms

pytestmark = pytest.mark.gpu

W = 'wait_torch_stream'
SPARSE = ['rhsFromSparseDevice', W]                      # (rhsFromSparseDevice waits for its own uploads)

# per pipeline, the log of ONE work item of a 2-D operator.  'fixed' / 'relative': the receiver array; 'complex128' / 'complex64': the store
ORDER = {
    'dpred':                  SPARSE + ['solveDevice', 'sampleDevice'],
    'fields': {
        'complex128':         SPARSE + [W, 'solveDevice'],
        'complex64':          SPARSE + [W, 'solveDevice', 'packDevice']},
    'dpredFromFields':        [W, 'sampleDevice'],
    'bornFromFields':         [W, 'virtualSourcesDevice', 'solveDevice', 'sampleDevice'],
    'gradient': {
        'fixed':              SPARSE + [W, 'solveDevice', 'imagingAccumulateDevice'],
        'relative':           SPARSE + [W, 'rhsFromSamplesDevice', W, 'solveDevice', 'imagingAccumulateDevice']},
    'gradientFromFields': {
        'fixed':              SPARSE + [W, 'solveDevice', 'imagingAccumulateDevice'],
        'relative':           [W, 'rhsFromSamplesDevice', W, 'solveDevice', 'imagingAccumulateDevice']},
    'illumination':           SPARSE + [W, 'solveDevice', 'energyAccumulateDevice'],
    'illuminationFromFields': [W, 'energyAccumulateDevice'],
}
ORDER['transpose'] = ORDER['gradientFromFields']         # Jtvec(u=F, adjoint='transpose'): the same item body on the transposed operators

# MiniZephyr25D with nky = 2: the composite's method, then what it hands on to its ky operators
ORDER_25D = {
    'dpred':    ['rhsFromSparseDevice'] + SPARSE + ['sampleSumDevice', 'solveDevice', 'solveDevice'],
    'gradient': ['rhsFromSparseDevice'] + SPARSE + [W, 'solveDevice', 'solveDevice', 'solveDevice', 'imagingAccumulateDevice', 'imagingAccumulateDevice'],
}

# the multiscale pair: the up-scaled scaler is made on an item's first visit to its frequency (a wait and a grid transfer of its own), and
# every item ends in the grid transfer that adds its imaging sum to the gradient
ORDER_MULTISCALE = {
    'dpred':    SPARSE + ['solveDevice', 'sampleDevice'],
    'gradient': SPARSE + [W, 'apply_device', W, 'solveDevice', 'imagingAccumulateDevice', 'apply_device'],
}


def expected(table, name, mode, store):
    seq = table[name]
    if isinstance(seq, dict):
        seq = seq[mode] if mode in seq else seq[store]
    return seq


class Recorder(object):
    """Patches the operators' `*Device` methods, the grid transfer and `_lib.wait_torch_stream` to append their names to the log of the work item that is
    running on the calling thread, and `device_survey.runOnDevices` to open one log per item.  `runs`: per call of runOnDevices, a list of
    ((ifreq, c0, c1), thread, log) in the order the items finished."""

    def __init__(self, monkeypatch):
        from zephyr_amd import _lib, device_survey
        from zephyr_amd.discretization import BaseDiscretization
        from zephyr_amd.interpolation import SplineGridInterpolator
        from zephyr_amd.minizephyr import MiniZephyr, MiniZephyrHD, MiniZephyr25D
        self.runs = []
        self._here = threading.local()
        self._lock = threading.Lock()
        for cls in (BaseDiscretization, MiniZephyr, MiniZephyrHD, MiniZephyr25D):
            for name, fn in list(vars(cls).items()):
                if name.endswith('Device') and not name.startswith('_') and callable(fn):
                    monkeypatch.setattr(cls, name, self._logged(name, fn))
        monkeypatch.setattr(SplineGridInterpolator, 'apply_device', self._logged('apply_device', SplineGridInterpolator.apply_device))
        monkeypatch.setattr(_lib, 'wait_torch_stream', self._logged(W, _lib.wait_torch_stream))
        real_run = device_survey.runOnDevices

        def run(devs, items, fn, **kw):
            done = []
            self.runs.append(done)

            def item(ws, op, ifreq, c0, c1):
                self._here.log = log = []
                try:
                    return fn(ws, op, ifreq, c0, c1)
                finally:
                    self._here.log = None
                    with self._lock:
                        done.append(((ifreq, c0, c1), threading.get_ident(), log))
            return real_run(devs, items, item, **kw)
        monkeypatch.setattr(device_survey, 'runOnDevices', run)

    def _logged(self, name, fn):
        def wrapped(*a, **k):
            log = getattr(self._here, 'log', None)          # (None on the calling thread and on the prepare-ahead threads: not part of an item)
            if log is not None:
                log.append(name)
            return fn(*a, **k)
        return wrapped

    def take(self):
        'the one run since the last take()'
        assert len(self.runs) == 1, len(self.runs)
        return self.runs.pop()


def check(run, want_items, want_log, what):
    assert sorted(key for key, _, _ in run) == sorted(want_items), (what, [key for key, _, _ in run])
    for key, _, log in run:
        assert log == want_log, '%s, item %s:\n  recorded %s\n  expected %s' % (what, key, log, want_log)


LAYOUTS = {
    #               HELM_DEVICES  frequencies        items (ifreq, c0, c1)                                threads
    '0':           ('0',          None,              [(f, 0, ta.NSRC) for f in range(len(ta.FREQS))],    1),
    '0,0':         ('0,0',        None,              [(f, 0, ta.NSRC) for f in range(len(ta.FREQS))],    1),
    '0,0-1freq':   ('0,0',        [ta.FREQS[1]],     [(0, 0, 6), (0, 6, ta.NSRC)],                       2),
}


@pytest.mark.parametrize('store', ['complex128', 'complex64'])
@pytest.mark.parametrize('mode', ['fixed', 'relative'])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_every_pipeline_issues_its_library_calls_and_waits_in_the_recorded_order(helm_lib, monkeypatch, layout, mode, store):
    devices, freqs, items, nthreads = LAYOUTS[layout]
    monkeypatch.setenv('HELM_DEVICES', devices)
    extra = dict(fieldsDtype=store)
    if freqs is not None:
        extra.update(freqs=freqs, sterms=np.array([0.8 - 0.3j]))
    prob, sv = ta.device_pair(mode, **extra)
    assert prob._deviceGradientAvailable() and len(prob.system.devices) == len(devices.split(','))
    rng = np.random.default_rng(61)
    v, r = rng.standard_normal(prob.nrow), ta.randc(rng, sv.nD)
    rec = Recorder(monkeypatch)
    held = {}
    calls = [('dpred', lambda: sv.dpred()),
             ('gradient', lambda: prob.Jtvec(None, r)),
             ('illumination', lambda: prob.illumination()),
             ('fields', lambda: held.update(F=prob.fieldsDevice())),
             ('dpredFromFields', lambda: sv.dpred(u=held['F'])),
             ('bornFromFields', lambda: prob.JvecBorn(None, v, u=held['F'])),
             ('gradientFromFields', lambda: prob.Jtvec(None, r, u=held['F'])),
             ('illuminationFromFields', lambda: prob.illumination(u=held['F'])),
             ('transpose', lambda: prob.Jtvec(None, r, u=held['F'], adjoint='transpose'))]
    for name, call in calls:
        call()
        run = rec.take()
        check(run, items, expected(ORDER, name, mode, store), '%s (%s, %s, HELM_DEVICES=%s)' % (name, mode, store, devices))
        assert len(set(thread for _, thread, _ in run)) == nthreads, name
    assert held['F'].dtype == store
    held['F'].release()
    del prob.factors


def test_25d_composite_dpred_through_sample_sum_and_gradient(helm_lib, monkeypatch):
    import zephyr_amd as za
    monkeypatch.setenv('HELM_DEVICES', '0')
    sc = ta.ac.survey_config(ta.NZ, ta.NX, ta.NSRC, ta.NREC, ta.FREQS, 'fixed', nPML=8)
    sc.update(Disc=za.MiniZephyr25D, nky=2, rtol=1e-11)
    prob, sv = ta.ac.Helm25DProblem(sc), ta.ac.Helm25DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    r = ta.randc(np.random.default_rng(67), sv.nD)
    rec = Recorder(monkeypatch)
    items = [(f, 0, ta.NSRC) for f in range(len(ta.FREQS))]
    for name, call in (('dpred', lambda: sv.dpred()), ('gradient', lambda: prob.Jtvec(None, r))):
        call()
        check(rec.take(), items, ORDER_25D[name], '2.5-D ' + name)
    del prob.factors


def test_multiscale_dpred_and_gradient_through_the_upscaled_adding_step(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, _ = tms.pair()
    assert prob._deviceGradientAvailable()
    rng = np.random.default_rng(71)
    r = ta.randc(rng, sv.nD)
    rec = Recorder(monkeypatch)
    items = [(f, 0, sv.nsrc) for f in range(sv.nfreq)]
    for name, call in (('dpred', lambda: sv.dpred()), ('gradient', lambda: prob.Jtvec(v=r))):
        call()
        check(rec.take(), items, ORDER_MULTISCALE[name], 'multiscale ' + name)
    del prob.factors
