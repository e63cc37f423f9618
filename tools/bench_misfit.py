#!/usr/bin/env python3
"""What DataMisfit.valueAndGradient costs against the calls it is made of, at config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m), 8 frequencies
3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr, an explicit density, the factors of A and A^T resident.  Prints one JSON object and
writes it to --out (default profiles/misfit_bench.json).

Routes.  After a warm-up of each, the calls alternate one by one, `reps` rounds, all in one run:

  jtvec_full                Jtvec(u=F, adjoint='transpose', linearisation='full') with a host residual: what a gradient cost before
  misfit_store              valueAndGradient(u=F), the data kept on the device (supposition (a): within a few percent of jtvec_full)
  misfit_store_host_data    the same with misfitHostData=True: dpred(u=F) down, numpy, the adjoint source up (supposition (c): NOT measurably slower)
  fields                    fieldsDevice() and its release
  misfit_one_pass           valueAndGradient(u=None), source='perSource': no store (supposition (b): fields + jtvec_full)
  misfit_internal_store     valueAndGradient(u=None) of a per-frequency estimate whose group spans items -- only where the deal splits a frequency; else absent

with the peak of torch's device memory over each call and the bytes the library's pool allocated anew during it.

Kernels, on (nrec, nsrc) panels (wall time around the call, launch and stream synchronisation included; `empty_call` is that overhead alone, the moments entry
point on a 1 x 1 panel): the three entry points for every kind.

Per figure: the median, every time and the run-to-run spread (max - min) / median."""
import argparse
import ctypes
import json
import os
import sys
import time

for _k in ('OPENBLAS_NUM_THREADS', 'OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(_k, '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.bench_fields import job_config, stat


def routes(cfg, reps):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib, device_survey
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = dict(cfg, Disc=za.MiniZephyr)
    sc['rho'] = 310. * np.real(np.asarray(cfg['c'])) ** 0.25
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    dev = torch.device('cuda', prob.system.subProblems[0].device)
    rng = np.random.default_rng(3)
    shape = (sv.nrec, sv.nsrc, sv.nfreq)
    p = sv.dpred().reshape(shape)
    rms = np.sqrt(np.mean(np.abs(p) ** 2))
    dobs = (1.3 - 0.4j) * p + 0.05 * rms * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    r = (p - dobs).ravel()
    F = prob.fieldsDevice()
    phi = za.DataMisfit(prob, dobs, kind='l2', source='perSource')
    per_freq = za.DataMisfit(prob, dobs, kind='l2', source='perFrequency')
    items = device_survey.deviceItems(prob.system, prob.ownedFreqs, sv.nsrc)[1]

    def host_data():
        prob._misfitHostData = True
        try:
            return phi.valueAndGradient(None, u=F)
        finally:
            prob._misfitHostData = False

    def fields():
        F2 = prob.fieldsDevice()
        F2.release()
    calls = {'jtvec_full': lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full'),
             'misfit_store': lambda: phi.valueAndGradient(None, u=F),
             'misfit_store_host_data': host_data,
             'fields': fields,
             'misfit_one_pass': lambda: phi.valueAndGradient(None)}
    if not device_survey.misfitInOnePass(per_freq, items):
        calls['misfit_internal_store'] = lambda: per_freq.valueAndGradient(None)
    times, peak, pool, res = {}, {}, {}, {}

    def one_round():
        for name, fn in calls.items():
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            _lib.runtime_stats(reset=True)
            t0 = time.perf_counter()
            res[name] = fn()
            times.setdefault(name, []).append(time.perf_counter() - t0)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated(dev) - base)
            pool[name] = max(pool.get(name, 0.), _lib.runtime_stats()['dev_alloc_bytes'])
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    store_bytes = sum(sl.numel() * sl.element_size() for sl, _ in F._store.values())
    F.release()
    del prob.factors
    out = {name: dict(stat(ts), torch_peak_bytes_over_call=int(peak[name]), pool_bytes_allocated_in_call=float(pool[name])) for name, ts in times.items()}
    med = lambda name: out[name]['median_s']
    out['store_bytes'] = store_bytes
    out['items'] = len(items)
    out['misfit_store_over_jtvec_full'] = med('misfit_store') / med('jtvec_full')
    out['misfit_store_over_host_data'] = med('misfit_store') / med('misfit_store_host_data')
    out['misfit_one_pass_over_fields_plus_jtvec'] = med('misfit_one_pass') / (med('fields') + med('jtvec_full'))
    g, gh, g1 = res['misfit_store'][1], res['misfit_store_host_data'][1], res['misfit_one_pass'][1]
    out['store_against_host_data'] = float(np.linalg.norm(g - gh) / np.linalg.norm(gh))
    out['one_pass_same_bits_as_store'] = bool(np.array_equal(g, g1) and res['misfit_store'][0] == res['misfit_one_pass'][0])
    return out


def kernels(nrec, ncol, reps):
    import torch
    from zephyr_amd import _lib, device_survey
    lib = _lib.load()
    h = lib.helm_create(0, _lib.HELM_MINIZEPHYR, 8, 8, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))

    class Op(object):
        handle = h
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    cplx = lambda *s: torch.view_as_complex(torch.randn(s + (2,), dtype=torch.float64, device=dev, generator=gen))
    P, D, PSI = cplx(nrec, ncol), cplx(nrec, ncol), cplx(nrec, ncol)
    W = torch.rand((nrec, ncol), dtype=torch.float64, device=dev, generator=gen) + 0.5
    P1, D1 = cplx(1, 1), cplx(1, 1)
    s = np.ones(ncol, dtype=np.complex128) * (1.2 - 0.3j)
    coef = np.full((ncol, 3), 0.1)
    torch.cuda.synchronize(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts
    res = dict(nrec=nrec, ncol=ncol, reps=reps, panel_bytes=16 * nrec * ncol)
    res['empty_call'] = stat(timed(lambda: device_survey.misfitMomentsDevice(Op, P1, D1, None)))
    res['moments'] = stat(timed(lambda: device_survey.misfitMomentsDevice(Op, P, D, W)))
    for kind, code in device_survey.MISFIT_KINDS.items():
        par = (0.5, 0.5)
        res['terms_' + kind] = stat(timed(lambda: device_survey.misfitTermsDevice(Op, code, par, P, D, W, s, PSI)))
        V = torch.empty_like(P)
        res['adjoint_' + kind] = stat(timed(lambda: device_survey.misfitAdjointDevice(Op, code, par, PSI, s, coef, P, D, W, None, V)))
    lib.helm_destroy(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'misfit_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['kernels'] = kernels(args.nrec, args.nsrc, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    res['routes'] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
