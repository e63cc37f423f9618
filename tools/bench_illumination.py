#!/usr/bin/env python3
"""What the illumination / diagonal pseudo-Hessian costs with the wavefields in HBM, at config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m),
Eurus, 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU.  Prints one JSON object and writes it to --out (default
profiles/illumination_bench.json).

Routes, alternating run by run in one process after a warm-up of each; the ones that solve start from fresh factors (del prob.factors before, none inside):

  fields128 / fields64:   F = fieldsDevice() alone, for scale (the store complex128 / complex64)
  illum_F128 / illum_F64: illumination(u=F) on a store that is already there: no solve, one kernel per frequency, 8 N bytes down
  illum_solve:            illumination(): nsrc columns per frequency solved into HBM, accumulated and dropped
  illum_receiver:         illumination(side='receiver'): the same with the 128 receivers as sources
  host_fields:            u = prob.fields(), then sum_f |scaler_f|^2 sum_s |u_f|^2 in numpy -- the only route before this method existed: every wavefield
                          crosses PCIe

Per route: the median, every time, and the run-to-run spread (max - min) / median.  Then the two energy kernels alone on nsrc columns of n^2 cells, at the
survey's size and at 256 columns of 1024^2 cells: wall time around the call (it returns when E is complete, so launch and stream synchronisation are
included; `empty_call` is that overhead alone, a launch on 9 cells), the bytes each has to move, and the rate against a device-to-device copy of the same
complex128 buffer measured the same way in the same process.
"""
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


def host_route(prob):
    u = prob.fields()
    H = np.zeros(prob.nrow)
    for ifreq, uf in enumerate(u):
        w = prob.gradientScaler(ifreq)
        H += (np.square(w.real) + np.square(w.imag)) * np.add.reduce(np.square(uf.real) + np.square(uf.imag), axis=1)
    return H


def routes(cfg, reps):
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    pairs = {}
    for dt in ('complex128', 'complex64'):
        sc = dict(cfg, fieldsDtype=dt)
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        pairs[dt] = prob
    p128, p64 = pairs['complex128'], pairs['complex64']
    times, res = {}, {}

    def clock(name, fn, fresh=None):
        if fresh is not None:
            del fresh.factors
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def one_round():
        F128 = clock('fields128', p128.fieldsDevice, fresh=p128)
        res['F128'] = clock('illum_F128', lambda: p128.illumination(u=F128))
        res['F128_energy'] = clock('illum_F128_energy', lambda: p128.illumination(u=F128, kind='energy'))
        F128.release()
        F64 = clock('fields64', p64.fieldsDevice, fresh=p64)
        res['F64'] = clock('illum_F64', lambda: p64.illumination(u=F64))
        F64.release()
        res['solve'] = clock('illum_solve', p128.illumination, fresh=p128)
        res['receiver'] = clock('illum_receiver', lambda: p128.illumination(side='receiver'), fresh=p128)
        res['host'] = clock('host_fields', lambda: host_route(p128), fresh=p128)
    one_round()                                               # (warm: plans, pools, first launches, the survey's cached matrices)
    times.clear()
    for _ in range(reps):
        one_round()
    del p128.factors, p64.factors
    nrm = np.linalg.norm
    out = {name: stat(ts) for name, ts in times.items()}
    out['agreement'] = dict(F128_vs_host=float(nrm(res['F128'] - res['host']) / nrm(res['host'])),
                            solve_vs_F128_bit_identical=bool(np.array_equal(res['solve'], res['F128'])),
                            F64_vs_F128=float(nrm(res['F64'] - res['F128']) / nrm(res['F128'])))
    N = p128.nrow
    out['bytes_down'] = dict(illum=8 * N, host_fields=16 * N * len(cfg['freqs']) * cfg['geom']['src'].shape[0])
    out['host_over_illum_solve'] = out['host_fields']['median_s'] / out['illum_solve']['median_s']
    out['illum_F128_over_fields128'] = out['illum_F128']['median_s'] / out['fields128']['median_s']
    return out


def kernels(n, nsrc, reps):
    'the two energy kernels on nsrc columns of n^2 cells against a device-to-device copy of the complex128 columns, all timed the same way'
    import torch
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    h = lib.helm_create(0, 0, n, n, 10., 10., 10, None)
    tiny = lib.helm_create(0, 0, 3, 3, 10., 10., 1, None)
    assert h and tiny
    dev = torch.device('cuda', 0)
    N = n * n
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    U2 = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    X = torch.empty(nsrc, dtype=torch.int32, device=dev)
    W = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    E = torch.zeros(N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(X.data_ptr())), h)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts

    def copy():
        U2.copy_(U)
        torch.cuda.synchronize(dev)
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        energy_c128=(lambda: _lib.check(lib.helm_energy_accumulate_device(h, P(U.data_ptr()), nsrc, N, 0.5, P(W.data_ptr()), P(E.data_ptr())), h), 16 * nsrc * N + 24 * N),
        energy_c64=(lambda: _lib.check(lib.helm_energy_accumulate_c64_device(h, P(P64.data_ptr()), P(X.data_ptr()), nsrc, N, 0.5, P(W.data_ptr()), P(E.data_ptr())), h),
                    8 * nsrc * N + 24 * N),
        empty_call=(lambda: _lib.check(lib.helm_energy_accumulate_device(tiny, P(U.data_ptr()), 1, 9, 0.5, None, P(E.data_ptr())), tiny), None))
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        r = stat(timed(fn))
        r['bytes'] = nbytes
        if nbytes:
            r['TBps'] = nbytes / r['median_s'] / 1e12
        res[name] = r
    over = res['empty_call']['median_s']
    for name in ('energy_c128', 'energy_c64'):
        res[name]['rate_over_copy'] = res[name]['TBps'] / res['copy_c128']['TBps']
        res[name]['TBps_without_call_overhead'] = res[name]['bytes'] / max(res[name]['median_s'] - over, 1e-9) / 1e12
    lib.helm_destroy(h)
    lib.helm_destroy(tiny)
    del U, U2, P64
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'illumination_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['kernels'] = [kernels(args.n, args.nsrc, args.kernel_reps), kernels(1024, 256, args.kernel_reps)]
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    res['routes'] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
