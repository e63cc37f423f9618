#!/usr/bin/env python3
"""What the exact adjoint, the Born data and the Gauss-Newton product cost with the forward fields in HBM, at config 4's survey: bench.py's 512^2
Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU -- with MiniZephyr in the place of
config 4's Eurus, which has no transposed operator.  Prints one JSON object and writes it to --out (default profiles/adjoint_bench.json).

Routes, alternating run by run in one process after a warm-up of each, on one store F = fieldsDevice() per round (its time is reported for scale):

  jtvec_F:            Jtvec(u=F), the back-propagation through the forward factors, which the store's solve has left resident
  jtvec_T_fresh:      Jtvec(u=F, adjoint='transpose') with no factors of A^T: the eight extra factorisations are inside (started one item ahead by the
                      pipeline's prepare thread)
  jtvec_T_resident:   the same call again: the factors of A^T are resident.  fresh - resident is what the factorisations cost after the pipeline has
                      hidden what it can; factor_T_serial is what they cost back to back with nothing to hide behind (prefactor + a one-column solve each)
  born_F:             JvecBorn(u=F)
  hvec_F:             Hvec(u=F) with both sets of factors resident, beside born_F + jtvec_T_resident

Then the two new kernels alone, wall time around the call (launch and stream synchronisation included; `empty_call` is that overhead alone), against a
device-to-device copy of a complex128 buffer measured the same way in the same process: k_transpose_planes through helm_assemble with the flag on minus the
same call with the flag off (the assembly kernel is common to both), and helm_virtual_sources[_c64]_device on nsrc columns of n^2 cells.
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


def routes(cfg, reps):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = dict(cfg, Disc=za.MiniZephyr)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    rng = np.random.default_rng(3)
    v = rng.standard_normal(prob.nrow)
    times, res = {}, {}

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def factor_T_serial():
        q = np.zeros((prob.nrow, 1), dtype=np.complex128)
        q[prob.nrow // 2] = 1.
        for sub in prob.adjointSystem.subProblems:
            sub * q

    def one_round():
        del prob.factors
        F = clock('fields', prob.fieldsDevice)
        if 'r' not in res:
            d = sv.dpred(u=F)
            res['r'] = (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) * np.abs(d).mean()
        r = res['r']
        res['g'] = clock('jtvec_F', lambda: prob.Jtvec(None, r, u=F))
        res['gT'] = clock('jtvec_T_fresh', lambda: prob.Jtvec(None, r, u=F, adjoint='transpose'))
        clock('jtvec_T_resident', lambda: prob.Jtvec(None, r, u=F, adjoint='transpose'))
        res['Jv'] = clock('born_F', lambda: prob.JvecBorn(None, v, u=F))
        res['Hv'] = clock('hvec_F', lambda: prob.Hvec(None, v, u=F))
        del prob.adjointSystem.factors
        clock('factor_T_serial', factor_T_serial)
        F.release()
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    med = lambda k: out[k]['median_s']
    lhs = float(np.real(np.vdot(res['Jv'], res['r'])))
    out['identity_miss'] = dict(transpose=abs(lhs - float(v @ res['gT'])) / abs(lhs), reciprocity=abs(lhs - float(v @ res['g'])) / abs(lhs))
    out['extra_factorisations_s'] = med('jtvec_T_fresh') - med('jtvec_T_resident')
    out['hidden_fraction_of_serial_factorisations'] = 1.0 - out['extra_factorisations_s'] / med('factor_T_serial')
    out['hvec_over_sum_of_halves'] = med('hvec_F') / (med('born_F') + med('jtvec_T_resident'))
    out['hvec_over_two_jtvec_F'] = med('hvec_F') / (2 * med('jtvec_F'))
    return out


def kernels(n, nsrc, reps):
    import torch
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    h = lib.helm_create(0, 0, n, n, 10., 10., 10, None)
    tiny = lib.helm_create(0, 0, 3, 3, 10., 10., 2, None)
    assert h and tiny
    dev = torch.device('cuda', 0)
    N = n * n
    c = np.full(N, 2500. + 25j, dtype=np.complex128)
    _lib.check(lib.helm_set_model(h, _lib.ptr(c), None, None, None, None), h)
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    R = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    X = torch.empty(nsrc, dtype=torch.int32, device=dev)
    W = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float64, device=dev, generator=gen))
    planes, planes2 = torch.empty(9 * N, dtype=torch.complex128, device=dev), torch.empty(9 * N, dtype=torch.complex128, device=dev)
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
        R.copy_(U)
        torch.cuda.synchronize(dev)

    def copy_planes():
        planes2.copy_(planes)
        torch.cuda.synchronize(dev)

    def assemble(on):
        def fn():
            _lib.check(lib.helm_set_transposed(h, on), h)
            _lib.check(lib.helm_assemble(h, 8.0, 0.0, float('inf'), 0.0, 0.0), h)
        return fn
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        virtual_sources_c128=(lambda: _lib.check(lib.helm_virtual_sources_device(h, P(U.data_ptr()), nsrc, N, P(W.data_ptr()), P(R.data_ptr()), N), h), 32 * nsrc * N + 16 * N),
        virtual_sources_c64=(lambda: _lib.check(lib.helm_virtual_sources_c64_device(h, P(P64.data_ptr()), P(X.data_ptr()), nsrc, N, P(W.data_ptr()), P(R.data_ptr()), N), h),
                             24 * nsrc * N + 16 * N),
        empty_call=(lambda: _lib.check(lib.helm_virtual_sources_device(tiny, P(U.data_ptr()), 1, 9, P(W.data_ptr()), P(R.data_ptr()), 9), tiny), None),
        copy_planes=(copy_planes, 2 * 9 * 16 * N),
        assemble_plain=(assemble(0), None),
        assemble_transposed=(assemble(1), None))
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        r = stat(timed(fn))
        r['bytes'] = nbytes
        if nbytes:
            r['TBps'] = nbytes / r['median_s'] / 1e12
        res[name] = r
    for name in ('virtual_sources_c128', 'virtual_sources_c64'):
        res[name]['rate_over_copy'] = res[name]['TBps'] / res['copy_c128']['TBps']
    dt = res['assemble_transposed']['median_s'] - res['assemble_plain']['median_s']
    res['transpose_planes'] = dict(extra_s=dt, bytes=2 * 9 * 16 * N, TBps=2 * 9 * 16 * N / max(dt, 1e-9) / 1e12)
    res['transpose_planes']['rate_over_copy'] = res['transpose_planes']['TBps'] / res['copy_planes']['TBps']
    lib.helm_destroy(h)
    lib.helm_destroy(tiny)
    del U, R, P64, planes, planes2
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adjoint_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps, disc='MiniZephyr')
    res['kernels'] = kernels(args.n, args.nsrc, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    res['routes'] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
