#!/usr/bin/env python3
"""What parameter='rho' costs beside parameter='c' (both linearisation='operator'), with the forward fields in HBM, at config 4's survey: bench.py's 512^2
Marmousi-like model (dx = 10 m) with an explicit density (Gardner's formula evaluated once), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128
receivers, one GPU, MiniZephyr.  Prints one JSON object and writes it to --out (default profiles/density_bench.json).

Routes, per store format (complex128, complex64), on one store F = fieldsDevice() with the factors of A and of A^T resident, the two parameters alternating
call by call in one process after a warm-up of each:  JvecBorn(u=F),  Jtvec(u=F, adjoint='transpose'),  Hvec(u=F).  The yardstick of every 'rho' figure is
the 'c' figure of the same run.

Then the kernels alone, wall time around the call (launch and stream synchronisation included; `empty_call` is that overhead alone), against a
device-to-device copy of a complex128 buffer measured the same way in the same process: helm_stencil_sources[_c64]_device beside
helm_virtual_sources_op[_c64]_device and helm_lag_imaging_accumulate[_c64]_device beside helm_imaging_op_accumulate[_c64]_device, on nsrc columns of n^2
cells (--kernel-shapes, default 512x64 and 1024x256).
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

PARS = ('c', 'rho')


def routes(cfg, reps, dtype):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    c = np.asarray(cfg['c'])
    sc = dict(cfg, Disc=za.MiniZephyr, rho=310. * np.real(c) ** 0.25, fieldsDtype=dtype)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    rng = np.random.default_rng(3)
    v = rng.standard_normal(prob.nrow)
    times, res = {}, {}
    kw = dict(linearisation='operator')

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    F = prob.fieldsDevice()
    d = sv.dpred(u=F)
    r = (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) * np.abs(d).mean()

    def one_round():
        for par in PARS:
            res['Jv_' + par] = clock('born_' + par, lambda: prob.JvecBorn(None, v, u=F, parameter=par, **kw))
        for par in PARS:
            res['g_' + par] = clock('jtvec_T_' + par, lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', parameter=par, **kw))
        for par in PARS:
            clock('hvec_' + par, lambda: prob.Hvec(None, v, u=F, parameter=par, **kw))
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    F.release()
    del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    for what in ('born', 'jtvec_T', 'hvec'):
        out[what + '_rho_over_c'] = out[what + '_rho']['median_s'] / out[what + '_c']['median_s']
    out['identity_miss'] = {}
    for par in PARS:
        lhs = float(np.real(np.vdot(res['Jv_' + par], r)))
        out['identity_miss'][par] = abs(lhs - float(v @ res['g_' + par])) / abs(lhs)
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
    gen = torch.Generator(device=dev).manual_seed(1)
    cplx = lambda *shape: torch.view_as_complex(torch.randn(shape + (2,), dtype=torch.float64, device=dev, generator=gen))
    U, B, W, G, C9 = cplx(nsrc, N), cplx(nsrc, N), cplx(N), cplx(N), cplx(9, N)
    R = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    X = torch.empty(nsrc, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(X.data_ptr())), h)
    u, b, w, g, rr, p64, x, c9 = (P(t.data_ptr()) for t in (U, B, W, G, R, P64, X, C9))

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
    ck = lambda rc: _lib.check(rc, h)
    groups = (nsrc + 3) // 4
    # bytes a call has to move: the fields once; the nine planes once per group of four columns (stencil sources), read and written once (lag imaging)
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        virtual_sources_op_c128=(lambda: ck(lib.helm_virtual_sources_op_device(h, u, nsrc, N, w, -1.0, 0.0, 1, rr, N)), 32 * nsrc * N + 16 * N),
        stencil_sources_c128=(lambda: ck(lib.helm_stencil_sources_device(h, u, nsrc, N, c9, -1.0, 0.0, 1, rr, N)), 32 * nsrc * N + 144 * N * groups),
        virtual_sources_op_c64=(lambda: ck(lib.helm_virtual_sources_op_c64_device(h, p64, x, nsrc, N, w, -1.0, 0.0, 1, rr, N)), 24 * nsrc * N + 16 * N),
        stencil_sources_c64=(lambda: ck(lib.helm_stencil_sources_c64_device(h, p64, x, nsrc, N, c9, -1.0, 0.0, 1, rr, N)), 24 * nsrc * N + 144 * N * groups),
        imaging_op_c128=(lambda: ck(lib.helm_imaging_op_accumulate_device(h, u, N, b, N, nsrc, w, g)), 32 * nsrc * N + 48 * N),
        lag_imaging_c128=(lambda: ck(lib.helm_lag_imaging_accumulate_device(h, u, N, b, N, nsrc, c9)), 32 * nsrc * N + 288 * N),
        imaging_op_c64=(lambda: ck(lib.helm_imaging_op_accumulate_c64_device(h, p64, x, N, b, N, nsrc, w, g)), 24 * nsrc * N + 48 * N),
        lag_imaging_c64=(lambda: ck(lib.helm_lag_imaging_accumulate_c64_device(h, p64, x, N, b, N, nsrc, c9)), 24 * nsrc * N + 288 * N),
        empty_call=(lambda: _lib.check(lib.helm_virtual_sources_op_device(tiny, u, 1, 9, w, 1.0, 0.0, 0, rr, 9), tiny), None))
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        s = stat(timed(fn))
        s['bytes'] = nbytes
        if nbytes:
            s['TBps'] = nbytes / s['median_s'] / 1e12
            s['rate_over_copy'] = s['TBps'] / res['copy_c128']['TBps'] if name != 'copy_c128' else 1.0
        res[name] = s
    for fmt in ('c128', 'c64'):
        res['stencil_sources_over_virtual_sources_op_' + fmt] = res['stencil_sources_' + fmt]['median_s'] / res['virtual_sources_op_' + fmt]['median_s']
        res['lag_imaging_over_imaging_op_' + fmt] = res['lag_imaging_' + fmt]['median_s'] / res['imaging_op_' + fmt]['median_s']
    lib.helm_destroy(h)
    lib.helm_destroy(tiny)
    del U, B, R, P64, C9
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
    ap.add_argument('--kernel-shapes', default='512x64,1024x256', help='n x nsrc of the kernel timings, comma separated')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'density_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps, disc='MiniZephyr', kernels=[], routes={})
    for shape in args.kernel_shapes.split(','):
        n, nsrc = (int(t) for t in shape.split('x'))
        res['kernels'].append(kernels(n, nsrc, args.kernel_reps))
        print(json.dumps({'kernels': res['kernels'][-1]}, default=float), flush=True)
    for dtype in ('complex128', 'complex64'):
        res['routes'][dtype] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps, dtype)
        print(json.dumps({'routes_' + dtype: res['routes'][dtype]}, default=float), flush=True)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
