#!/usr/bin/env python3
"""What linearisation='full' costs beside 'operator' (parameter 'c' and 'rho'), with the forward fields in HBM, at config 4's survey: bench.py's 512^2
Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr.  Prints one JSON object and writes it
to --out (default profiles/full_bench.json).

Two problems live side by side in one process, each with its store F = fieldsDevice() and the factors of A and of A^T resident: one with an explicit density
(Gardner's formula evaluated once), one without `rho` (the density follows c).  Per store format (complex128, complex64), after a warm-up of each, the variants
alternate call by call:  ('operator', 'c'),  ('operator', 'rho'),  ('full', 'c') on the first problem and  ('full', 'c') on the second ('full_gardner'), for
JvecBorn(u=F),  Jtvec(u=F, adjoint='transpose')  and  Hvec(u=F).  The yardstick of every figure is the ('operator', 'c') figure of the same run.

Then the two new kernels alone beside k_buoyancy_planes / k_buoyancy_adjoint on assembled n^2 handles (--kernel-shapes, default 512 and 1024): wall time around
the call, launch and stream synchronisation included (`empty_call` is that overhead alone: the same entry point on a 3 x 3 handle).
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

VARIANTS = {'operator_c': ('rho', dict(linearisation='operator')), 'operator_rho': ('rho', dict(linearisation='operator', parameter='rho')),
            'full_c': ('rho', dict(linearisation='full')), 'full_gardner': ('gardner', dict(linearisation='full'))}


def routes(cfg, reps, dtype):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    c = np.asarray(cfg['c'])
    pairs = {}
    for name, extra in (('rho', dict(rho=310. * np.real(c) ** 0.25)), ('gardner', {})):
        sc = dict(cfg, Disc=za.MiniZephyr, fieldsDtype=dtype)
        sc.pop('rho', None)
        sc.update(extra)
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        pairs[name] = (prob, sv, prob.fieldsDevice())
    rng = np.random.default_rng(3)
    v = rng.standard_normal(pairs['rho'][0].nrow)
    d = pairs['rho'][1].dpred(u=pairs['rho'][2])
    r = (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) * np.abs(d).mean()
    times, res = {}, {}

    def clock(name, fn):
        t0 = time.perf_counter()
        out = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def one_round():
        for var, (which, kw) in VARIANTS.items():
            prob, _, F = pairs[which]
            res['Jv_' + var] = clock('born_' + var, lambda: prob.JvecBorn(None, v, u=F, **kw))
        for var, (which, kw) in VARIANTS.items():
            prob, _, F = pairs[which]
            res['g_' + var] = clock('jtvec_T_' + var, lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', **kw))
        for var, (which, kw) in VARIANTS.items():
            prob, _, F = pairs[which]
            clock('hvec_' + var, lambda: prob.Hvec(None, v, u=F, **kw))
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    for prob, _, F in pairs.values():
        F.release()
        del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    for what in ('born', 'jtvec_T', 'hvec'):
        for var in VARIANTS:
            if var != 'operator_c':
                out['%s_%s_over_operator_c' % (what, var)] = out['%s_%s' % (what, var)]['median_s'] / out[what + '_operator_c']['median_s']
    out['identity_miss'] = {}
    for var in VARIANTS:
        lhs = float(np.real(np.vdot(res['Jv_' + var], r)))
        out['identity_miss'][var] = abs(lhs - float(v @ res['g_' + var])) / abs(lhs)
    return out


def kernels(n, reps):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    rng = np.random.default_rng(5)
    model = lambda m: dict(nz=m, nx=m, dx=10., dz=10., nPML=min(10, m - 1), freq=6., c=rng.uniform(2000., 2600., (m, m)), rho=rng.uniform(1800., 2300., (m, m)), device=0)
    op, tiny = za.MiniZephyr(model(n)), za.MiniZephyr(model(3))
    h, ht = op.handle, tiny.handle
    dev = torch.device('cuda', 0)
    N = n * n
    gen = torch.Generator(device=dev).manual_seed(1)
    C9 = torch.view_as_complex(torch.randn((9, N, 2), dtype=torch.float64, device=dev, generator=gen))
    G = torch.zeros(N, dtype=torch.complex128, device=dev)
    DC, DB = (torch.randn(N, dtype=torch.float64, device=dev, generator=gen) for _ in range(2))
    torch.cuda.synchronize(dev)
    c9, g, dc, db = (P(t.data_ptr()) for t in (C9, G, DC, DB))

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts
    ck = lambda rc: _lib.check(rc, h)
    # bytes a call has to move: the nine planes written (planes) or read (adjoint) once, the model and the perturbations once
    calls = dict(
        buoyancy_planes=(lambda: ck(lib.helm_buoyancy_planes_device(h, db, c9)), (144 + 16 + 8) * N),
        velocity_planes=(lambda: ck(lib.helm_velocity_planes_device(h, dc, None, c9)), (144 + 16 + 8 + 8) * N),
        velocity_planes_db=(lambda: ck(lib.helm_velocity_planes_device(h, dc, db, c9)), (144 + 16 + 8 + 8 + 8) * N),
        buoyancy_adjoint=(lambda: ck(lib.helm_buoyancy_adjoint_device(h, c9, 1.0, 0.5, 1, g)), (144 + 16 + 32) * N),
        velocity_adjoint=(lambda: ck(lib.helm_velocity_adjoint_device(h, c9, 1.0, 0.5, 1, g)), (144 + 16 + 8 + 32) * N),
        empty_call=(lambda: _lib.check(lib.helm_velocity_adjoint_device(ht, c9, 1.0, 0.5, 1, g), ht), None))
    res = dict(n=n, reps=reps)
    for name, (fn, nbytes) in calls.items():
        s = stat(timed(fn))
        s['bytes'] = nbytes
        if nbytes:
            s['TBps'] = nbytes / s['median_s'] / 1e12
        res[name] = s
    res['velocity_planes_over_buoyancy_planes'] = res['velocity_planes']['median_s'] / res['buoyancy_planes']['median_s']
    res['velocity_planes_db_over_buoyancy_planes'] = res['velocity_planes_db']['median_s'] / res['buoyancy_planes']['median_s']
    res['velocity_adjoint_over_buoyancy_adjoint'] = res['velocity_adjoint']['median_s'] / res['buoyancy_adjoint']['median_s']
    del op.factors, tiny.factors
    del C9, G
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
    ap.add_argument('--kernel-shapes', default='512,1024', help='n of the kernel timings, comma separated')
    ap.add_argument('--formats', default='complex128,complex64')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'full_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps, disc='MiniZephyr', kernels=[], routes={})
    for n in args.kernel_shapes.split(','):
        res['kernels'].append(kernels(int(n), args.kernel_reps))
        print(json.dumps({'kernels': res['kernels'][-1]}, default=float), flush=True)
    for dtype in args.formats.split(','):
        res['routes'][dtype] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps, dtype)
        print(json.dumps({'routes_' + dtype: res['routes'][dtype]}, default=float), flush=True)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
