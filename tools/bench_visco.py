#!/usr/bin/env python3
"""What the exact velocity and Q derivatives of a visco problem cost, with the forward fields in HBM, at config 4's survey as a visco problem: bench.py's 512^2
Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr, an explicit density (Gardner's formula
evaluated once), Q from a smooth map (40 .. 120) and freqBase = 5 Hz.  Prints one JSON object and writes it to --out (default profiles/visco_bench.json).

Routes.  The visco problem and, beside it, the NON-visco problem on the same model, each with its store F = fieldsDevice() and the factors of A and A^T resident.
After a warm-up of each, the calls alternate one by one, `reps` rounds, all in one run:

  visco/<lin>/jtvec_c, _Q, _cQ            Jtvec(u=F, adjoint='transpose', parameter=): one back-solve and one imaging pass per item whatever the parameter
  visco/<lin>/born_c, _Q, _cQ             JvecBorn(u=F, parameter=): one Born solve per item
  visco/<lin>/hvec_c, _Q, _cQ             Hvec(u=F, parameter=): two solves per item
  plain/<lin>/jtvec_c, born_c, hvec_c     the same calls of the non-visco problem

for linearisation='full' and 'operator' and for both formats of the store.  The supposition: a 'cQ' call takes about what the non-visco 'c' call takes (the same
solves, three N-sized launches more per item), and the two single-parameter calls it replaces take 2x.

Kernels, on an assembled n^2 handle (wall time around the call, launch and stream synchronisation included; `empty_call` is that overhead alone, the same entry point on
a 3 x 3 handle): k_visco_perturbation, k_velocity_planes_z and k_visco_chain_adjoint beside k_velocity_planes and k_velocity_adjoint.

Per figure: the median, every time and the run-to-run spread (max - min) / median.  Nothing here was tuned.
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

PARAMETERS = ('c', 'Q', 'cQ')


def smooth_q(n):
    'a smooth map of Q in 40 .. 120 on the n x n grid'
    z, x = np.meshgrid(np.linspace(0., 1., n), np.linspace(0., 1., n), indexing='ij')
    return 80. + 40. * np.sin(2. * np.pi * x) * np.cos(np.pi * z)


def routes(cfg, reps, dtype):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = dict(cfg, Disc=za.MiniZephyr, fieldsDtype=dtype)
    sc['rho'] = 310. * np.real(np.asarray(cfg['c'])) ** 0.25
    n = int(sc['nz'])
    probs = {}
    creal = np.ascontiguousarray(np.real(np.asarray(cfg['c'])))          # (the visco wrapper takes the real velocity; the model has no imaginary part)
    for name, Problem, extra in (('visco', Helm2DViscoProblem, dict(c=creal, Q=smooth_q(n), freqBase=5., viscoDerivatives=True)), ('plain', Helm2DProblem, {})):
        scp = dict(sc, **extra)
        prob, sv = Problem(scp), Helm2DSurvey(scp)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        probs[name] = (prob, sv, prob.fieldsDevice())
    N = probs['visco'][0].nrow
    rng = np.random.default_rng(3)
    nD = probs['visco'][1].nD
    r = rng.standard_normal(nD) + 1j * rng.standard_normal(nD)
    v = np.concatenate((50. * rng.uniform(-1., 1., N), 2. * rng.uniform(-1., 1., N)))
    vec = {'c': v[:N].copy(), 'Q': v[N:].copy(), 'cQ': v}
    calls = {}
    for lin in ('full', 'operator'):
        for name, pars in (('visco', PARAMETERS), ('plain', ('c',))):
            prob, sv, F = probs[name]
            for par in pars:
                kw = dict(u=F, linearisation=lin, parameter=par)
                calls['%s/%s/jtvec_%s' % (name, lin, par)] = lambda prob=prob, kw=kw: prob.Jtvec(None, r, adjoint='transpose', **kw)
                calls['%s/%s/born_%s' % (name, lin, par)] = lambda prob=prob, kw=kw, par=par: prob.JvecBorn(None, vec[par], **kw)
                calls['%s/%s/hvec_%s' % (name, lin, par)] = lambda prob=prob, kw=kw, par=par: prob.Hvec(None, vec[par], **kw)
    times, res = {}, {}

    def one_round():
        for name, fn in calls.items():
            t0 = time.perf_counter()
            res[name] = fn()
            times.setdefault(name, []).append(time.perf_counter() - t0)
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    for prob, sv, F in probs.values():
        F.release()
        del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    med = lambda name: out[name]['median_s']
    for lin in ('full', 'operator'):
        for what in ('jtvec', 'born', 'hvec'):
            k = lambda name, par: '%s/%s/%s_%s' % (name, lin, what, par)
            out['%s/%s_cQ_over_plain_c' % (lin, what)] = med(k('visco', 'cQ')) / med(k('plain', 'c'))
            out['%s/%s_c_over_plain_c' % (lin, what)] = med(k('visco', 'c')) / med(k('plain', 'c'))
            out['%s/%s_two_calls_over_cQ' % (lin, what)] = (med(k('visco', 'c')) + med(k('visco', 'Q'))) / med(k('visco', 'cQ'))
        # what the run computed: the stacked gradient against the two single-parameter calls
        g2 = np.concatenate((res['visco/%s/jtvec_c' % lin], res['visco/%s/jtvec_Q' % lin]))
        out['%s/jtvec_cQ_against_two_calls' % lin] = float(np.linalg.norm(res['visco/%s/jtvec_cQ' % lin] - g2) / np.linalg.norm(g2))
        b2 = res['visco/%s/born_c' % lin] + res['visco/%s/born_Q' % lin]
        out['%s/born_cQ_against_two_calls' % lin] = float(np.linalg.norm(res['visco/%s/born_cQ' % lin] - b2) / np.linalg.norm(b2))
    return out


def kernels(n, reps):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    rng = np.random.default_rng(5)

    def model(m):
        c, Q = rng.uniform(2000., 2600., (m, m)), rng.uniform(40., 120., (m, m))
        return dict(nz=m, nx=m, dx=10., dz=10., nPML=min(10, m - 1), freq=6., c=c * (1. + 0.058 / Q) * (1. + 0.5j / Q), rho=rng.uniform(1800., 2300., (m, m)), device=0)
    op, tiny = za.MiniZephyr(model(n)), za.MiniZephyr(model(3))
    h, ht = op.handle, tiny.handle
    dev = torch.device('cuda', 0)
    N = n * n
    gen = torch.Generator(device=dev).manual_seed(1)
    V = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 0.5
    W = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 0.5
    Q = 40. + 80. * torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    G = torch.zeros(2 * N, dtype=torch.complex128, device=dev)
    Z = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float64, device=dev, generator=gen))
    C9 = torch.view_as_complex(torch.randn((9 * N, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    v, w, q, g, z, c9 = (P(t.data_ptr()) for t in (V, W, Q, G, Z, C9))
    gq = P(G.data_ptr() + 16 * N)
    ck = lambda rc, hd=h: _lib.check(rc, hd)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts
    calls = dict(
        empty_call=lambda: ck(lib.helm_visco_chain_adjoint_device(ht, q, 0.058, c9, 1, g, None), ht),
        visco_perturbation=lambda: ck(lib.helm_visco_perturbation_device(h, q, 0.058, v, w, z)),
        velocity_planes_z=lambda: ck(lib.helm_velocity_planes_z_device(h, z, c9)),
        visco_chain_adjoint=lambda: ck(lib.helm_visco_chain_adjoint_device(h, q, 0.058, z, 1, g, gq)),
        velocity_planes=lambda: ck(lib.helm_velocity_planes_device(h, v, None, c9)),
        velocity_adjoint=lambda: ck(lib.helm_velocity_adjoint_device(h, c9, 1.0, 0.5, 1, g)))
    res = dict(n=n, reps=reps)
    for name, fn in calls.items():
        res[name] = stat(timed(fn))
    res['velocity_planes_z_over_velocity_planes'] = res['velocity_planes_z']['median_s'] / res['velocity_planes']['median_s']
    del op.factors, tiny.factors
    del C9
    torch.cuda.empty_cache()
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visco_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['kernels'] = kernels(args.n, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    cfg = job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec)
    res['routes'] = {}
    for dt in ('complex128', 'complex64'):
        res['routes'][dt] = routes(cfg, args.reps, dt)
        print(json.dumps({dt: res['routes'][dt]}, default=float), flush=True)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
