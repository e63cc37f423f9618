#!/usr/bin/env python3
"""What the exact adjoint and the exact derivatives of an Eurus problem (config key eurusDerivatives, eps == delta) cost with the forward fields in HBM, at config 4's
survey as an Eurus problem: bench.py's 512^2 Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, an
explicit density (Gardner's formula evaluated once) and a tilted elliptical anisotropy (smooth eps == delta in 0.05 .. 0.15, theta in -0.4 .. 0.4).  Prints one JSON
object and writes it to --out (default profiles/eurus_bench.json).

Routes.  The Eurus problem and, beside it, the MiniZephyr problem on the same c and rho, each with its store F = fieldsDevice() and the factors of its operator and of
the transposed one resident.  After a warm-up of each, the calls alternate one by one, `reps` rounds, all in one run:

  eurus/jtvec_c, _rho, _joint       Jtvec(u=F, adjoint='transpose', linearisation='full', parameter=)
  eurus/born_*, eurus/hvec_*        JvecBorn and Hvec of the same
  minizephyr/...                    the same calls of the MiniZephyr problem

The supposition: an Eurus call costs what the MiniZephyr 'full' call costs -- the same solves, one planes or adjoint kernel per item.  The ratios are reported; nothing
here was tuned to them.

Kernels, on an assembled n^2 handle (wall time around the call, launch and stream synchronisation included; `empty_call` is that overhead alone, the same entry point
on a 3 x 3 handle): k_eurus_planes, k_eurus_adjoint (both outputs and each alone) and k_lag_centre_edges beside k_velocity_planes and k_velocity_adjoint.

Factorisation: the first solve of a fresh operator minus its second, for M1 and for M1^T of the tilted model, with the count of fronts handed to the pivoted LU
(the library's HELM_ND_DEBUG line) read from stderr.

Per figure: the median, every time and the run-to-run spread (max - min) / median."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

for _k in ('OPENBLAS_NUM_THREADS', 'OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(_k, '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.bench_fields import job_config, stat

PARAMETERS = ('c', 'rho', 'joint')


def tilted(n):
    'smooth eps == delta in 0.05 .. 0.15 and theta in -0.4 .. 0.4 on the n x n grid'
    z, x = np.meshgrid(np.linspace(0., 1., n), np.linspace(0., 1., n), indexing='ij')
    e = 0.10 + 0.05 * np.sin(2. * np.pi * x) * np.cos(np.pi * z)
    return dict(eps=e, delta=e.copy(), theta=0.4 * np.cos(2. * np.pi * z) * np.sin(np.pi * x))


def routes(cfg, reps):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = dict(cfg)
    sc['c'] = np.ascontiguousarray(np.real(np.asarray(cfg['c'])))
    sc['rho'] = 310. * sc['c'] ** 0.25
    n = int(sc['nz'])
    probs = {}
    for name, extra in (('eurus', dict(Disc=za.Eurus, eurusDerivatives=True, **tilted(n))), ('minizephyr', dict(Disc=za.MiniZephyr))):
        scp = dict(sc, **extra)
        prob, sv = Helm2DProblem(scp), Helm2DSurvey(scp)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        probs[name] = (prob, sv, prob.fieldsDevice())
    N = probs['eurus'][0].nrow
    rng = np.random.default_rng(3)
    nD = probs['eurus'][1].nD
    r = rng.standard_normal(nD) + 1j * rng.standard_normal(nD)
    v = np.concatenate((50. * rng.uniform(-1., 1., N), 40. * rng.uniform(-1., 1., N)))
    vec = {'c': v[:N].copy(), 'rho': v[N:].copy(), 'joint': v}
    calls = {}
    for name, (prob, sv, F) in probs.items():
        for par in PARAMETERS:
            kw = dict(u=F, linearisation='full', parameter=par)
            calls['%s/jtvec_%s' % (name, par)] = lambda prob=prob, kw=kw: prob.Jtvec(None, r, adjoint='transpose', **kw)
            calls['%s/born_%s' % (name, par)] = lambda prob=prob, kw=kw, par=par: prob.JvecBorn(None, vec[par], **kw)
            calls['%s/hvec_%s' % (name, par)] = lambda prob=prob, kw=kw, par=par: prob.Hvec(None, vec[par], **kw)
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
    for what in ('jtvec', 'born', 'hvec'):
        for par in PARAMETERS:
            out['%s_%s_eurus_over_minizephyr' % (what, par)] = out['eurus/%s_%s' % (what, par)]['median_s'] / out['minizephyr/%s_%s' % (what, par)]['median_s']
    g2 = np.concatenate((res['eurus/jtvec_c'], res['eurus/jtvec_rho']))
    out['jtvec_joint_against_two_calls'] = float(np.linalg.norm(res['eurus/jtvec_joint'] - g2) / np.linalg.norm(g2))
    lhs = float(np.real(np.vdot(res['eurus/born_joint'], r)))
    out['adjoint_identity_miss'] = abs(lhs - float(v @ res['eurus/jtvec_joint'])) / abs(lhs)
    return out


def kernels(n, reps):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    rng = np.random.default_rng(5)

    def model(m, cls, **extra):
        return cls(dict(nz=m, nx=m, dx=10., dz=10., nPML=min(10, m - 1), freq=6., c=rng.uniform(2000., 2600., (m, m)), rho=rng.uniform(1800., 2300., (m, m)), device=0,
                        **extra))
    eu, tiny, mz = model(n, za.Eurus, eurusDerivatives=True, **tilted(n)), model(3, za.Eurus, eurusDerivatives=True), model(n, za.MiniZephyr)
    h, ht, hm = eu.handle, tiny.handle, mz.handle
    dev = torch.device('cuda', 0)
    N, nsrc = n * n, 8
    gen = torch.Generator(device=dev).manual_seed(1)
    V = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 0.5
    W = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 0.5
    G = torch.zeros(2 * N, dtype=torch.complex128, device=dev)
    C9 = torch.view_as_complex(torch.randn((9 * N, 2), dtype=torch.float64, device=dev, generator=gen))
    U = torch.view_as_complex(torch.randn((2 * nsrc * N, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    v, w, g, c9, u = (P(t.data_ptr()) for t in (V, W, G, C9, U))
    gb, ub = P(G.data_ptr() + 16 * N), P(U.data_ptr() + 16 * nsrc * N)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts
    ck = lambda rc, hd: _lib.check(rc, hd)
    calls = dict(
        empty_call=lambda: ck(lib.helm_eurus_adjoint_device(ht, c9, 1.0, 0.5, 1, g, None), ht),
        eurus_planes=lambda: ck(lib.helm_eurus_planes_device(h, v, w, c9), h),
        eurus_planes_dc=lambda: ck(lib.helm_eurus_planes_device(h, v, None, c9), h),
        eurus_adjoint_both=lambda: ck(lib.helm_eurus_adjoint_device(h, c9, 1.0, 0.5, 1, g, gb), h),
        eurus_adjoint_c=lambda: ck(lib.helm_eurus_adjoint_device(h, c9, 1.0, 0.5, 1, g, None), h),
        eurus_adjoint_b=lambda: ck(lib.helm_eurus_adjoint_device(h, c9, 1.0, 0.5, 1, None, gb), h),
        lag_centre_edges=lambda: ck(lib.helm_lag_centre_edges_accumulate_device(h, u, N, ub, N, nsrc, c9), h),
        velocity_planes=lambda: ck(lib.helm_velocity_planes_device(hm, v, None, c9), hm),
        velocity_adjoint=lambda: ck(lib.helm_velocity_adjoint_device(hm, c9, 1.0, 0.5, 1, g), hm),
        buoyancy_adjoint=lambda: ck(lib.helm_buoyancy_adjoint_device(hm, c9, 1.0, 0.5, 1, g), hm))
    res = dict(n=n, reps=reps, nsrc_edges=nsrc)
    for name, fn in calls.items():
        res[name] = stat(timed(fn))
    del eu.factors, tiny.factors, mz.factors
    del C9, U
    torch.cuda.empty_cache()
    return res


FACTOR_CHILD = r'''
import json, sys, time
sys.path.insert(0, %(root)r)
import numpy as np
import zephyr_amd as za
from tools.bench_eurus import tilted
from bench import build_config
n = %(n)d
cfg = build_config(n, 10.)
c = np.ascontiguousarray(np.real(np.asarray(cfg['c'])))
sc = dict(nx=n, nz=n, dx=10., dz=10., c=c, rho=310. * c ** 0.25, freq=%(freq)r, nPML=cfg.get('nPML', 10), eurusDerivatives=True, rtol=1e-10, method='direct', device=0,
          transposed=%(transposed)r, **tilted(n))
q = np.zeros((n * n, 4), dtype=np.complex128)
q[(n // 2) * n + n // 3 + np.arange(4) * 7, np.arange(4)] = 1.
out = []
for rep in range(%(reps)d):
    op = za.Eurus(sc)
    op.handle
    t0 = time.perf_counter(); op * q; t1 = time.perf_counter(); op * q; t2 = time.perf_counter()
    out.append(dict(first_s=t1 - t0, second_s=t2 - t1, factor_ms=op.lastTiming()['factor_ms'], relres=max(i['relres'] for i in op.lastInfo)))
    del op.factors
print('RESULT ' + json.dumps(out))
'''


def factorisation(n, reps, freq=8.):
    'the first solve of a fresh operator minus its second, M1 and M1^T, each in a fresh child process with HELM_ND_DEBUG=1; fronts re-eliminated by the pivoted LU'
    res = {}
    for name, tr in (('M1', False), ('M1T', True)):
        code = FACTOR_CHILD % dict(root=ROOT, n=n, freq=freq, transposed=tr, reps=reps)
        p = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HELM_ND_DEBUG='1'), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if p.returncode != 0:
            res[name] = dict(error=p.stderr.decode()[-800:])
            continue
        runs = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith('RESULT ')][-1][7:])
        treated = [int(m) for m in re.findall(r'(\d+) ill-conditioned front\(s\) re-eliminated', p.stderr.decode())]
        res[name] = dict(factor_s=stat([r['first_s'] - r['second_s'] for r in runs[1:] or runs]), first_solve_s=[r['first_s'] for r in runs],
                         worst_relres=max(r['relres'] for r in runs), fronts_re_eliminated=sum(treated), factorisations=len(runs))
    if 'factor_s' in res.get('M1', {}) and 'factor_s' in res.get('M1T', {}):
        res['M1T_over_M1'] = res['M1T']['factor_s']['median_s'] / res['M1']['factor_s']['median_s']
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eurus_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['factorisation'] = factorisation(args.n, 4)
    print(json.dumps({'factorisation': res['factorisation']}, default=float), flush=True)
    res['kernels'] = kernels(args.n, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    cfg = job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec)
    res['routes'] = routes(cfg, args.reps)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
