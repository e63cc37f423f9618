#!/usr/bin/env python3
"""What the stacked (c, rho) routes, parameter='joint', cost against the single-parameter calls they replace, with the forward fields in HBM, at config 4's survey:
bench.py's 512^2 Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr.  Prints one JSON object
and writes it to --out (default profiles/joint_bench.json).

Routes.  One problem with an explicit density (Gardner's formula evaluated once), its store F = fieldsDevice() and the factors of A and A^T resident.  After a
warm-up of each, the calls alternate one by one, `reps` rounds, all in one run:

  jtvec_joint                        Jtvec(u=F, adjoint='transpose', parameter='joint'): one back-solve per item, both transposes on the same lag products
  jtvec_c, jtvec_rho                 the two calls it replaces
  gauss_newton_joint                 Hvec(u=F, parameter='joint'): two solves per item
  gauss_newton_cc, _rc, _cr, _rr     the four block calls it replaces (parameter 'c', ('rho', 'c'), ('c', 'rho'), 'rho'), two solves each
  newton_joint                       Hvec(u=F, parameter='joint', resid=r): three solves per item
  newton_c, newton_rho               the two diagonal blocks that could be had before; the off-diagonal Newton blocks could not

for linearisation='full' and 'operator' and for both formats of the store.  The supposition: a joint call takes about what ONE single-parameter call takes (1, 2
and 3 solves per item), against 2x for two Jtvec calls and 4x for four Gauss-Newton block calls.

Kernels, on an assembled n^2 handle (wall time around the call, launch and stream synchronisation included; `empty_call` is that overhead alone, the same entry point on
a 3 x 3 handle): k_mixed_adjoint and k_velocity_adjoint_b with and without their stretch parts, beside k_buoyancy_adjoint and k_velocity_adjoint, whose gathers they are.

Per figure: the median, every time and the run-to-run spread (max - min) / median.
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

BLOCKS = {'cc': 'c', 'rc': ('rho', 'c'), 'cr': ('c', 'rho'), 'rr': 'rho'}


def routes(cfg, reps, dtype):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = dict(cfg, Disc=za.MiniZephyr, fieldsDtype=dtype)
    sc['rho'] = 310. * np.real(np.asarray(cfg['c'])) ** 0.25
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    N = prob.nrow
    rng = np.random.default_rng(3)
    r = rng.standard_normal(sv.nD) + 1j * rng.standard_normal(sv.nD)
    v = 50. * rng.uniform(-1., 1., 2 * N)
    vc, vr = v[:N].copy(), v[N:].copy()
    half = {'c': vc, 'rho': vr}
    calls = {}
    for lin in ('full', 'operator'):
        kw = dict(u=F, linearisation=lin)
        calls[lin + '/jtvec_joint'] = lambda kw=kw: prob.Jtvec(None, r, adjoint='transpose', parameter='joint', **kw)
        calls[lin + '/gauss_newton_joint'] = lambda kw=kw: prob.Hvec(None, v, parameter='joint', **kw)
        calls[lin + '/newton_joint'] = lambda kw=kw: prob.Hvec(None, v, parameter='joint', resid=r, **kw)
        for par in ('c', 'rho'):
            calls['%s/jtvec_%s' % (lin, par)] = lambda kw=kw, par=par: prob.Jtvec(None, r, adjoint='transpose', parameter=par, **kw)
            calls['%s/newton_%s' % (lin, par)] = lambda kw=kw, par=par: prob.Hvec(None, half[par], parameter=par, resid=r, **kw)
        for name, par in BLOCKS.items():
            pin = par if isinstance(par, str) else par[0]
            calls['%s/gauss_newton_%s' % (lin, name)] = lambda kw=kw, par=par, pin=pin: prob.Hvec(None, half[pin], parameter=par, **kw)
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
    F.release()
    del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    med = lambda name: out[name]['median_s']
    for lin in ('full', 'operator'):
        k = lambda name: '%s/%s' % (lin, name)
        out[k('jtvec_joint_over_jtvec_c')] = med(k('jtvec_joint')) / med(k('jtvec_c'))
        out[k('two_jtvec_over_jtvec_joint')] = (med(k('jtvec_c')) + med(k('jtvec_rho'))) / med(k('jtvec_joint'))
        out[k('gauss_newton_joint_over_gauss_newton_cc')] = med(k('gauss_newton_joint')) / med(k('gauss_newton_cc'))
        out[k('four_blocks_over_gauss_newton_joint')] = sum(med(k('gauss_newton_' + b)) for b in BLOCKS) / med(k('gauss_newton_joint'))
        out[k('newton_joint_over_newton_c')] = med(k('newton_joint')) / med(k('newton_c'))
        out[k('newton_joint_over_gauss_newton_joint')] = med(k('newton_joint')) / med(k('gauss_newton_joint'))
        # what the run computed: the joint products against what the single-parameter calls assemble
        g2 = np.concatenate((res[k('jtvec_c')], res[k('jtvec_rho')]))
        h4 = np.concatenate((res[k('gauss_newton_cc')] + res[k('gauss_newton_rc')], res[k('gauss_newton_cr')] + res[k('gauss_newton_rr')]))
        out[k('jtvec_joint_against_two_calls')] = float(np.linalg.norm(res[k('jtvec_joint')] - g2) / np.linalg.norm(g2))
        out[k('gauss_newton_joint_against_four_blocks')] = float(np.linalg.norm(res[k('gauss_newton_joint')] - h4) / np.linalg.norm(h4))
        out[k('residual_part')] = float(np.linalg.norm(res[k('newton_joint')] - res[k('gauss_newton_joint')]) / np.linalg.norm(res[k('newton_joint')]))
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
    V = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 0.5
    G = torch.zeros(N, dtype=torch.complex128, device=dev)
    C9 = torch.view_as_complex(torch.randn((9 * N, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    v, g, c9 = (P(t.data_ptr()) for t in (V, G, C9))
    ck = lambda rc, hd=h: _lib.check(rc, hd)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts
    calls = dict(
        empty_call=lambda: ck(lib.helm_mixed_adjoint_device(ht, c9, v, 1.0, 0.5, 1, 1, g), ht),
        mixed_adjoint=lambda: ck(lib.helm_mixed_adjoint_device(h, c9, v, 1.0, 0.5, 1, 1, g)),
        mixed_adjoint_mass=lambda: ck(lib.helm_mixed_adjoint_device(h, c9, v, 1.0, 0.5, 1, 0, g)),
        velocity_adjoint_b=lambda: ck(lib.helm_velocity_adjoint_b_device(h, c9, v, 1.0, 0.5, 1, 1, g)),
        velocity_adjoint_b_mass=lambda: ck(lib.helm_velocity_adjoint_b_device(h, c9, v, 1.0, 0.5, 1, 0, g)),
        buoyancy_adjoint=lambda: ck(lib.helm_buoyancy_adjoint_device(h, c9, 1.0, 0.5, 1, g)),
        velocity_adjoint=lambda: ck(lib.helm_velocity_adjoint_device(h, c9, 1.0, 0.5, 1, g)))
    res = dict(n=n, reps=reps)
    for name, fn in calls.items():
        res[name] = stat(timed(fn))
    res['mixed_adjoint_over_buoyancy_adjoint'] = res['mixed_adjoint']['median_s'] / res['buoyancy_adjoint']['median_s']
    res['velocity_adjoint_b_over_velocity_adjoint'] = res['velocity_adjoint_b']['median_s'] / res['velocity_adjoint']['median_s']
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_bench.json'))
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
