#!/usr/bin/env python3
"""What the exact derivatives of a 2.5-D problem (config key kyDerivatives) cost with the forward fields of every ky in HBM, at config 4's survey as a 2.5-D
problem: bench.py's 512^2 Marmousi-like model (dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, nky = 8, an explicit cmin and an
explicit density (Gardner's formula evaluated once), one GPU.  Prints one JSON object and writes it to --out (default profiles/ky_exact_bench.json).

Routes.  One Helm25DProblem with the factors of every A_ky and A_ky^T resident, its per-ky store FK = fieldsDevice(perKy=True) and its ky-sum store
F = fieldsDevice().  After a warm-up of each, the calls alternate one by one, `reps` rounds, all in one run:

  full_fk/jtvec, born, hvec     Jtvec(adjoint='transpose') / JvecBorn / Hvec with linearisation='full', u=FK
  full_none/...                 the same with u=None (the forward fields of a ky solved into the workspace just before they are used; no store)
  scaler_f/...                  the 'scaler' transposed routes with u=F, the ky-sum store
  fields_per_ky, fields_sum     fieldsDevice(perKy=True) beside fieldsDevice(), each released again

The supposition, stated before the run and resting on no measurement: with the factors resident an exact call costs what the 'scaler' call costs -- both solve
nky k columns per item -- and u=None adds one forward solve set, i.e. about doubles Jtvec and JvecBorn.  The ratios are reported; nothing here was tuned to them.

Also recorded: the size of the per-ky store in both formats beside the ky-sum store.  Per figure: the median, every time and the run-to-run spread
(max - min) / median.  The share of an item's time outside the solves (planes, stencil sources, lag imaging, transposes, zeroing) comes from a kernel trace of this
tool run with --trace-only (one round, no JSON file), kernel tracing only."""
import argparse
import json
import os
import sys
import time

for _k in ('OPENBLAS_NUM_THREADS', 'OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(_k, '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.bench_fields import stat


def job_config(n, dx, nsrc, nfreq, nrec, nky):
    from bench import build_config
    from zephyr_amd import MiniZephyr25D
    cfg = build_config(n, dx)
    c = np.ascontiguousarray(np.real(np.asarray(cfg['c'])))
    src = np.stack([np.linspace(200.0, dx * n - 200.0, nsrc), np.full(nsrc, 20.0)], axis=1)
    rec = np.stack([np.linspace(100.0, dx * n - 100.0, nrec), np.full(nrec, 20.0)], axis=1)
    cfg.update(Disc=MiniZephyr25D, nky=nky, c=c, rho=310. * c ** 0.25, cmin=float(c.min()), freqs=list(np.linspace(3.0, 10.0, nfreq)),
               geom=dict(src=src, rec=rec, mode='fixed'), batch=nsrc, kyDerivatives=True)
    return cfg


def routes(cfg, reps, trace_only=False):
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    probs = {}
    for dtype in ('complex128', 'complex64'):
        sc = dict(cfg, fieldsDtype=dtype)
        prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        probs[dtype] = (prob, sv)
    prob, sv = probs['complex128']
    out = {}
    # the sizes: the per-ky store in both formats beside the ky-sum store
    F64 = probs['complex64'][0].fieldsDevice(perKy=True)
    out['store_bytes_per_ky_complex64'] = int(sum(F64.nbytes.values()))
    F64.release()
    del probs['complex64'][0].factors
    FK, F = prob.fieldsDevice(perKy=True), prob.fieldsDevice()
    out['store_bytes_per_ky_complex128'] = int(sum(FK.nbytes.values()))
    out['store_bytes_ky_sum_complex128'] = int(sum(F.nbytes.values()))
    N, nD = prob.nrow, sv.nD
    rng = np.random.default_rng(3)
    r = rng.standard_normal(nD) + 1j * rng.standard_normal(nD)
    v = 50. * rng.uniform(-1., 1., N)
    T = dict(adjoint='transpose')
    calls = {}
    for name, kw in (('full_fk', dict(u=FK, linearisation='full')), ('scaler_f', dict(u=F)), ('full_none', dict(linearisation='full'))):
        calls[name + '/jtvec'] = lambda kw=kw: prob.Jtvec(None, r, **kw, **T)
        calls[name + '/born'] = lambda kw=kw: prob.JvecBorn(None, v, **kw)
        calls[name + '/hvec'] = lambda kw=kw: prob.Hvec(None, v, **kw)
    calls['fields_per_ky'] = lambda: prob.fieldsDevice(perKy=True).release()
    calls['fields_sum'] = lambda: prob.fieldsDevice().release()
    times, res = {}, {}

    def one_round():
        for name, fn in calls.items():
            t0 = time.perf_counter()
            res[name] = fn()
            times.setdefault(name, []).append(time.perf_counter() - t0)
    one_round()
    if not trace_only:
        times.clear()
        for _ in range(reps):
            one_round()
    FK.release()
    F.release()
    del prob.factors
    out.update({name: stat(ts) for name, ts in times.items()})
    for what in ('jtvec', 'born', 'hvec'):
        out['%s_full_fk_over_scaler_f' % what] = out['full_fk/' + what]['median_s'] / out['scaler_f/' + what]['median_s']
        out['%s_full_none_over_full_fk' % what] = out['full_none/' + what]['median_s'] / out['full_fk/' + what]['median_s']
    out['fields_per_ky_over_sum'] = out['fields_per_ky']['median_s'] / out['fields_sum']['median_s']
    out['u_none_against_fk'] = float(np.linalg.norm(res['full_none/jtvec'] - res['full_fk/jtvec']) / np.linalg.norm(res['full_fk/jtvec']))
    lhs = float(np.real(np.vdot(res['full_fk/born'], r)))
    out['adjoint_identity_miss'] = abs(lhs - float(v @ res['full_fk/jtvec'])) / abs(lhs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--nky', type=int, default=8)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--trace-only', action='store_true', help='one round of every call and no JSON file: what a kernel trace is taken of')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ky_exact_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, nky=args.nky, reps=args.reps,
               supposition='full_fk costs what scaler_f costs (ratio 1); full_none adds one forward solve set (ratio 2 for jtvec and born)')
    res['routes'] = routes(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec, args.nky), args.reps, args.trace_only)
    line = json.dumps(res, default=float)
    print(line)
    if args.out and not args.trace_only:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
