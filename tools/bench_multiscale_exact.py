#!/usr/bin/env python3
"""What the exact derivatives of a multiscale pairing (config key multiscaleDerivatives) cost, at the bench's workload: bench.py's 1024^2 Marmousi-like model
(dx = 9 m), 16 frequencies 2 .. 9.5 Hz, 256 sources, a fixed line of 128 receivers, cMin = 1500 m/s, targetGPW = 8, an explicit density (Gardner's formula
evaluated once), MiniZephyr operators, one GPU.  Prints one JSON object and writes it to --out (default profiles/multiscale_exact_bench.json).

Routes.  Per pairing one Helm2DProblem with the factors of every A_f and A_f^T resident and its store F = fieldsDevice().  After a warm-up of each, the calls of
a pairing alternate one by one, `reps` rounds, in one run; the multiscale pairing runs first and is released before the fixed-grid one (the two sets of factors
and stores of the fixed grid alone take most of the device):

  multiscale/jtvec, born, hvec   Jtvec(adjoint='transpose') / JvecBorn / Hvec with linearisation='full', u=F, on MultiGridMultiFreq + Helm2DMultiGridSurvey
  multiscale/mux_jtvec           the reference's mux Jtvec of the same pairing (forward and back-propagated columns solved together, factors resident)
  multiscale/fields              fieldsDevice(), released again; the size of the store
  fixed/...                      the same calls on MultiFreq + Helm2DSurvey of the same model (a MemoryError there is recorded, not raised).  Its store and its
                                 two sets of factors take most of the device, so it is run in a process of its own (`--only fixed`, merged into the same file);
                                 `--fields-dtype complex64` halves its store where complex128 does not fit, and the record says which format was timed

  transfer: 256 fields through the transposed plan at 1024^2 <- 468^2 and at the integer scale 4 (1024^2 <- 256^2), beside the forward transfer of the same plan
            pair and a device copy of the transposed transfer's bytes in the same run.

The supposition, stated before the run and resting on no measurement: an exact multiscale call costs what the mux multiscale call costs per solved column --
Jtvec(u=F) and JvecBorn solve nsrc columns per frequency, the mux call 2 nsrc, Hvec 2 nsrc -- and the transposed transfers are below a few percent of it.  The
ratios are reported; nothing here was tuned to them.  Per figure: the median, every time and the run-to-run spread (max - min) / median."""
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


def job_config(n, dx, gpw, nsrc, nfreq):
    from tools.bench_multiscale import job_config as base
    cfg = base(n, dx, gpw, nsrc, nfreq)
    c = np.ascontiguousarray(np.real(np.asarray(cfg['c'])))
    cfg.update(c=c, rho=310. * c ** 0.25, multiscaleDerivatives=True)
    return cfg


def pairing_leg(cfg, multiscale, reps, dtype='complex128'):
    from zephyr_amd import MultiFreq, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    W, S = (MultiGridMultiFreq, Helm2DMultiGridSurvey) if multiscale else (MultiFreq, Helm2DSurvey)
    prob, sv = Helm2DProblem(dict(cfg, SystemWrapper=W, fieldsDtype=dtype)), S(cfg)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    out = dict(fieldsDtype=dtype, grids=[list(map(int, (s.nz, s.nx))) for s in prob.system.subProblems])
    F = prob.fieldsDevice()
    out['store_bytes'] = int(sum(F.nbytes.values()))
    N, nD = prob.nrow, sv.nD
    rng = np.random.default_rng(3)
    r = rng.standard_normal(nD) + 1j * rng.standard_normal(nD)
    v = 50. * rng.uniform(-1., 1., N)
    kw = dict(u=F, linearisation='full')
    calls = {'jtvec': lambda: prob.Jtvec(None, r, adjoint='transpose', **kw), 'born': lambda: prob.JvecBorn(None, v, **kw), 'hvec': lambda: prob.Hvec(None, v, **kw),
             'mux_jtvec': lambda: prob.Jtvec(None, r), 'fields': lambda: prob.fieldsDevice().release()}
    times, res = {}, {}

    def one_round():
        for name, fn in calls.items():
            t0 = time.perf_counter()
            res[name] = fn()
            times.setdefault(name, []).append(time.perf_counter() - t0)
    try:
        one_round()
        times.clear()
        for _ in range(reps):
            one_round()
        out.update({name: stat(ts) for name, ts in times.items()})
        lhs = float(np.real(np.vdot(res['born'], r)))
        out['adjoint_identity_miss'] = abs(lhs - float(v @ res['jtvec'])) / abs(lhs)
    finally:
        F.release()
        del prob.factors
    return out


def transfer_leg(reps, k=256):
    import torch
    from zephyr_amd.interpolation import SplineGridInterpolator
    dev = torch.device('cuda', 0)
    out = {}
    for name, scale in (('468', 1024 / 468.), ('integer4', 4.)):
        ds = SplineGridInterpolator(dict(nx=1024, nz=1024, dx=9., dz=9., scale=scale, device=0))
        N, Nf = ds.adjoint.shape
        fine = torch.randn((k, N), dtype=torch.complex128, device=dev)
        coarse = torch.randn((k, Nf), dtype=torch.complex128, device=dev)
        spare = torch.empty_like(fine)
        calls = {'transposed': lambda: ds.adjoint.apply_device(coarse, fine, k=k), 'forward': lambda: ds.apply_device(fine, coarse, k=k),
                 'copy': lambda: (spare.copy_(fine), torch.cuda.synchronize(dev))}
        times = {}
        for rep in range(reps + 1):
            for what, fn in calls.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                if rep:
                    times.setdefault(what, []).append(time.perf_counter() - t0)
        leg = {what: stat(ts) for what, ts in times.items()}
        leg.update(fields=k, coarse=[int(ds.snz), int(ds.snx)], bytes_moved=16 * k * (N + Nf), copy_bytes=2 * 16 * k * N)
        leg['transposed_GBps'] = leg['bytes_moved'] / leg['transposed']['median_s'] / 1e9
        leg['forward_GBps'] = leg['bytes_moved'] / leg['forward']['median_s'] / 1e9
        leg['copy_GBps'] = leg['copy_bytes'] / leg['copy']['median_s'] / 1e9
        out[name] = leg
        del fine, coarse, spare
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--dx', type=float, default=9.)
    ap.add_argument('--gpw', type=float, default=8.)
    ap.add_argument('--nsrc', type=int, default=256)
    ap.add_argument('--nfreq', type=int, default=16)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--only', choices=['all', 'transfer', 'multiscale', 'fixed'], default='all')
    ap.add_argument('--fields-dtype', default='complex128', help='the store format of the fixed-grid leg')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiscale_exact_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nfreq=args.nfreq, targetGPW=args.gpw, cMin=1500., reps=args.reps,
               supposition='per solved column an exact multiscale call costs what the mux multiscale call costs (jtvec and born 0.5, hvec 1.0 of mux_jtvec); the '
                           'transposed transfers are below a few percent of it')
    if args.only != 'all' and args.out and os.path.exists(args.out):          # (a leg run in a process of its own joins the record of the others)
        with open(args.out) as f:
            old = json.loads(f.read())
        if all(old.get(k) == res[k] for k in ('n', 'dx', 'nsrc', 'nfreq', 'targetGPW', 'reps')):
            res = old
    cfg = job_config(args.n, args.dx, args.gpw, args.nsrc, args.nfreq)
    if args.only in ('all', 'transfer'):
        res['transfer'] = transfer_leg(args.reps)
        print(json.dumps(dict(transfer=res['transfer']), default=float), flush=True)
    if args.only in ('all', 'multiscale'):
        res['multiscale'] = pairing_leg(cfg, True, args.reps)
        print(json.dumps(dict(multiscale=res['multiscale']), default=float), flush=True)
    if args.only in ('all', 'fixed'):
        try:
            res['fixed'] = pairing_leg(cfg, False, args.reps, args.fields_dtype)
        except MemoryError as e:
            res['fixed'] = dict(fieldsDtype=args.fields_dtype, error='MemoryError: %s' % (e,))
    if 'multiscale' in res and 'mux_jtvec' in res['multiscale']:
        ms = res['multiscale']
        for what in ('jtvec', 'born', 'hvec'):
            ms[what + '_over_mux_jtvec'] = ms[what]['median_s'] / ms['mux_jtvec']['median_s']
            if what in res.get('fixed', {}):
                res[what + '_fixed_over_multiscale'] = res['fixed'][what]['median_s'] / ms[what]['median_s']
        if 'fields' in res.get('fixed', {}):
            res['fields_fixed_over_multiscale'] = res['fixed']['fields']['median_s'] / ms['fields']['median_s']
            res['store_fixed_over_multiscale'] = res['fixed']['store_bytes'] / ms['store_bytes']
        if 'transfer' in res:
            # one transposed transfer (k = 1) per item: 1 / 256 of the 256-field figure per frequency, against the Jtvec call
            res['transposed_share_of_jtvec_upper'] = args.nfreq * res['transfer']['468']['transposed']['median_s'] / 256. / ms['jtvec']['median_s']
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
