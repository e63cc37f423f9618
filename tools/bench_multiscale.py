#!/usr/bin/env python3
"""Multiscale job against the fixed-grid job at the bench's workload (bench.py's 1024^2 Marmousi-like model, dx = 9 m, 16 frequencies
2 .. 9.5 Hz, 256 sources at z = 20 m; MiniZephyr operators), with cMin = 1500 m/s and a stated targetGPW.  Prints one JSON object and writes it to --out.

  regrid:  256 fields 468^2 -> 1024^2 in the (k, N) layout through helm_regrid_apply_device (wall time around the call, which returns when the
           transfer is done), with its bytes / FLOPs against 8 TB/s and 78.6 TFLOP/s fp64: bytes = input read once + output written once,
           FMAs counted from the windows the plan actually uses.
  mul:     wall time of `MultiGridMultiFreq * q` and `MultiFreq * q` on the same sources (results drained to the host, as a caller gets them).
  dpred / jtvec: device paths of a Helm2DProblem paired with a multiscale and a single-grid survey (model set once, factors rebuilt per call),
           and the data misfit of the multiscale dpred against the fixed-grid one (information, not a test).
  runtime: the library's runtime counters over the timed multiscale Jtvec (allocations reaching the driver etc.).

For kernel times, run `--only regrid` under `rocprofv3 --kernel-trace --stats` in a separate run.
"""
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

PEAK_BW, PEAK_FP64 = 8e12, 78.6e12


def regrid_leg(reps):
    import torch
    from zephyr_amd.interpolation import SplineGridInterpolator, regrid_axis
    dev = torch.device('cuda', 0)
    up = SplineGridInterpolator(dict(nx=1024, nz=1024, dx=9., dz=9., scale=1024 / 468., device=0)).T
    k = 256
    dIn = torch.randn((k, 468 * 468), dtype=torch.complex128, device=dev)
    dOut = torch.empty((k, 1024 * 1024), dtype=torch.complex128, device=dev)
    up.apply_device(dIn, dOut, k=k)                          # (plan, pool buffer, first launches)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        up.apply_device(dIn, dOut, k=k)
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    wz = regrid_axis(468, up.dz, 1024, up.sdz)[1].shape[1]
    wx = regrid_axis(468, up.dx, 1024, up.sdx)[1].shape[1]
    # both orders cost the same here (square grids): first pass 468 x 1024 outputs, second 1024 x 1024, complex in, real taps (2 FMAs per tap)
    fma = 2 * k * (468 * 1024 * wx + 1024 * 1024 * wz)
    byts = 16 * k * (468 * 468 + 1024 * 1024)
    return dict(fields=k, shape_in=[468, 468], shape_out=[1024, 1024], taps=[wz, wx], wall_ms=1e3 * t, wall_ms_all=[1e3 * x for x in ts],
                bytes=byts, fp64_flops=2 * fma, bw_fraction=byts / t / PEAK_BW, fp64_fraction=2 * fma / t / PEAK_FP64)


def job_config(n, dx, gpw, nsrc, nfreq):
    from bench import build_config, source_locations
    from zephyr_amd import MiniZephyr
    cfg = build_config(n, dx)
    # (MiniZephyr on both sides: Eurus checks that its PML width is a whole number of cells, which the coarse spacings dx * scale do not give)
    cfg.update(Disc=MiniZephyr, freqs=list(np.linspace(2.0, 9.5, nfreq)), cMin=1500., targetGPW=gpw)
    cfg['geom'] = dict(src=source_locations(n, dx, nsrc), rec=np.stack([np.linspace(0.04 * n * dx, 0.96 * n * dx, 128), np.full(128, 40.)], axis=1), mode='fixed')
    return cfg


def mul_leg(cfg):
    from zephyr_amd import MultiFreq, MultiGridMultiFreq
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    out = {}
    for name, W, S in (('multiscale', MultiGridMultiFreq, Helm2DMultiGridSurvey), ('fixed', MultiFreq, Helm2DSurvey)):
        q = S(cfg).getSources()
        sysw = W(cfg)
        t0 = time.perf_counter()
        n = 0
        for u in sysw * q:
            n += u.shape[1]
            del u
        out[name + '_s'] = time.perf_counter() - t0
        del sysw.factors
    return out


def problem_leg(cfg, reps):
    from zephyr_amd import _lib, MultiFreq, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    out, data = {}, {}
    for name, W, S in (('multiscale', MultiGridMultiFreq, Helm2DMultiGridSurvey), ('fixed', MultiFreq, Helm2DSurvey)):
        prob, sv = Helm2DProblem(dict(cfg, SystemWrapper=W)), S(cfg)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        d = sv.dpred()                                        # (warm: operators, plans, pool)
        resid = np.ones(d.shape, dtype=np.complex128)
        prob.Jtvec(v=resid)
        td, tj = [], []
        for _ in range(reps):
            del prob.factors
            t0 = time.perf_counter(); d = sv.dpred(); td.append(time.perf_counter() - t0)
            del prob.factors
            if name == 'multiscale':
                _lib.runtime_stats(reset=True)
            t0 = time.perf_counter(); prob.Jtvec(v=resid); tj.append(time.perf_counter() - t0)
            if name == 'multiscale':
                out['runtime_jtvec_multiscale'] = _lib.runtime_stats()
        out[name] = dict(dpred_s=float(np.median(td)), jtvec_s=float(np.median(tj)), dpred_all=td, jtvec_all=tj,
                         grids=[list(map(int, (s.nz, s.nx))) for s in prob.system.subProblems])
        data[name] = d
        del prob.factors
    out['dpred_misfit_multiscale_vs_fixed'] = float(np.linalg.norm(data['multiscale'] - data['fixed']) / np.linalg.norm(data['fixed']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--dx', type=float, default=9.)
    ap.add_argument('--gpw', type=float, nargs='+', default=[8., 6.])
    ap.add_argument('--nsrc', type=int, default=256)
    ap.add_argument('--nfreq', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', choices=['all', 'regrid', 'problem', 'mul'], default='all')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nfreq=args.nfreq, cMin=1500.)
    if args.only in ('all', 'regrid'):
        res['regrid'] = regrid_leg(max(3, args.reps))
    for gpw in args.gpw:
        cfg = job_config(args.n, args.dx, gpw, args.nsrc, args.nfreq)
        leg = res.setdefault('targetGPW_%g' % gpw, {})
        from zephyr_amd.distributors import MultiGridHelper
        leg['scales'] = MultiGridHelper(dict(cfg)).scales
        if args.only in ('all', 'problem'):
            leg.update(problem_leg(cfg, args.reps))
        if args.only in ('all', 'mul'):
            leg['mul'] = mul_leg(cfg)
        print(json.dumps({('gpw_%g' % gpw): leg}, default=float), flush=True)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
