"""Timings of the 3-D density, joint and Gardner routes on one GPU: config 5 at one eighth (128 x 128 x 64, c = 2000 m/s, h = 10 m, 4 and 5 Hz, 16 sources,
64 receivers), the workload of tools/bench_3d_survey.py.

    python tools/bench_3d_density.py [--reps 5] [--out profiles/3d_density_bench.json]

The calls alternate in one process; medians and spreads (min, max) of `reps` repetitions, each timed by the host clock around a call that ends in a device
synchronise.  Two problems share the process: one with an explicit `rho` ('c', 'rho', 'joint') and one without (the Gardner total derivative), both with
derivatives3D=True, each on its own stored fields.

Suppositions stated before anything was measured:
  1. a 'joint' Jtvec costs one 'c' Jtvec plus the time of the new kernels (k_lap3_imaging and the chain), not two 'c' Jtvecs: there is ONE back-solve per item;
  2. a 'rho' Jtvec costs what a 'c' Jtvec costs (the same solve; one more imaging kernel);
  3. the Gardner 'full' Jtvec costs what the 'joint' Jtvec costs (the same launches, another chain);
and likewise for JvecBorn, whose joint right-hand side is one.  The report says for each whether it held.

The kernels: k_lap3_sources and k_lap3_imaging through their entry points at 128 x 128 x 64 x 16, beside k_mass3_sources, k_mass3_imaging and a device copy of
32 N k bytes in the same run -- the byte count of the store-mode sources kernels; the add mode and the imaging kernels move somewhat more (below), so for them the
copy is only approximately the same bytes, and each kernel's GB/s is formed from its own count.  Algorithmic bytes: sources 16 B read and 16 B written per
cell and column (plus 8 B of B per cell; in add mode 16 B more read); imaging 32 B read per cell and column and 32 B of P per cell.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(x, scale=1.0):
    return dict(median=scale * statistics.median(x), min=scale * min(x), max=scale * max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import zephyr_amd as za
    from zephyr_amd import device_survey3d as d3
    nz, ny, nx, h, nsrc = 64, 128, 128, 10., 16
    freqs = (4., 5.)
    rng = np.random.default_rng(0)
    src = np.stack([rng.uniform(200., 1070., nsrc), rng.uniform(200., 1070., nsrc), np.full(nsrc, 150.)], axis=1)
    gx, gy = np.meshgrid(np.linspace(250., 1020., 8), np.linspace(250., 1020., 8))
    rec = np.stack([gx.ravel(), gy.ravel(), np.full(64, 480.)], axis=1)
    sc = dict(nx=nx, ny=ny, nz=nz, dx=h, c=2000. * np.ones((nz, ny, nx)), rho=1000. * np.ones((nz, ny, nx)), nPML=10, freqs=list(freqs), rtol=1e-8, maxit=20000,
              method='auto', batch=nsrc, geom=dict(src=src, rec=rec, mode='fixed'), parallel=False, derivatives3D=True)
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    scg = {k: v for k, v in sc.items() if k != 'rho'}
    pg, sg = za.Helm3DProblem(scg), za.Helm3DSurvey(scg)
    pg.pair(sg)
    out = dict(geometry='%dx%dx%d, h=%g m, c=2000 m/s, %s Hz, %d sources, %d receivers' % (nx, ny, nz, h, freqs, nsrc, len(rec)), reps=args.reps)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def alternate(calls):
        ts = {k: [] for k in calls}
        for fn in calls.values():
            fn()                                         # every shape warmed, every hierarchy built, outside the timing
        for _ in range(args.reps):
            for k, fn in calls.items():
                ts[k].append(timed(fn))
        return ts

    F, Fg = prob.fieldsDevice(), pg.fieldsDevice()
    N = prob.nrow
    r = rng.standard_normal(sv.nD) + 1j * rng.standard_normal(sv.nD)
    v = rng.standard_normal(2 * N)
    X = dict(adjoint='transpose', linearisation='full')
    ts = alternate({"Jtvec 'c'": lambda: prob.Jtvec(None, r, u=F, **X),
                    "Jtvec 'rho'": lambda: prob.Jtvec(None, r, u=F, parameter='rho', **X),
                    "Jtvec 'joint'": lambda: prob.Jtvec(None, r, u=F, parameter='joint', **X),
                    "Jtvec Gardner 'full'": lambda: pg.Jtvec(None, r, u=Fg, **X),
                    "JvecBorn 'c'": lambda: prob.JvecBorn(None, v[:N], u=F, linearisation='full'),
                    "JvecBorn 'rho'": lambda: prob.JvecBorn(None, v[N:], u=F, linearisation='full', parameter='rho'),
                    "JvecBorn 'joint'": lambda: prob.JvecBorn(None, v, u=F, linearisation='full', parameter='joint'),
                    "JvecBorn Gardner 'full'": lambda: pg.JvecBorn(None, v[:N], u=Fg, linearisation='full'),
                    "Hvec 'joint'": lambda: prob.Hvec(None, v, u=F, linearisation='full', parameter='joint')})
    out['routes_s'] = {k: stats(x) for k, x in ts.items()}
    # the kernels beside a device copy of their algorithmic bytes
    op = prob.system.subProblems[0]
    k = nsrc
    U = torch.randn(k, N, dtype=torch.complex128, device='cuda:0')
    Z = torch.randn(k, N, dtype=torch.complex128, device='cuda:0')
    W = torch.randn(N, dtype=torch.complex128, device='cuda:0')
    B = torch.randn(N, dtype=torch.float64, device='cuda:0')
    R = torch.zeros_like(U)
    P = torch.zeros(N, dtype=torch.complex128, device='cuda:0')
    kern = {'k_lap3_sources (store)': (lambda: d3.lapSourcesDevice(op, U, k, B, 1.0, R, conj=True), N * (k * 32 + 8)),
            'k_lap3_sources (add)': (lambda: d3.lapSourcesDevice(op, U, k, B, 1e-3, R, conj=True, add=True), N * (k * 48 + 8)),
            'k_lap3_imaging': (lambda: d3.lapImagingAccumulateDevice(op, U, Z, k, P, conj=True), N * (k * 32 + 32)),
            'k_mass3_sources': (lambda: d3.massSourcesDevice(op, U, k, W, 1.0, R, conj=True), N * (k * 32 + 16)),
            'k_mass3_imaging': (lambda: d3.massImagingAccumulateDevice(op, U, Z, k, P), N * (k * 32 + 32)),
            'device copy': (lambda: R.copy_(U), N * k * 32)}
    ts = alternate({name: fn for name, (fn, _) in kern.items()})
    out['kernels'] = {name: dict(us=stats(ts[name], 1e6), algorithmic_GBps=kern[name][1] / statistics.median(ts[name]) / 1e9) for name in kern}
    # what held
    m = {name: s['median'] for name, s in out['routes_s'].items()}
    new_kernels = sum(out['kernels'][n]['us']['median'] for n in ('k_lap3_imaging',)) * 1e-6 * len(freqs)
    out['suppositions'] = {
        "joint Jtvec = 'c' Jtvec + the new kernels": dict(joint_s=m["Jtvec 'joint'"], c_s=m["Jtvec 'c'"], new_kernels_s=new_kernels, two_c_s=2 * m["Jtvec 'c'"],
                                                         excess_over_c_s=m["Jtvec 'joint'"] - m["Jtvec 'c'"]),
        "'rho' Jtvec = 'c' Jtvec": dict(rho_s=m["Jtvec 'rho'"], c_s=m["Jtvec 'c'"], ratio=m["Jtvec 'rho'"] / m["Jtvec 'c'"]),
        "Gardner 'full' Jtvec = 'joint' Jtvec": dict(gardner_s=m["Jtvec Gardner 'full'"], joint_s=m["Jtvec 'joint'"], ratio=m["Jtvec Gardner 'full'"] / m["Jtvec 'joint'"]),
        "joint JvecBorn = 'c' JvecBorn + the new kernels": dict(joint_s=m["JvecBorn 'joint'"], c_s=m["JvecBorn 'c'"], ratio=m["JvecBorn 'joint'"] / m["JvecBorn 'c'"])}
    F.release()
    Fg.release()
    del prob.factors, pg.factors
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
