"""Timings of the exact 3-D pseudo-Hessian on one GPU: the workload of tools/bench_3d_density.py (128 x 128 x 64, c = 2000 m/s, h = 10 m, 4 and 5 Hz, 16 sources,
64 receivers).

    python tools/bench_3d_pseudohessian.py [--reps 5] [--out profiles/3d_pseudohessian_bench.json]

The calls alternate in one process; medians and spreads (min, max) of `reps` repetitions, each timed by the host clock around a call that ends in a stream wait
(every entry point waits for its stream; the routes end in the download of their partial).  Two problems share the process: one with an explicit `rho` ('c',
'rho', the blocks) and one without (the Gardner total derivative), both with derivatives3D=True and hessian3D=True, each on its own stored fields.

Suppositions stated before anything was measured:
  (a) k_ph3_moments costs no more than k_lap3_sources in store mode timed in the same run (margin: that run's own spread): it forms the same sum and reads the
      same bytes, and writes 8 N - 24 N bytes instead of 16 N k;
  (b) hessianBlocks costs one 'rho' diagonal plus the extra stores, not three diagonals;
  (c) every exact kind is below a few percent of fieldsDevice of the same run.
The report says for each whether it held.

Recorded beside them: k_energy and a device copy of 16 N k bytes in the same run, the coefficient kernel (once per mode), and per kernel its algorithmic bytes
and the rate they give -- k_ph3_moments 16 B read per cell and column, 40 (blocks: 72) B of coefficient planes and 16 (blocks: 48 + 24) B of H, c and rho per
cell; k_lap3_sources 16 B read and 16 B written per cell and column and 8 B of B per cell; k_energy 16 B per cell and column and 24 B per cell;
k_ph3_coefficients 24 B read per cell and 32 (blocks: 56) B written.
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
              method='auto', batch=nsrc, geom=dict(src=src, rec=rec, mode='fixed'), parallel=False, derivatives3D=True, hessian3D=True)
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

    def alternate(calls, warm=True):
        ts = {k: [] for k in calls}
        if warm:
            for fn in calls.values():
                fn()                                     # every shape warmed, every hierarchy built, outside the timing
        for _ in range(args.reps):
            for k, fn in calls.items():
                ts[k].append(timed(fn))
        return ts

    F, Fg = prob.fieldsDevice(), pg.fieldsDevice()
    N = prob.nrow
    X = dict(kind='pseudoHessian', linearisation='full')

    def fields():
        prob.fieldsDevice().release()
    ts = alternate({'fieldsDevice': fields,
                    "illumination 'scaler'": lambda: prob.illumination(None, u=F, kind='pseudoHessian'),
                    "illumination 'c' (closed form)": lambda: prob.illumination(None, u=F, parameter='c', **X),
                    "illumination 'rho'": lambda: prob.illumination(None, u=F, parameter='rho', **X),
                    "illumination Gardner 'full'": lambda: pg.illumination(None, u=Fg, parameter='c', **X),
                    'hessianBlocks': lambda: prob.hessianBlocks(None, u=F, **X)})
    out['routes_s'] = {k: stats(x) for k, x in ts.items()}
    # the kernels through their entry points, beside a device copy
    op = prob.system.subProblems[0]
    k = nsrc
    U = torch.randn(k, N, dtype=torch.complex128, device='cuda:0')
    R = torch.zeros_like(U)
    B = torch.randn(N, dtype=torch.float64, device='cuda:0')
    W = torch.rand(N, dtype=torch.float64, device='cuda:0')
    H = torch.zeros(3 * N, dtype=torch.float64, device='cuda:0')
    cpl = lambda: torch.zeros(N, dtype=torch.complex128, device='cuda:0')
    rea = lambda: torch.zeros(N, dtype=torch.float64, device='cuda:0')
    planes = [cpl(), rea(), rea(), cpl(), rea()]
    torch.cuda.synchronize()
    d3.ph3CoefficientsDevice(op, 'blocks', *planes)
    kern = {'k_ph3_moments (diagonal)': (lambda: d3.ph3MomentsAccumulateDevice(op, U, k, planes[:3], 0.5, W, H), N * (k * 16 + 40 + 8 + 16)),
            'k_ph3_moments (blocks)': (lambda: d3.ph3MomentsAccumulateDevice(op, U, k, planes, 0.5, None, H, blocks=True, ldh=N), N * (k * 16 + 72 + 48 + 24)),
            'k_lap3_sources (store)': (lambda: d3.lapSourcesDevice(op, U, k, B, 1.0, R, conj=True), N * (k * 32 + 8)),
            'k_energy': (lambda: op.energyAccumulateDevice(U.data_ptr(), k, 0.5, W.data_ptr(), H.data_ptr(), rows=N), N * (k * 16 + 24)),
            'k_ph3_coefficients (buoyancy)': (lambda: d3.ph3CoefficientsDevice(op, 'buoyancy', *planes[:3]), N * (24 + 32)),
            'k_ph3_coefficients (gardner)': (lambda: d3.ph3CoefficientsDevice(op, 'gardner', *planes[:3]), N * (24 + 32)),
            'k_ph3_coefficients (blocks)': (lambda: d3.ph3CoefficientsDevice(op, 'blocks', *planes), N * (24 + 56)),
            'device copy (16 N k bytes)': (lambda: R[:k // 2].copy_(U[:k // 2]), N * k * 16)}
    ts = alternate({name: fn for name, (fn, _) in kern.items()})
    out['kernels'] = {name: dict(us=stats(ts[name], 1e6), algorithmic_bytes=kern[name][1], algorithmic_TBps=kern[name][1] / statistics.median(ts[name]) / 1e12) for name in kern}
    # what held
    m = {name: s['median'] for name, s in out['routes_s'].items()}
    ku = {name: s['us'] for name, s in out['kernels'].items()}
    lap = ku['k_lap3_sources (store)']
    exact = ("illumination 'c' (closed form)", "illumination 'rho'", "illumination Gardner 'full'", 'hessianBlocks')
    out['suppositions'] = {
        '(a) k_ph3_moments <= k_lap3_sources (store), margin the spread of the run': dict(
            moments_diagonal_us=ku['k_ph3_moments (diagonal)'], moments_blocks_us=ku['k_ph3_moments (blocks)'], lap3_sources_store_us=lap,
            held=bool(ku['k_ph3_moments (diagonal)']['median'] <= lap['max'] and ku['k_ph3_moments (blocks)']['median'] <= lap['max'])),
        "(b) hessianBlocks = one 'rho' diagonal plus the extra stores, not three": dict(
            blocks_s=m['hessianBlocks'], rho_s=m["illumination 'rho'"], three_rho_s=3 * m["illumination 'rho'"], ratio=m['hessianBlocks'] / m["illumination 'rho'"],
            held=bool(m['hessianBlocks'] < 2 * m["illumination 'rho'"])),
        '(c) every exact kind below a few percent of fieldsDevice': dict(
            fieldsDevice_s=m['fieldsDevice'], fraction={n: m[n] / m['fieldsDevice'] for n in exact}, held=bool(all(m[n] <= 0.05 * m['fieldsDevice'] for n in exact)))}
    out['not_measured'] = 'a kernel trace (every time includes the launch and the stream wait); the halo traffic from L2; occupancy; k_stencil3 beside the kernels'
    F.release()
    Fg.release()
    del prob.factors, pg.factors
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
