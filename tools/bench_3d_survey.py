"""Timings of the 3-D survey routes on one GPU: config 5 at one eighth (128 x 128 x 64, c = 2000 m/s, h = 10 m, 4 and 5 Hz, 16 sources, 64 receivers).

    python tools/bench_3d_survey.py [--reps 9] [--out profiles/3d_survey_bench.json]

Medians of `reps` alternating repetitions in one run: the transposed solve beside the forward solve (time and iterations per frequency), Jtvec(adjoint='transpose',
linearisation='full', u=F) beside the default Jtvec(u=F), JvecBorn(linearisation='operator', u=F), and k_mass3_sources / k_mass3_imaging at 128 x 128 x 64 x 16 beside a
same-run device copy of the same bytes.  Suppositions stated beforehand: equal iterations of the two solves and a time ratio set by the loss of the on-the-fly
apply; the ratio of the two Jtvec times that of their back-solves, the kernels under a few percent of either.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
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
              method='auto', batch=nsrc, geom=dict(src=src, rec=rec, mode='fixed'), parallel=False)
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    q = sv.getSources()
    q = [q] * len(freqs) if not isinstance(q, list) else q
    out = dict(geometry='%dx%dx%d, h=%g m, c=2000 m/s, %s Hz, %d sources, %d receivers' % (nx, ny, nz, h, freqs, nsrc, len(rec)), reps=args.reps)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    solves = {}
    for i, f in enumerate(freqs):
        ops = {'forward': prob.system.subProblems[i], 'transposed': prob.adjointSystem.subProblems[i]}
        for op in ops.values():
            op * q[i]                                    # set-up and first solve outside the timing
        ts = {k: [] for k in ops}
        for _ in range(args.reps):
            for k, op in ops.items():
                ts[k].append(timed(lambda: op * q[i])[0])
        solves['%g Hz' % f] = {k: dict(median_s=statistics.median(ts[k]), iterations=max(j['iterations'] for j in ops[k].lastInfo)) for k in ops}
    out['solves'] = solves
    F = prob.fieldsDevice()
    r = rng.standard_normal(sv.nD) + 1j * rng.standard_normal(sv.nD)
    v = rng.standard_normal(prob.nrow)
    routes = {'Jtvec default (u=F)': lambda: prob.Jtvec(None, r, u=F),
              "Jtvec transpose/full (u=F)": lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full'),
              "JvecBorn operator (u=F)": lambda: prob.JvecBorn(None, v, u=F, linearisation='operator')}
    ts = {k: [] for k in routes}
    for fn in routes.values():
        fn()
    for _ in range(args.reps):
        for k, fn in routes.items():
            ts[k].append(timed(fn)[0])
    out['routes_s'] = {k: statistics.median(x) for k, x in ts.items()}
    # the kernels beside a device copy of their algorithmic bytes
    op = prob.system.subProblems[0]
    N, k = op.nrow, nsrc
    U = torch.randn(k, N, dtype=torch.complex128, device='cuda:0')
    B = torch.randn(k, N, dtype=torch.complex128, device='cuda:0')
    W = torch.randn(N, dtype=torch.complex128, device='cuda:0')
    R = torch.empty_like(U)
    P = torch.zeros(N, dtype=torch.complex128, device='cuda:0')
    kern = {'k_mass3_sources': (lambda: d3.massSourcesDevice(op, U, k, W, 1.0, R, conj=True), N * k * 32),
            'k_mass3_imaging': (lambda: d3.massImagingAccumulateDevice(op, U, B, k, P), N * (k * 32 + 16)),
            'device copy': (lambda: R.copy_(U), N * k * 32)}
    ts = {name: [] for name in kern}
    for fn, _ in kern.values():
        fn()
    for _ in range(args.reps):
        for name, (fn, _) in kern.items():
            ts[name].append(timed(fn)[0])
    out['kernels'] = {name: dict(median_us=1e6 * statistics.median(ts[name]), algorithmic_GBps=kern[name][1] / statistics.median(ts[name]) / 1e9) for name in kern}
    F.release()
    del prob.factors
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
