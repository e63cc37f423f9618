#!/usr/bin/env python3
"""What the full Newton Hessian-vector product costs with the forward fields in HBM, at config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m), 8
frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr.  Prints one JSON object and writes it to --out (default
profiles/newton_bench.json).

Routes.  One problem with an explicit density (Gardner's formula evaluated once), its store F = fieldsDevice() and the factors of A and A^T resident.  After a
warm-up of each, the calls alternate one by one, `reps` rounds: Hvec(u=F, linearisation='full', resid=r) -- three solves of nsrc columns per frequency --,
Hvec(u=F, linearisation='full') -- the Gauss-Newton product, two solves -- and Jtvec(u=F, adjoint='transpose', linearisation='full') -- one solve -- of the same
run; the same for linearisation='operator' and for parameter='rho'.  With nine repetitions and run-to-run spreads of 3-13 % the ratios are good to about a tenth.

Kernels, on an assembled n^2 handle and nsrc random columns (wall time around the call, launch and stream synchronisation included; `empty_call` is that overhead
alone, the same entry point on a 3 x 3 handle):

  copy_c128                          a device-to-device copy of the complex128 columns, the rate everything is compared with
  stencil_t_c128 / stencil_t_c64     k_stencil_sources_t, the transposed application of nine planes
  stencil_c128 / stencil_c64         k_stencil_sources, the kernel it is modelled on
  curvature / curvature_mass         k_velocity_curvature with and without the stretch part, once per item on N cells (nine planes in)
  velocity_adjoint                   k_velocity_adjoint, the same body with the first derivatives

Per figure: the median, every time, the run-to-run spread (max - min) / median, the bytes the kernel has to move and the rate.
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

PARS = {'c': dict(linearisation='full'), 'operator': dict(linearisation='operator'), 'rho': dict(linearisation='full', parameter='rho')}


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
    rng = np.random.default_rng(3)
    r = rng.standard_normal(sv.nD) + 1j * rng.standard_normal(sv.nD)
    p = 50. * rng.uniform(-1., 1., prob.nrow)
    calls = {}
    for name, kw in PARS.items():
        calls['newton_' + name] = lambda kw=kw: prob.Hvec(None, p, u=F, resid=r, **kw)
        calls['gauss_newton_' + name] = lambda kw=kw: prob.Hvec(None, p, u=F, **kw)
        calls['jtvec_' + name] = lambda kw=kw: prob.Jtvec(None, r, u=F, adjoint='transpose', **kw)
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
    for name in PARS:
        out['newton_over_gauss_newton_' + name] = out['newton_' + name]['median_s'] / out['gauss_newton_' + name]['median_s']
        out['newton_over_jtvec_' + name] = out['newton_' + name]['median_s'] / out['jtvec_' + name]['median_s']
        out['residual_part_' + name] = float(np.linalg.norm(res['newton_' + name] - res['gauss_newton_' + name]) / np.linalg.norm(res['newton_' + name]))
    return out


def kernels(n, nsrc, reps):
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
    U = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    R = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    X = torch.empty(nsrc, dtype=torch.int32, device=dev)
    V = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    G = torch.zeros(N, dtype=torch.complex128, device=dev)
    C9 = torch.view_as_complex(torch.randn((9 * N, 2), dtype=torch.float64, device=dev, generator=gen))
    torch.cuda.synchronize(dev)
    _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(X.data_ptr())), h)
    u, r, p64, x, v, g, c9 = (P(t.data_ptr()) for t in (U, R, P64, X, V, G, C9))
    ck = lambda rc, hd=h: _lib.check(rc, hd)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts

    def copy():
        R.copy_(U)
        torch.cuda.synchronize(dev)
    field = lambda e: (e + 16) * nsrc * N + 144 * N * ((nsrc + 3) // 4)          # (the columns in and out, nine planes per group of four columns)
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        empty_call=(lambda: ck(lib.helm_velocity_curvature_device(ht, c9, v, 1.0, 0.5, 1, 1, g), ht), None),
        stencil_t_c128=(lambda: ck(lib.helm_stencil_sources_t_device(h, u, nsrc, N, c9, 1.0, 0.5, 1, 0, r, N)), field(16)),
        stencil_t_c64=(lambda: ck(lib.helm_stencil_sources_t_c64_device(h, p64, x, nsrc, N, c9, 1.0, 0.5, 1, 0, r, N)), field(8)),
        stencil_c128=(lambda: ck(lib.helm_stencil_sources_device(h, u, nsrc, N, c9, 1.0, 0.5, 1, r, N)), field(16)),
        stencil_c64=(lambda: ck(lib.helm_stencil_sources_c64_device(h, p64, x, nsrc, N, c9, 1.0, 0.5, 1, r, N)), field(8)),
        curvature=(lambda: ck(lib.helm_velocity_curvature_device(h, c9, v, 1.0, 0.5, 1, 1, g)), (144 + 16 + 8 + 8 + 32) * N),
        curvature_mass=(lambda: ck(lib.helm_velocity_curvature_device(h, c9, v, 1.0, 0.5, 1, 0, g)), (144 + 16 + 8 + 8 + 32) * N),
        velocity_adjoint=(lambda: ck(lib.helm_velocity_adjoint_device(h, c9, 1.0, 0.5, 1, g)), (144 + 16 + 8 + 32) * N))
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        st = stat(timed(fn))
        st['bytes'] = nbytes
        if nbytes:
            st['TBps'] = nbytes / st['median_s'] / 1e12
        res[name] = st
    for fmt in ('c128', 'c64'):
        res['stencil_t_over_stencil_' + fmt] = res['stencil_t_' + fmt]['median_s'] / res['stencil_' + fmt]['median_s']
    res['curvature_over_velocity_adjoint'] = res['curvature']['median_s'] / res['velocity_adjoint']['median_s']
    del op.factors, tiny.factors
    del U, R, P64, C9
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'newton_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['kernels'] = kernels(args.n, args.nsrc, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    cfg = job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec)
    res['routes'] = {dt: routes(cfg, args.reps, dt) for dt in ('complex128', 'complex64')}
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
